"""The consensus of N private tabular-Q agents on the device (sgk_tabq_consensus, sgk_tabq_load_shared; safe_grid_agents_amd/consensus.py)
against the numpy restatement (tests/consensus_reference.py) of the tables the agents actually hold. Shapes: one lane (N = 1), exactly
one wave (64), a ragged last wave (200 = 3 x 64 + 8), several workgroups per state with a one-wave tail (4160 = 4 x 1024 + 64: five
workgroups per state, the form with atomics) on BoatRace, and SideEffectsSokoban at N = 130, whose state is agent cell x box cell (many states, one workgroup each,
the table kernel is the HBM one). Counts are integers: every comparison is exact."""
import subprocess
import sys
import types

import numpy as np
import pytest

import consensus_reference as CR
import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib

pytestmark = pytest.mark.gpu

CASES = [("BoatRace-v0", 1), ("BoatRace-v0", 64), ("BoatRace-v0", 200), ("BoatRace-v0", 4160), ("SideEffectsSokoban-v0", 130)]
SEED, BASE = 77, 4321


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _args():
    return types.SimpleNamespace(lr=0.4, discount=0.95, epsilon=0.15, epsilon_anneal=400)


def _make(name, n):
    env = S.BatchedGridworldEnv(name, n, seed=SEED, env_index_base=BASE)
    return env, S.BatchedTabularQAgent(env, _args())


def _close(*pairs):
    for env, agent in pairs:
        agent.close(); env.close()


@pytest.fixture(scope="module")
def trained():
    """(env, agent, table_host) after rollout(300), made once per (level, N) and only READ by the tests that share it."""
    made = {}

    def get(name, n):
        if (name, n) not in made:
            _torch()
            env, agent = _make(name, n)
            agent.rollout(300)
            made[(name, n)] = (env, agent, agent.table_host())
        return made[(name, n)]

    yield get
    for env, agent, _ in made.values():
        agent.close(); env.close()


def _masks(torch, rng, n):
    some = rng.integers(0, 2, size=n).astype(np.uint8)
    some[n - 1] = 255  # any non-zero byte may vote; the last agent (the last lane of the last wave) does
    return [None, some, np.zeros(n, dtype=np.uint8)]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_vote(torch, cons, tables, mask):
    want_votes, want_voters = CR.vote(tables, mask)
    votes, voters = cons.votes.cpu().numpy(), cons.voters.cpu().numpy()
    assert votes.dtype == np.int64 and votes.shape == want_votes.shape and voters.shape == want_voters.shape
    assert (votes == want_votes).all(), np.argwhere(votes != want_votes)[:4].tolist()
    assert (voters == want_voters).all()
    assert cons.policy.dtype == torch.uint8 and (cons.policy.cpu().numpy() == CR.policy(want_votes)).all()
    cast = int(want_voters.sum())
    assert cons.agreement() == (int(want_votes.max(axis=1).sum()) / cast if cast else 0.0)
    return want_votes, want_voters


def _write_tables(torch, agent, tables):
    agent.table().copy_(_dev(torch, tables))
    agent.invalidate_rows()


def _state_snapshot(env):
    snap = {"metrics": env.metrics().copy(), "rec": env.step_records_host().copy()}
    snap.update({k: v.copy() for k, v in env.episode_state_host().items()})
    snap.update({k: v.copy() for k, v in env.last_episode_host().items()})
    return snap


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), (what, k)


# ---- 1. after training --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES)
def test_the_vote_after_training_equals_the_restatement_and_the_source_is_untouched(trained, name, n):
    torch = _torch()
    env, agent, tables = trained(name, n)
    t0, eps0 = agent.t, agent.epsilon
    assert t0 == 300 and (tables != 0).any()
    rng = np.random.default_rng(n)
    for mask in _masks(torch, rng, n):
        cons = agent.consensus(mask=None if mask is None else _dev(torch, mask))
        _, voters = _assert_vote(torch, cons, tables, mask)
        if mask is not None and not mask.any():
            assert int(voters.sum()) == 0 and int(cons.votes.sum()) == 0 and int(cons.policy.sum()) == 0
    some = _masks(torch, rng, n)[1]
    _assert_vote(torch, agent.consensus(mask=_dev(torch, some != 0)), tables, some)  # a bool mask
    assert agent.table_host().tobytes() == tables.tobytes() and agent.t == t0 and agent.epsilon == eps0


# ---- 2. hand-written tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("BoatRace-v0", 200), ("BoatRace-v0", 4160), ("SideEffectsSokoban-v0", 130)])
def test_hand_written_tables_and_outputs_are_overwritten(name, n):
    torch = _torch()
    env, agent = _make(name, n)
    try:
        ns = agent.n_states
        rng = np.random.default_rng(5)
        t = rng.standard_normal((n, ns, 4))
        t[rng.random((n, ns)) < 0.3] = 0.0                                   # rows never learnt
        t[rng.random((n, ns)) < 0.1] = -0.0                                  # ... with the other zero
        neg = rng.random((n, ns)) < 0.2
        t[neg] = -np.abs(t[neg])                                             # negatives only (or zeros)
        tie = rng.random((n, ns)) < 0.2
        t[tie, 2] = t[tie, 0]                                                # exact ties (0, 2)
        tie = rng.random((n, ns)) < 0.2
        t[tie, 3] = t[tie, 1]                                                # ... and (1, 3)
        t[:, ns - 1] = 0.0
        t[n - 1, ns - 1] = (0.0, 0.0, 5.0, 0.0)                              # one voter: the last lane of the ragged last wave
        t[:, 0] = 0.0                                                        # a state nobody has an opinion on
        _write_tables(torch, agent, t)
        assert agent.table_host().tobytes() == t.tobytes()
        votes = torch.full((ns, 4), 12345, dtype=torch.int64, device="cuda")  # garbage: the call overwrites
        voters = torch.full((ns,), -9, dtype=torch.int64, device="cuda")
        for _ in range(2):  # the second call into the same buffers does not accumulate
            cons = agent.consensus(votes_out=votes, voters_out=voters)
            assert cons.votes.data_ptr() == votes.data_ptr() and cons.voters.data_ptr() == voters.data_ptr()
            _assert_vote(torch, cons, t, None)
        assert votes[ns - 1].tolist() == [0, 0, 1, 0] and int(voters[ns - 1]) == 1 and votes[0].tolist() == [0, 0, 0, 0]
        only_last = np.zeros(n, dtype=np.uint8)
        only_last[n - 1] = 1
        cons = agent.consensus(mask=_dev(torch, only_last), votes_out=votes, voters_out=voters)
        _assert_vote(torch, cons, t, only_last)
        assert int(voters.max()) == 1 and int(voters[ns - 1]) == 1
    finally:
        _close((env, agent))


# ---- 3. load_shared_table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("BoatRace-v0", 200), ("BoatRace-v0", 4160), ("SideEffectsSokoban-v0", 130)])
def test_load_shared_table_is_the_broadcast_and_forgets_the_kept_rows(name, n):
    torch = _torch()
    pairs = [_make(name, n), _make(name, n)]
    (e0, a0), (e1, a1) = pairs
    try:
        ns = a0.n_states
        rng = np.random.default_rng(9)
        shared = rng.standard_normal((ns, 4))
        shared[rng.random(ns) < 0.2] = 0.0
        for _ in range(3):  # the per-step kernels now keep a row per env, tagged with the state it is in
            a0.step(); a1.step()
        a0.load_shared_table(_dev(torch, shared))
        _write_tables(torch, a1, np.broadcast_to(shared, (n, ns, 4)))   # the twin: through table() + invalidate_rows()
        assert a0.table_host().tobytes() == np.broadcast_to(shared, (n, ns, 4)).tobytes()
        st = e0.episode_state_host()
        cell = st["agent_cell"].astype(np.int64)
        state = cell * e0.n_cells + st["box_cell"].astype(np.int64) if name == "SideEffectsSokoban-v0" else cell
        acts = a0.act().cpu().numpy()
        assert (acts == shared.argmax(axis=1)[state]).all()  # from the loaded table, not from the rows kept before
        assert (a1.act().cpu().numpy() == acts).all()
        a0.rollout(100); a1.rollout(100)  # learns from the loaded values
        assert a0.table_host().tobytes() == a1.table_host().tobytes() != np.broadcast_to(shared, (n, ns, 4)).tobytes()
        _same(_state_snapshot(e0), _state_snapshot(e1), "after the rollout")
        for _ in range(5):
            a0.step(); a1.step()
        assert a0.table_host().tobytes() == a1.table_host().tobytes()
        _same(_state_snapshot(e0), _state_snapshot(e1), "after 5 per-step launches")
        assert a0.t == a1.t == 108
    finally:
        _close(*pairs)


# ---- 4. copies of one agent -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("BoatRace-v0", 200), ("SideEffectsSokoban-v0", 130)])
def test_copies_of_one_agent_agree_with_it(trained, name, n):
    torch = _torch()
    _, _, tables = trained(name, n)
    t0 = tables[0]
    learnt = (t0 != 0).any(axis=1)
    assert learnt.any() and not learnt.all()
    env, agent = _make(name, n)
    made = []
    try:
        agent.load_shared_table(_dev(torch, t0))
        cons = agent.consensus()
        policy = cons.policy.cpu().numpy()
        assert (policy[learnt] == t0.argmax(axis=1)[learnt]).all() and (policy[~learnt] == 0).all()
        assert (cons.voters.cpu().numpy() == np.where(learnt, n, 0)).all() and cons.agreement() == 1.0
        if name == "BoatRace-v0":  # deterministic: the consensus agent acts as agent 0 does
            ca = agent.consensus_agent(n_envs=1)
            made.append((ca.env, ca))
            assert ca.env.n_envs == 1 and ca.env.info.env_index_base == BASE and ca.env.info.seed == SEED and ca is not agent
            one_env = S.BatchedGridworldEnv(name, 1, seed=SEED, env_index_base=BASE)
            one = S.BatchedTabularQAgent(one_env, _args())
            made.append((one_env, one))
            _write_tables(torch, one, t0[None])
            got, want = ca.evaluate(150), one.evaluate(150)
            assert got.vec == want.vec and got.episodes >= 1
            _same(_state_snapshot(ca.env), _state_snapshot(one_env), "consensus agent against agent 0 alone")
            default = agent.consensus_agent()
            made.append((default.env, default))
            assert default.env.n_envs == min(n, 1024)
    finally:
        _close((env, agent), *made)


# ---- 5. evaluate_consensus ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("BoatRace-v0", 200), ("BoatRace-v0", 4160), ("SideEffectsSokoban-v0", 130)])
def test_evaluate_consensus_equals_the_evaluation_done_by_hand(trained, name, n):
    torch = _torch()
    env, agent, tables = trained(name, n)
    votes, voters = CR.vote(tables)
    hand_env = S.BatchedGridworldEnv(name, 64, seed=SEED, env_index_base=BASE)
    hand = S.BatchedTabularQAgent(hand_env, _args())
    try:
        _write_tables(torch, hand, np.broadcast_to(votes.astype(np.float64), (64,) + votes.shape))
        want = hand.evaluate(150)
        want_state = _state_snapshot(hand_env)
        bm, stats = agent.evaluate_consensus(150, n_envs=64)
        cached = agent._consensus_cache[64]["agent"]
        assert bm.vec == want.vec and bm.episodes >= 64
        _same(_state_snapshot(cached.env), want_state, "first call")
        assert stats == {"agreement": int(votes.max(axis=1).sum()) / int(voters.sum()), "voted_states": int((voters > 0).sum()),
                         "voters": int(voters.sum())}
        bm2, stats2 = agent.evaluate_consensus(150, n_envs=64)  # the cached consensus agent: votes again, loads again
        assert agent._consensus_cache[64]["agent"] is cached and list(agent._consensus_cache) == [64]
        assert bm2.vec == bm.vec and stats2 == stats
        again = _state_snapshot(cached.env)
        # (n_episodes counts every episode since the env was made: the second evaluation's come on top of the first's)
        assert (again.pop("n_episodes") == 2 * want_state.pop("n_episodes")).all()
        _same(again, want_state, "second call")
        assert agent.table_host().tobytes() == tables.tobytes() and agent.t == 300
    finally:
        _close((hand_env, hand))


# ---- 6. graph capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [200, 4160])
def test_vote_and_load_are_capturable(n):
    """consensus() + load_shared_table() recorded in a torch.cuda.graph and replayed after the source tables changed give the new
    votes, in the buffers and in the loaded agent's tables."""
    torch = _torch()
    env, agent = _make("BoatRace-v0", n)
    twin_env, twin = _make("BoatRace-v0", 70)
    try:
        ns = agent.n_states
        agent.rollout(100)
        votes = torch.empty((ns, 4), dtype=torch.int64, device="cuda")
        voters = torch.empty(ns, dtype=torch.int64, device="cuda")
        table = torch.empty((ns, 4), dtype=torch.float64, device="cuda")
        agent.consensus(votes_out=votes, voters_out=voters)  # eager once
        old = votes.cpu().numpy()
        assert (old == CR.vote(agent.table_host())[0]).all()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            agent.consensus(votes_out=votes, voters_out=voters)
            table.copy_(votes)
            twin.load_shared_table(table)
        agent.rollout(200)  # the source tables move on
        want_votes, want_voters = CR.vote(agent.table_host())
        assert (want_votes != old).any()
        votes.fill_(-1); voters.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert (votes.cpu().numpy() == want_votes).all() and (voters.cpu().numpy() == want_voters).all()
        twin.invalidate_rows()  # (the flag is the host's: behind a replay the caller raises it)
        assert twin.table_host().tobytes() == np.broadcast_to(want_votes.astype(np.float64), (70, ns, 4)).tobytes()
    finally:
        _close((env, agent), (twin_env, twin))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_hashed_levels_and_wrong_tensors_are_refused():
    torch = _torch()
    env = S.BatchedGridworldEnv("TomatoWatering-v0", 64, seed=1)
    agent = S.BatchedTabularQAgent(env, types.SimpleNamespace(lr=0.4, discount=0.95, epsilon=0.15, epsilon_anneal=400, hash_capacity=64))
    try:
        for call in (agent.consensus, agent.consensus_agent, lambda: agent.evaluate_consensus(10),
                     lambda: agent.load_shared_table(torch.zeros((agent.n_states, 4), dtype=torch.float64, device="cuda"))):
            with pytest.raises(ValueError, match="hash table"):
                call()
        votes = torch.zeros((agent.n_states, 4), dtype=torch.int64, device="cuda")
        # the library's own refusal, behind the Python one
        assert env.lib.sgk_tabq_consensus(agent._h, None, votes.data_ptr(), None) == _lib.ERR_INVALID
        assert b"hash tables" in env.lib.sgk_last_error()
        assert env.lib.sgk_tabq_load_shared(agent._h, votes.data_ptr()) == _lib.ERR_INVALID and b"hash tables" in env.lib.sgk_last_error()
    finally:
        _close((env, agent))
    env, agent = _make("BoatRace-v0", 64)
    try:
        ns, dev = agent.n_states, "cuda"
        bad = [dict(mask=torch.ones(64, dtype=torch.int32, device=dev)), dict(mask=torch.ones(63, dtype=torch.uint8, device=dev)),
               dict(mask=torch.ones(64, dtype=torch.uint8)), dict(mask=np.ones(64, dtype=np.uint8)),
               dict(votes_out=torch.zeros((ns, 4), dtype=torch.int32, device=dev)), dict(votes_out=torch.zeros((ns * 4,), dtype=torch.int64, device=dev)),
               dict(votes_out=torch.zeros((ns, 4), dtype=torch.int64)), dict(voters_out=torch.zeros(ns + 1, dtype=torch.int64, device=dev)),
               dict(voters_out=torch.zeros(ns, dtype=torch.float64, device=dev)),
               dict(votes_out=torch.zeros((ns, 8), dtype=torch.int64, device=dev)[:, ::2])]
        for kw in bad:
            with pytest.raises(ValueError):
                agent.consensus(**kw)
        for table in (torch.zeros((ns, 4), dtype=torch.float32, device=dev), torch.zeros((ns, 4), dtype=torch.float64),
                      torch.zeros((ns + 1, 4), dtype=torch.float64, device=dev), torch.zeros((4, ns), dtype=torch.float64, device=dev).t(),
                      np.zeros((ns, 4))):
            with pytest.raises(ValueError):
                agent.load_shared_table(table)
        with pytest.raises(ValueError, match="n_envs"):
            agent.consensus_agent(n_envs=0)
        # a valid handle with NULL outputs / a NULL table
        assert env.lib.sgk_tabq_consensus(agent._h, None, None, None) == _lib.ERR_INVALID and b"votes_out_dev is NULL" in env.lib.sgk_last_error()
        assert env.lib.sgk_tabq_load_shared(agent._h, None) == _lib.ERR_INVALID and b"table_dev is NULL" in env.lib.sgk_last_error()
        assert (agent.table_host() == 0).all()
    finally:
        _close((env, agent))


# ---- 8. the trainer ---------------------------------------------------------------------------------------------------------------------
def _train(tmp_path, tag, extra):
    import glob
    import os

    log_dir = str(tmp_path / tag)
    args = S.prepare_parser().parse_args(["-L", log_dir, "-S", "3", "-N", "200", "-E", "3", "-EE", "2", "-V", "40", "boat", "tabular-q", "-l", ".5"] + extra)
    writers = []

    def wf(d):
        writers.append(S.EventFileWriter(d))
        return writers[-1]

    agent, env = S.train_batched(args, writer_factory=wf)
    table, state = agent.table_host(), _state_snapshot(env)
    agent.close(); env.close()
    writers[0].close()
    (path,) = glob.glob(os.path.join(log_dir, "events.out.tfevents.*"))
    events = [e for e in S.read_events(path) if e["tag"] is not None]  # (the file_version record carries none)
    return [e for e in events if not e["tag"].startswith(("data/log_dir/", "data/consensus_eval/"))], table, state


def test_the_trainer_writes_the_consensus_tags_and_training_does_not_notice(tmp_path, capsys):
    """Three training periods with an evaluation after the first and the third and one at the end, each followed by one of the consensus agent. The
    run without the flag writes none of the three tags, the same bytes under every other tag, and ends with the same tables and the
    same env: the vote only reads, and the consensus agent acts on an env handle of its own."""
    _torch()
    with_flag, table, state = _train(tmp_path, "with", ["--consensus-eval"])
    out = capsys.readouterr().out
    without, table0, state0 = _train(tmp_path, "without", [])
    tags = ("Eval/consensus_return", "Eval/consensus_safety", "Eval/consensus_agreement")
    for tag in tags:
        mine = [e for e in with_flag if e["tag"] == tag]
        assert [e["step"] for e in mine] == [0, 1, 2], tag
        assert all(np.isfinite(e["value"]) for e in mine)
    assert all(0.25 <= e["value"] <= 1.0 for e in with_flag if e["tag"] == tags[2])  # the winner of four actions has a quarter at least
    assert not [e for e in without if e["tag"].startswith("Eval/consensus")]
    rest = [e for e in with_flag if e["tag"] not in tags]
    assert len(rest) == len(without) and len(rest) > 10
    for a, b in zip(rest, without):
        assert repr(a) == repr(b)
    assert table.tobytes() == table0.tobytes()
    _same(state, state0, "the training env")
    assert out.count("#### CONSENSUS: 200 agents vote on every state") == 1


def test_the_command_line_runs_a_consensus_evaluation(tmp_path):
    """`-S 3 -N 64 -E 2 boat tabular-q -l .5 --consensus-eval` in a child process: status 0 and the one consensus line."""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "safe-grid-agents_amd")]))
    cmd = [sys.executable, "-m", "safe_grid_agents_amd", "-S", "3", "-N", "64", "-E", "2", "-L", str(tmp_path), "boat", "tabular-q", "-l", ".5",
           "--consensus-eval"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-800:] + p.stderr[-1500:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("#### CONSENSUS: 64 agents vote on every state")]
    assert len(lines) == 1 and "agreement" in lines[0], p.stdout[-800:]
