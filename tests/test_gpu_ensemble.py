"""Ensemble acting for the populations -- sgk_policy_act_members_all / sgk_members_vote, EnsembleMixin -- on the GPU. Every comparison is
exact: integers as they are, floats through their bytes.

1. the cross product is M single calls: member m's actions and scores == env.policy_act(member m's slices, epsilon 0), on 128 + 37 envs,
   at a size where a member's workgroups walk a second env tile, and for H = 128 through the raw call;
2. the vote is tests/ensemble_reference.py's: actions, counts and the dissent counters; members [A, A, B, B] settle every disagreement
   on the lower action; a voter subset; envs whose episode is over do not count towards dissent;
3. identical members are one agent: evaluate_ensemble of five copies == batched_default_eval of the single agent, handle and metrics
   bit for bit, dissent 0 -- ppo-mlp and deep-q;
4. evaluate_ensemble == the loop done by hand (policy_act per member, the numpy vote on the host, env.step / reset_done); a recorded
   graph gives the same bytes; the population is untouched;
5. the trainer's --ensemble-eval writes its three tags and perturbs nothing else.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import hashlib
import types

import numpy as np
import pytest

import ensemble_reference as ER
import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib
from safe_grid_agents_amd import ppo_population as PP
from safe_grid_agents_amd.loops import batched_default_eval

pytestmark = pytest.mark.gpu

LEVELS = ["BoatRace-v0", "SideEffectsSokoban-v0"]
TILE = 128  # envs per workgroup and pass of the fused policy kernel (csrc/sgk_policy.hip: PMFMA_ENVS)
N_SMALL = TILE + 37  # one full tile, then one full wave and five envs of the next


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ppo_args(hidden, rollouts, seed=5):
    return types.SimpleNamespace(discount=0.99, batch_size=7, rollouts=rollouts, epochs=2, n_layers=2, n_hidden=hidden, n_channels=5,
                                 device=0, log_gradients=False, cheat=False, seed=seed, lr=1e-3, clipping=0.2, critic_coeff=1.0,
                                 entropy_bonus=0.01)


def _dqn_args(hidden, seed=5):
    return types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=8, sync_every=50, epsilon=0.1, epsilon_anneal=1000, n_layers=2,
                                 n_hidden=hidden, seed=seed, device=0, log_gradients=False, cheat=False, q_body="mlp", n_channels=5,
                                 replay_capacity=64)


def _random_weights(torch, rng, members, cells, hidden, dev):
    """Policy weights stacked [M, ...] in the fused kernels' layout, seeded (scale: scores that are neither flat nor saturated)."""
    shapes = {"w1t": (cells, hidden), "b1": (hidden,), "w2": (hidden, hidden), "b2": (hidden,), "w3t": (hidden, 4), "b3": (4,)}
    return {k: torch.as_tensor(rng.normal(0.0, 0.3, (members,) + s).astype(np.float32)).to(dev) for k, s in shapes.items()}


def _episodes(env):
    return env._device_views()["n_episodes"].cpu().numpy()


def _handle_state(env, episodes_before=0):
    """Everything an evaluation leaves in the handle: boards, last step records, the decoded state words, the episode arrays, the metrics.
    n_episodes counts over the handle's life (no reset clears it): what it gained since episodes_before (_episodes(env) then)."""
    v = env._device_views()
    out = {"boards": env.boards_host(), "records": env.step_records_host(), "metrics": env.metrics()}
    out.update({"word " + k: a for k, a in env.episode_state_host().items()})
    out.update({k: v[k].cpu().numpy() for k in ("last_return", "last_performance")})
    out["n_episodes"] = _episodes(env) - episodes_before
    return out


def _same_bytes(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def _population_hash(pop):
    """One digest over everything the ensemble must leave alone: weights, transposes, optimiser state, step and draw counters, the
    old / target policy and the members' metrics."""
    h = hashlib.sha256()
    tensors = dict(pop.tensors())
    tensors.update({"aux_" + k: t for k, t in (pop.old if hasattr(pop, "old") else pop.target).items()})
    tensors["member_metrics"] = pop.member_metrics
    for k in sorted(tensors):
        h.update(k.encode())
        h.update(tensors[k].cpu().numpy().tobytes())
    h.update(repr((getattr(pop, "draws", None), getattr(pop, "t", None))).encode())
    return h.hexdigest()


# ---- 1. the cross product is M single calls -------------------------------------------------------------------------------------------
def _check_cross_product(torch, env, weights, members):
    """member_actions[m] / member_scores[m] of ONE sgk_policy_act_members_all call against sgk_policy_act with member m's slices; the
    outputs carry sentinels, so every entry was written by the call."""
    n, dev = env.n_envs, "cuda:%d" % env.device
    actions = torch.full((members, n), 77, dtype=torch.uint8, device=dev)
    scores = torch.full((members, n, 4), float("nan"), dtype=torch.float32, device=dev)
    boards = env.boards_host()
    assert env.policy_act_members_all(weights, members, out=actions, scores_out=scores) is actions
    assert env.policy_act_members_all(weights, members).cpu().numpy().tobytes() == actions.cpu().numpy().tobytes()  # scores are optional
    got_a, got_s = actions.cpu().numpy(), scores.cpu().numpy()
    assert got_a.max() <= 3 and not np.isnan(got_s).any()
    for m in range(members):
        single = {k: v[m] for k, v in weights.items()}
        want_s = torch.full((n, 4), float("nan"), dtype=torch.float32, device=dev)
        want_a = env.policy_act(single, epsilon=0.0, draw_index=0, scores_out=want_s)
        assert got_a[m].tobytes() == want_a.cpu().numpy().tobytes(), (m, np.flatnonzero(got_a[m] != want_a.cpu().numpy())[:8])
        assert got_s[m].tobytes() == want_s.cpu().numpy().tobytes(), m
        assert (got_a[m] == got_s[m].argmax(axis=1)).all()  # greedy: the first maximum
    assert len({got_a[m].tobytes() for m in range(members)}) > 1 or members == 1  # the members are different policies
    assert env.boards_host().tobytes() == boards.tobytes()  # the env is read, never written
    return got_a


@pytest.mark.parametrize("hidden", [64, 100])
@pytest.mark.parametrize("name", LEVELS)
def test_the_cross_product_is_one_policy_act_per_member(name, hidden):
    """A ppo-mlp population of M = 3 (random init, not trained) on 128 + 37 envs, 5 random steps into their episodes so that the boards
    differ: two tiles per member, the second with one full wave and five envs."""
    torch = _torch()
    env = S.BatchedGridworldEnv(name, N_SMALL, seed=31, env_index_base=1000)
    try:
        pop = S.BatchedPPOPopulation(env, _ppo_args(hidden, N_SMALL // 3), 3)
        env.step_random(5, auto_reset=True)
        assert len({b.tobytes() for b in env.boards_host()}) > 1
        _check_cross_product(torch, env, pop._ensemble_weights(), 3)
    finally:
        env.close()


@pytest.mark.parametrize("name,hidden", [("BoatRace-v0", 100), ("SideEffectsSokoban-v0", 64)])
def test_a_members_second_grid_stride_pass_is_exact_and_stops_at_n(name, hidden):
    """launch_policy_act_members (csrc/sgk_policy.hip) starts grid_for(ceil(n / 128), max(n_cus / M, 1)) = min(tiles, n_cus // M) workgroups
    per member, each taking the tiles blockIdx.x, blockIdx.x + wgs, ...: with M = 3 and n = 128 (cus // 3 + 2) + 37 there are cus // 3 + 3
    tiles, so a member's workgroups 0 .. 2 run a second pass -- the board tile fetched into the other LDS buffer during the first, W2 /
    W3 not committed again -- and the last tile holds 37 envs."""
    torch = _torch()
    cus = torch.cuda.get_device_properties(0).multi_processor_count  # what the library's n_cus is (csrc/sgk_api.hip)
    wgs = max(cus // 3, 1)
    n = TILE * (wgs + 2) + 37
    assert -(-n // TILE) == wgs + 3 and n % TILE == 37 and n <= 35000
    env = S.BatchedGridworldEnv(name, n, seed=32)
    try:
        env.step_random(5, auto_reset=True)
        w = _random_weights(torch, np.random.default_rng(hidden), 3, env.n_cells, hidden, "cuda:%d" % env.device)
        _check_cross_product(torch, env, w, 3)
    finally:
        env.close()


@pytest.mark.parametrize("name", LEVELS)
def test_the_raw_call_covers_128_hidden_units_and_one_member(name):
    torch = _torch()
    env = S.BatchedGridworldEnv(name, N_SMALL, seed=33, layout="pitched" if name == "BoatRace-v0" else "compact")
    try:
        env.step_random(5, auto_reset=True)
        dev = "cuda:%d" % env.device
        _check_cross_product(torch, env, _random_weights(torch, np.random.default_rng(128), 3, env.n_cells, 128, dev), 3)
        _check_cross_product(torch, env, _random_weights(torch, np.random.default_rng(1), 1, env.n_cells, 100, dev), 1)
    finally:
        env.close()


def test_what_cannot_run_is_refused_with_the_reason():
    torch = _torch()
    env = S.BatchedGridworldEnv("BoatRace-v0", 64, seed=1)
    try:
        dev = "cuda:%d" % env.device
        w = _random_weights(torch, np.random.default_rng(0), 2, env.n_cells, 64, dev)
        ma = torch.zeros((2, 64), dtype=torch.uint8, device=dev)
        for call, message in (
            (lambda: env.policy_act_members_all(w, 3), "shape"), (lambda: env.policy_act_members_all(w, 0), "n_members"),
            (lambda: env.policy_act_members_all(w, 2, out=torch.zeros((2, 63), dtype=torch.uint8, device=dev)), "out has shape"),
            (lambda: env.policy_act_members_all(w, 2, out=ma.cpu()), "lives on"),
            (lambda: env.policy_act_members_all(w, 2, scores_out=torch.zeros((2, 64, 4), dtype=torch.float64, device=dev)), "dtype"),
            (lambda: env.members_vote(ma[0]), "member_actions"), (lambda: env.members_vote(ma.to(torch.int32)), "dtype"),
            (lambda: env.members_vote(ma, members=torch.zeros(3, dtype=torch.int32, device=dev)), "member indices"),
            (lambda: env.members_vote(ma, members=torch.zeros(1, dtype=torch.int64, device=dev)), "dtype"),
            (lambda: env.members_vote(ma, votes_out=torch.zeros((64, 4), dtype=torch.int32, device=dev)), "dtype"),
            (lambda: env.members_vote(ma, dissent=torch.zeros(3, dtype=torch.int64, device=dev)), "dissent has shape"),
        ):
            with pytest.raises(ValueError, match=message):
                call()
        odd = _random_weights(torch, np.random.default_rng(0), 2, env.n_cells, 96, dev)  # a hidden width without an instantiation
        with pytest.raises(_lib.SgkError, match="n_hidden"):
            env.policy_act_members_all(odd, 2)
        pop = S.BatchedPPOPopulation(env, _ppo_args(64, 16), 4)
        for members, message in (([], "selects nobody"), ([1, 1], "twice"), ([0, 4], "members 0 .. 3"),
                                 (torch.tensor([2, -1], device=dev), "members 0 .. 3"), (torch.tensor([0.5]), "dtype")):
            with pytest.raises(ValueError, match=message):
                pop.ensemble_act(members=members)
            with pytest.raises(ValueError, match=message):
                pop.evaluate_ensemble(3, members=members)
    finally:
        env.close()


# ---- 2. the vote is the numpy reference's ---------------------------------------------------------------------------------------------
def _two_by_two(env, hidden, seed):
    """A population of M = 4 whose members are [A, A, B, B]: two distinct random-init weight sets."""
    pop = S.BatchedPPOPopulation(env, _ppo_args(hidden, env.n_envs // 4, seed=seed), 4)
    pop.load_member(1, PP.unstack_state_dict(pop.cur, 0))
    pop.load_member(3, PP.unstack_state_dict(pop.cur, 2))
    return pop


@pytest.mark.parametrize("name,hidden", [("BoatRace-v0", 64), ("SideEffectsSokoban-v0", 100)])
def test_the_vote_is_the_numpy_reference(name, hidden):
    """Members [A, A, B, B] on 168 envs: every env is a 4-0 or a 2-2 vote, and a 2-2 tie goes to the lower action. Seed 5 (the run's
    seed behind default_member_seed) makes A and B different enough to disagree on some board of both levels after 5 random steps (on
    79 of BoatRace's 168 envs and on 158 of Sokoban's; the count is printed). Then a subset [2, 0] (one voter of each kind: every disagreement is a 1-1 tie), and the dissent counters on envs
    some of which are over: half the envs are reset 50 steps in, the others run into the level's step limit without auto-reset."""
    torch = _torch()
    n = TILE + 40
    env = S.BatchedGridworldEnv(name, n, seed=41)
    try:
        dev = "cuda:%d" % env.device
        pop = _two_by_two(env, hidden, seed=5)
        env.step_random(5, auto_reset=True)
        votes = torch.full((n, 4), 777, dtype=torch.uint16, device=dev)
        actions = pop.ensemble_act(votes_out=votes).cpu().numpy()
        ma = pop._ens["member_actions"].cpu().numpy()
        assert ma.shape == (4, n) and (ma[0] == ma[1]).all() and (ma[2] == ma[3]).all()
        want = ER.vote(ma)
        assert actions.tobytes() == want[0].tobytes() and votes.cpu().numpy().tobytes() == want[1].tobytes()
        disagree = ma[0] != ma[2]
        print("%s: A and B disagree on %d of %d envs" % (name, int(disagree.sum()), n))
        assert disagree.any() and (actions[disagree] == np.minimum(ma[0], ma[2])[disagree]).all()
        assert (actions[~disagree] == ma[0][~disagree]).all()
        # a subset, through the population and through the raw call with counters
        out = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        assert pop.ensemble_act(members=[2, 0], out=out) is out
        assert out.cpu().numpy().tobytes() == ER.vote(ma, members=[2, 0])[0].tobytes()
        assert pop.ensemble_act(members=torch.tensor([3], device=dev)).cpu().numpy().tobytes() == ma[3].tobytes()  # one voter: its own actions
        # some envs over: they are excluded from dissent
        horizon = int(env.info.max_iterations)
        mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        mask[::2] = 1
        env.step_random(45, auto_reset=True)
        env.reset(mask)
        env.step_random(horizon - 50, auto_reset=False)
        over = env.episode_state_host()["over"].astype(bool)
        assert over.any() and not over.all()
        ma_dev = env.policy_act_members_all(pop._ensemble_weights(), 4)
        dissent = torch.tensor([1000, 5], dtype=torch.int64, device=dev)
        for members in (None, [1, 2, 3]):
            ids = None if members is None else torch.tensor(members, dtype=torch.int32, device=dev)
            before = dissent.cpu().numpy().copy()
            got = env.members_vote(ma_dev, members=ids, votes_out=votes, dissent=dissent)
            want = ER.vote(ma_dev.cpu().numpy(), members=members, live=~over)
            assert got.cpu().numpy().tobytes() == want[0].tobytes() and votes.cpu().numpy().tobytes() == want[1].tobytes()
            assert (dissent.cpu().numpy() - before).tolist() == want[2].tolist()  # accumulated, not overwritten
            assert want[2][1] == (4 if members is None else 3) * int((~over).sum())
    finally:
        env.close()


# ---- 3. identical members are one agent -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ppo-mlp", "deep-q"])
@pytest.mark.parametrize("name,hidden", [("BoatRace-v0", 100), ("SideEffectsSokoban-v0", 64)])
def test_identical_members_are_one_agent(name, hidden, kind):
    """M = 5 load_member copies of one agent on 165 envs: evaluate_ensemble(T = 7) -- T - 1 steps of {act-all, vote, step, reset_done},
    then max_iterations steps without the reset -- leaves what batched_default_eval of the single agent (its greedy weights through
    sgk_policy_rollout) leaves on a twin env with the same seed and env_index_base, and nobody ever dissents."""
    torch = _torch()
    T, M = 7, 5
    e1, e2 = (S.BatchedGridworldEnv(name, N_SMALL, seed=51, env_index_base=700) for _ in range(2))
    try:
        torch.manual_seed(9)
        if kind == "ppo-mlp":
            agent = S.BatchedPPOAgent(e1, _ppo_args(hidden, N_SMALL))
            pop = S.BatchedPPOPopulation(e2, _ppo_args(hidden, N_SMALL // M), M)
            for m in range(M):
                pop.load_member(m, agent.net.state_dict())
        else:
            agent = S.BatchedDeepQAgent(e1, _dqn_args(hidden), replay_slices=2)
            pop = S.BatchedDeepQPopulation(e2, _dqn_args(hidden), M, replay_slices=2)
            for m in range(M):
                pop.load_member(m, agent.Q.state_dict())
        assert agent.greedy_weights() is not None  # (the single agent's evaluation is the fused rollout)
        want = batched_default_eval(agent, e1, T)
        got, dissent = pop.evaluate_ensemble(T)
        assert got.vec == want.vec
        assert want.vec[_lib.M_EPISODES] >= N_SMALL
        _same_bytes(_handle_state(e1), _handle_state(e2), (name, kind))
        horizon = int(e1.info.max_iterations)
        assert dissent["dissent"] == 0 and dissent["disagreement"] == 0.0 and 0 < dissent["votes"] <= M * N_SMALL * (T - 1 + horizon)
    finally:
        e1.close(); e2.close()


# ---- 4. the evaluation is the loop done by hand ---------------------------------------------------------------------------------------
def _by_hand(torch, env, weights, M, T, members=None):
    """evaluate_ensemble's schedule from the existing calls: env.policy_act per member, the vote on the host, env.step / reset_done."""
    dissent = np.zeros(2, dtype=np.int64)
    singles = [{k: v[m] for k, v in weights.items()} for m in range(M)]
    env.metrics_reset()
    env.reset()

    def step(reset_done):
        live = ~env.episode_state_host()["over"].astype(bool)
        ma = np.stack([env.policy_act(w, epsilon=0.0, draw_index=0).cpu().numpy() for w in singles])
        actions, _, d = ER.vote(ma, members=members, live=live)
        dissent[:] += d
        env.step(torch.as_tensor(actions).to("cuda:%d" % env.device), auto_reset=False)
        if reset_done:
            env.reset_done()

    for _ in range(T - 1):
        step(True)
    for _ in range(int(env.info.max_iterations)):
        step(False)
    return env.metrics(), dissent


@pytest.mark.parametrize("name,hidden", [("BoatRace-v0", 64), ("SideEffectsSokoban-v0", 100)])
def test_the_evaluation_is_the_loop_done_by_hand(name, hidden):
    """M = 3 distinct members on 165 envs, T = 7: metrics, the handle and the dissent counters against the hand-written loop on a twin
    env; graph=True (one recorded lockstep step per phase, replayed) gives the same bytes, twice; a subset [2, 0] likewise; and the
    population's weights, optimiser state, counters and member metrics are what they were."""
    torch = _torch()
    T, M = 7, 3
    e1, e2 = (S.BatchedGridworldEnv(name, N_SMALL, seed=61, env_index_base=64) for _ in range(2))
    try:
        pop = S.BatchedPPOPopulation(e2, _ppo_args(hidden, N_SMALL // M), M)
        before = _population_hash(pop)
        for members in (None, [2, 0]):
            episodes = _episodes(e1)
            want_metrics, want_dissent = _by_hand(torch, e1, pop._ensemble_weights(), M, T, members)
            want_state = _handle_state(e1, episodes)
            assert (want_state["n_episodes"] >= 1).all()
            assert want_dissent[1] > 0
            for graph in (False, True, True):
                episodes = _episodes(e2)
                bm, dissent = pop.evaluate_ensemble(T, members=members, graph=graph)
                assert bm.vec == want_metrics.tolist(), (members, graph)
                assert [dissent["dissent"], dissent["votes"]] == want_dissent.tolist(), (members, graph)
                assert dissent["disagreement"] == want_dissent[0] / want_dissent[1]
                _same_bytes(want_state, _handle_state(e2, episodes), (name, members, graph))
            if members is None:
                print("%s: disagreement %d / %d" % (name, want_dissent[0], want_dissent[1]))
        assert _population_hash(pop) == before
    finally:
        e1.close(); e2.close()


def test_a_deepq_population_is_untouched_by_its_ensemble():
    torch = _torch()
    env = S.BatchedGridworldEnv("BoatRace-v0", 64, seed=71)
    try:
        pop = S.BatchedDeepQPopulation(env, _dqn_args(64), 4, replay_slices=2)
        pop.warmup(2)
        env.reset()
        for _ in range(3):
            pop.step(learn=True)
        torch.cuda.synchronize()
        before = _population_hash(pop)
        bm, dissent = pop.evaluate_ensemble(3)
        actions = pop.ensemble_act()
        assert actions.shape == (64,) and dissent["votes"] > 0 and bm.vec[_lib.M_EPISODES] >= 64
        assert _population_hash(pop) == before
    finally:
        env.close()


# ---- 5. the trainer -------------------------------------------------------------------------------------------------------------------
TRAINER_ARGS = ["-S", "3", "-E", "2", "-EE", "1", "-V", "20", "boat", "ppo-mlp", "-l", "1e-3", "-r", "2", "-e", "2", "-b", "7", "--members", "3"]


def _train(tmp_path, tag, extra):
    import glob
    import os

    log_dir = str(tmp_path / tag)
    args = S.prepare_parser().parse_args(["-L", log_dir] + TRAINER_ARGS + extra)
    writers = []

    def wf(d):
        writers.append(S.EventFileWriter(d))
        return writers[-1]

    agent, env = S.train_batched(args, writer_factory=wf)
    env.close()
    writers[0].close()
    (path,) = glob.glob(os.path.join(log_dir, "events.out.tfevents.*"))
    events = [e for e in S.read_events(path) if e["tag"] is not None]  # (the file_version record carries none)
    return [e for e in events if not e["tag"].startswith(("data/log_dir/", "data/ensemble_eval/"))]  # the two flags that differ


def test_the_trainer_writes_the_ensemble_tags_and_nothing_else_moves(tmp_path, capsys):
    """`-S 3 -E 2 -EE 1 boat ppo-mlp -l 1e-3 -r 2 -e 2 -b 7 --members 3 --ensemble-eval` (with -V 20 to keep it short): three evaluations
    (after both periods and at the end), each followed by one of the ensemble. The run without the flag writes none of the three tags and
    the same bytes under every other tag: the ensemble evaluation draws nothing and touches no member (section 4), the env's metrics are
    reset by the next period before they are read, and the env.reset() that follows every evaluation puts the envs back (BoatRace has
    no draws of its own, so the extra resets leave no trace)."""
    _torch()
    with_flag = _train(tmp_path, "with", ["--ensemble-eval"])
    out = capsys.readouterr().out
    without = _train(tmp_path, "without", [])
    tags = ("Eval/ensemble_return", "Eval/ensemble_safety", "Eval/ensemble_disagreement")
    for tag in tags:
        mine = [e for e in with_flag if e["tag"] == tag]
        assert [e["step"] for e in mine] == [0, 1, 2], tag
        assert all(np.isfinite(e["value"]) for e in mine)
    assert all(0.0 <= e["value"] <= 1.0 for e in with_flag if e["tag"] == tags[2])
    assert not [e for e in without if e["tag"].startswith("Eval/ensemble")]
    rest = [e for e in with_flag if e["tag"] not in tags]
    assert len(rest) == len(without) and len(rest) > 10
    for a, b in zip(rest, without):
        assert repr(a) == repr(b)
    assert "#### ENSEMBLE: 3 members vote on every env" in out
