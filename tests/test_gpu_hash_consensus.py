"""The hashed levels' consensus by board key on the device (include/sgk.h: sgk_tabq_hash_consensus, sgk_tabq_hash_load_shared;
BatchedTabularQAgent.hash_consensus / load_shared_hash_table / hash_consensus_agent / evaluate_hash_consensus; --hash-consensus-eval):

1. the vote of 322 trained agents (capacity 64, 99 steps: tests/hashed_tabq_reference.py's cached run) against the dictionary vote
   (tests/hash_consensus_reference.py) by key, and against the host call on copy_keys / copy_table byte for byte -- everyone, every third
   agent, agent 7 alone, and max_keys below U; the source is only read;
2. later grid passes: 16 706 agents on a handle capped at 64 workgroups, device == host call;
3. the load: three masked loads build three groups, byte-equal to the host load and to each other, the rest untouched; the tag rule; a
   synthetic vote over the groups (ties, zero rows, displaced slots) against the dictionary;
4. end to end: evaluate_hash_consensus against the dictionaries' evaluation, agent 7 alone against a twin loaded with its own rows, a
   second call; hash_consensus_agent;
5. vote + conversion + load recorded once in a graph and replayed after more training;
6. guard bands under both patterns (tests/guard_arena.py; tests/test_hash_consensus_cpu.py points here);
7. refusals; 8. the trainer's flag.
Counts are integers and rows are copied: every comparison is exact."""
import ctypes
import glob
import os
import types

import numpy as np
import pytest

import guard_arena as GA
import hash_consensus_reference as HC
import hash_grow_plans as G
import hashed_tabq_reference as HR
import safe_grid_agents_amd as S
import test_gpu_parity as P
import test_gpu_tabq_consensus as TC
from safe_grid_agents_amd import _lib

pytestmark = pytest.mark.gpu

EMPTY = HC.EMPTY
MASKS = {"all": None, "thirds": np.arange(HR.N) % 3 == 0, "seven": np.arange(HR.N) == 7}
U_OF = {"all": 10044, "thirds": 4445, "seven": 61}  # tests/test_hash_consensus_cpu.py derives them from the dictionary


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _make(capacity, n=HR.N, env_index_base=0, name=HR.NAME):
    _torch()
    env = S.BatchedGridworldEnv(name, n, seed=HR.SEED, env_index_base=env_index_base)
    agent = S.BatchedTabularQAgent(env, types.SimpleNamespace(hash_capacity=capacity, **HR.ARGS))
    return env, agent


def _close(*pairs):
    for env, agent in pairs:
        agent.close()
        env.close()


def _dev_mask(torch, mask):
    return None if mask is None else torch.as_tensor(np.asarray(mask).astype(np.uint8), device="cuda")


def _got(cons):
    """(keys uint32, votes, voters, U) of a HashedConsensus on the host."""
    return (cons.keys.cpu().numpy().view(np.uint32), cons.votes.cpu().numpy(), cons.voters.cpu().numpy(), int(cons.count.item()))


def _same_vote(got, want, where):
    assert got[3] == want[3], (where, got[3], want[3])
    for a, b, what in zip(got[:3], want[:3], ("keys", "votes", "voters")):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (where, what)


def _dictionary_votes():
    """The 322 dictionaries of the cached run by key, as tests/test_hash_consensus_cpu.py reads them."""
    _, agents, _ = HR.run(64, 99, claim_start_on_reset=True)
    R = G.rules()
    return [{G.board_key(R, b): list(r) for b, r in a.rows.items()} for a in agents]


@pytest.fixture(scope="module")
def trained():
    """322 agents at capacity 64 behind rollout(99): made once, only read by the tests that share it."""
    env, agent = _make(64)
    agent.rollout(99, kernel="hbm")
    yield env, agent
    _close((env, agent))


# ---- 1. the vote against the dictionary -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("who", list(MASKS))
def test_the_device_vote_equals_the_dictionary_and_the_host_call(trained, who):
    torch = _torch()
    env, agent = trained
    mask = MASKS[who]
    keys0, tab0, info0, t0, eps0 = agent.keys_host(), agent.table_host(), agent.hash_info(), agent.t, agent.epsilon
    want = HC.vote(_dictionary_votes(), mask)
    assert len(want) == U_OF[who]
    K = HR.N * 64
    cons = agent.hash_consensus(mask=_dev_mask(torch, mask))
    assert cons.max_keys == K and cons.keys.dtype == torch.int32 and cons.count.shape == (1,) and cons.count.is_cuda
    got = _got(cons)
    _same_vote(got, HC.arrays(want, K), who + ": the dictionary")
    _same_vote(got, HC.host_vote(keys0, tab0, mask, max_keys=K), who + ": the host call")
    assert cons.n_keys() == len(want) and cons.as_dict() == want
    assert cons.policy[:len(want)].cpu().numpy().tolist() == HC.policy(got[1][:len(want)]).tolist() and not cons.policy[len(want):].any()
    cast = sum(sum(c) for c in want.values())
    assert cons.agreement() == sum(max(c) for c in want.values()) / cast
    if who == "all":
        assert int(got[2].max()) == HR.N and cast == 18942  # every agent votes on the start board: several waves on one address
        small = agent.hash_consensus(max_keys=4096)  # below U: the first 4 096 keys with their full counts, count = U
        _same_vote(_got(small), HC.arrays(want, 4096), "max_keys below U")
        with pytest.raises(RuntimeError, match="max_keys"):
            small.n_keys()
    # the source was only read
    assert agent.keys_host().tobytes() == keys0.tobytes() and agent.table_host().tobytes() == tab0.tobytes()
    assert agent.hash_info() == info0 and agent.t == t0 and float(agent.epsilon).hex() == float(eps0).hex()


# ---- 2. later grid passes -------------------------------------------------------------------------------------------------------------------
def test_the_vote_and_the_load_reach_every_agent_of_a_grid_stride_launch(monkeypatch):
    """16 384 + 322 agents on a handle whose grids are capped at 64 workgroups (256 waves for 262 agent tiles x 4 slot chunks: five
    passes, the last one partial; the key broadcast takes 66 passes): the device vote equals the host call, and a masked load reaches
    the agents of the later passes."""
    torch = _torch()
    n = 16384 + HR.N
    monkeypatch.setenv("SGK_MAX_GRID", "64")
    env, agent = _make(64, n=n)
    monkeypatch.delenv("SGK_MAX_GRID")
    try:
        grids = (ctypes.c_int32 * 4)()
        _lib.check(env.lib.sgk_debug_launch_grids(env.handle, grids))
        assert grids[1] == 64, "the handle ignored the grid knob: the case would be empty"
        agent.rollout(20, kernel="hbm")
        keys0, tab0 = agent.keys_host(), agent.table_host()
        mask = np.arange(n) % 5 != 1
        for m in (None, mask):
            cons = agent.hash_consensus(mask=_dev_mask(torch, m), max_keys=1 << 15)
            _same_vote(_got(cons), HC.host_vote(keys0, tab0, m, max_keys=1 << 15), "capped grid")
        U = cons.n_keys()
        assert 500 < U < 1 << 15
        pick = np.zeros(n, dtype=np.uint8)
        pick[[3, 16383, 16384, 16500, n - 1]] = 1
        rows = cons.votes.to(torch.float64)
        agent.load_shared_hash_table(cons.keys, rows, cons.count, mask=_dev_mask(torch, pick))
        keys1, tab1 = agent.keys_host(), agent.table_host()
        want_keys, want_rows, over = HC.host_load(_got(cons)[0], rows.cpu().numpy(), 64, count=U)
        assert over == 1 and agent.hash_info()[2]  # more voted boards than slots: the template overflows, as the header says
        for e in np.flatnonzero(pick):
            assert keys1[e].tobytes() == want_keys.tobytes() and tab1[e].tobytes() == want_rows.tobytes(), e
        rest = pick == 0
        assert keys1[rest].tobytes() == keys0[rest].tobytes() and tab1[rest].tobytes() == tab0[rest].tobytes()
    finally:
        _close((env, agent))


# ---- 3. the load ----------------------------------------------------------------------------------------------------------------------------
def _key_lists(rng):
    """Three (keys, rows) lists: A with a duplicate and rows of every special kind, B that shares keys with A at other positions (so
    the same key is displaced differently), C longer than the capacity."""
    pool = rng.permutation(1 << 22)[:120].astype(np.uint32)
    pool[:4] = (0, 0x3F, 0x40, 0x200010)
    a_keys = pool[:50].copy()
    a_keys[30] = a_keys[2]
    a_rows = rng.standard_normal((50, 4))
    a_rows[1], a_rows[5], a_rows[6], a_rows[7] = 0.0, (2.0, 1.0, 2.0, -1.0), (-0.0, -0.0, -0.0, -0.0), (-1.5, -0.25, -3.0, -0.25)
    b_keys = pool[10:70][::-1].copy()
    b_rows = rng.standard_normal((60, 4))
    b_rows[3], b_rows[9] = (0.5, 3.0, -2.0, 3.0), 0.0
    c_keys = pool[20:120].copy()
    c_rows = rng.standard_normal((100, 4))
    return (a_keys, a_rows), (b_keys, b_rows), (c_keys, c_rows)


def test_three_masked_loads_build_three_groups():
    torch = _torch()
    n = 200
    env, agent = _make(64, n=n)
    twin_env, twin = _make(64, n=n)
    try:
        for a in (agent, twin):
            a.rollout(30, kernel="hbm")
        lists = _key_lists(np.random.default_rng(3))
        group = np.arange(n) % 4  # group 3 is never selected
        keys0, tab0 = agent.keys_host(), agent.table_host()
        assert twin.keys_host().tobytes() == keys0.tobytes()
        acted = agent.act_explore().clone()  # a pending act(): the selected agents forget it
        twin_acted = twin.act_explore()
        assert torch.equal(acted, twin_acted)
        hosts = []
        for g, (keys, rows) in enumerate(lists):
            k = torch.as_tensor(keys.view(np.int32), device="cuda")
            r = torch.as_tensor(rows, device="cuda")
            count = torch.tensor([len(keys) - (2 if g == 1 else 0)], dtype=torch.int64, device="cuda")  # B: a count below the list
            agent.load_shared_hash_table(k, r, count if g else None, mask=_dev_mask(torch, group == g))
            hosts.append(HC.host_load(keys, rows, 64, count=int(count.item())))
        assert [h[2] for h in hosts] == [0, 0, 1] and agent.hash_info()[2]  # C: 100 distinct keys, 64 slots
        keys1, tab1 = agent.keys_host(), agent.table_host()
        for g, (want_keys, want_rows, _) in enumerate(hosts):
            for e in np.flatnonzero(group == g):
                assert keys1[e].tobytes() == want_keys.tobytes() and tab1[e].tobytes() == want_rows.tobytes(), (g, e)
            table, dropped = HC.load(lists[g][0][:len(lists[g][0]) - (2 if g == 1 else 0)], lists[g][1], 64)
            assert HC.table_as_dict(want_keys, want_rows) == table and bool(dropped) == (g == 2)
        rest = group == 3
        assert keys1[rest].tobytes() == keys0[rest].tobytes() and tab1[rest].tobytes() == tab0[rest].tobytes()
        # the tag rule: learn() behind a load without a new act() learns nothing in the loaded agents -- and what it does in the others
        # is what it does in the twin that was never loaded
        env.step(acted, auto_reset=False)
        agent.learn(action=acted)
        twin_env.step(twin_acted, auto_reset=False)
        twin.learn(action=twin_acted)
        keys2, tab2 = agent.keys_host(), agent.table_host()
        loaded = ~rest
        assert keys2[loaded].tobytes() == keys1[loaded].tobytes() and tab2[loaded].tobytes() == tab1[loaded].tobytes()
        assert keys2[rest].tobytes() == twin.keys_host()[rest].tobytes() and tab2[rest].tobytes() == twin.table_host()[rest].tobytes()
        assert tab2[rest].tobytes() != tab1[rest].tobytes()  # (they did learn)
        # a synthetic vote over the groups: ties, zero rows, -0.0 rows and displaced slots on the device
        for mask in (None, group != 3, group == 1):
            cons = agent.hash_consensus(mask=_dev_mask(torch, mask))
            want = HC.vote(HC.tables_as_dicts(keys2, tab2), mask)
            _same_vote(_got(cons), HC.arrays(want, n * 64), "synthetic")
        both = set(lists[0][0][:50].tolist()) & set(lists[1][0][:58].tolist())
        where = {k: {int(np.flatnonzero(hosts[g][0] == k)[0]) for g in (0, 1)} for k in both}
        assert any(len(s) == 2 for s in where.values())  # the same key at different slots in different agents
    finally:
        _close((env, agent), (twin_env, twin))


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------------------
def _dictionary_twin(votes, n):
    """n dictionaries that hold the vote counts as rows, by board."""
    R = G.rules()
    out = HR.new_agents(n, 1 << 20)
    for a in out:
        a.rows = {G.board_of_key(R, k): [float(c) for c in counts] for k, counts in sorted(votes.items())}
    return out


def _assert_twin_tables(twin, ref, where):
    R = G.rules()
    keys, tab = twin.keys_host(), twin.table_host()
    for e, a in enumerate(ref):
        got = {G.board_of_key(R, k): row for k, row in HC.table_as_dict(keys[e], tab[e]).items()}
        assert got == a.rows, (where, e, len(got), len(a.rows))


def test_evaluate_hash_consensus_equals_the_dictionaries_evaluation(trained):
    torch = _torch()
    env, agent = trained
    votes = HC.vote(_dictionary_votes())
    steps = 10
    horizon = int(env.info.max_iterations)
    envs = HR.O.EnvBatch(HR.NAME, 64, seed=HR.SEED, env_begin=0)
    ref = _dictionary_twin(votes, 64)
    HR.evaluate(envs, ref, steps - 1, horizon)
    bm, stats = agent.evaluate_hash_consensus(steps, n_envs=64)
    twin = agent._hash_consensus_cache[64]["agent"]
    assert twin.n_states == twin.hash_capacity == agent._hash_capacity_for(len(votes), steps - 1 + horizon) == 16384
    assert stats == {"agreement": sum(max(c) for c in votes.values()) / 18942, "voted_states": 10044, "voters": 18942}
    P.assert_same_state(twin.env, envs, "the consensus twin behind the evaluation")
    _assert_twin_tables(twin, ref, "first call")  # the vote's rows and the zero rows greedy acting claimed, no more
    assert bm.episodes >= 64 and not twin.hash_info()[2]
    # by hand: hash_consensus_agent + evaluate
    hand = agent.hash_consensus_agent(n_envs=64, reserve_steps=steps - 1 + horizon)
    try:
        assert hand.n_states == 16384 and hand is not twin
        want = hand.evaluate(steps)
        assert bm.vec == want.vec
        assert hand.keys_host().tobytes() == twin.keys_host().tobytes() and hand.table_host().tobytes() == twin.table_host().tobytes()
    finally:
        _close((hand.env, hand))
    # A second call on the cached twin: it votes again and loads again, so the slots the first evaluation claimed are gone. This level's
    # own draws are keyed by the env's step count, which an env carries on across evaluations: the second evaluation is the one the
    # dictionaries give when THEIR envs go on too -- fresh dictionaries (the vote alone), the same oracle envs.
    ref2 = _dictionary_twin(votes, 64)
    HR.evaluate(envs, ref2, steps - 1, horizon)
    bm2, stats2 = agent.evaluate_hash_consensus(steps, n_envs=64)
    assert agent._hash_consensus_cache[64]["agent"] is twin and list(agent._hash_consensus_cache) == [64]
    assert stats2 == stats and bm2.episodes == bm.episodes
    P.assert_same_state(twin.env, envs, "second call")
    _assert_twin_tables(twin, ref2, "second call")
    # agent 7 alone, one env: a one-hot count has the row's argmax, so the twin plays agent 7's own greedy policy
    seven = torch.as_tensor((np.arange(HR.N) == 7).astype(np.uint8), device="cuda")
    bm7, stats7 = agent.evaluate_hash_consensus(steps, n_envs=1, mask=seven)
    assert stats7 == {"agreement": 1.0, "voted_states": 61, "voters": 61}
    own_env, own = _make(256, n=1)
    try:
        keys7, tab7 = agent.keys_host(7, 1)[0], agent.table_host(7, 1)[0]
        held = keys7 != EMPTY
        own.load_shared_hash_table(torch.as_tensor(keys7[held].view(np.int32), device="cuda"), torch.as_tensor(tab7[held], device="cuda"))
        assert bm7.vec == own.evaluate(steps).vec
        TC._same(TC._state_snapshot(agent._hash_consensus_cache[1]["agent"].env), TC._state_snapshot(own_env), "agent 7 alone")
    finally:
        _close((own_env, own))


# ---- 5. a recorded graph --------------------------------------------------------------------------------------------------------------------
def test_vote_conversion_and_load_replay_from_a_graph():
    torch = _torch()
    env, agent = _make(64)
    twin_env, twin = _make(256, n=64)
    eager_env, eager = _make(256, n=64)
    try:
        agent.rollout(40, kernel="hbm")
        rows = torch.empty((HR.N * 64, 4), dtype=torch.float64, device="cuda")

        def chain(target):
            cons = agent.hash_consensus()
            rows.copy_(cons.votes)
            target.load_shared_hash_table(cons.keys, rows, cons.count)
            return cons

        chain(twin)  # (eagerly first: buffers and workspaces exist before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cons = chain(twin)
        agent.rollout(10, kernel="hbm")
        graph.replay()
        torch.cuda.synchronize()
        replayed = _got(cons)
        keys_r, tab_r = twin.keys_host(), twin.table_host()
        _same_vote(replayed, HC.host_vote(agent.keys_host(), agent.table_host(), None, max_keys=HR.N * 64), "replay")
        chain(eager)
        assert eager.keys_host().tobytes() == keys_r.tobytes() and eager.table_host().tobytes() == tab_r.tobytes()
        assert replayed[3] > 256 and twin.hash_info()[2]  # (more boards than the twins' slots: the drop is part of what replays)
    finally:
        _close((env, agent), (twin_env, twin), (eager_env, eager))


# ---- 6. guard bands -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_the_vote_and_the_load_stay_inside_their_guard_bands(pattern):
    """"keys", "votes", "voters", "count" and a "workspace" of exactly the advertised size carved from a guard_arena.Arena, the load's
    inputs as frozen inputs: no guard byte and no input byte changes, no output entry keeps the pattern, and the bytes equal what the
    same calls leave on plain tensors."""
    torch = _torch()
    n, K = 130, 130 * 64
    env, agent = _make(64, n=n)
    try:
        agent.rollout(60, kernel="hbm")
        plain = _got(agent.hash_consensus(max_keys=K))
        U = plain[3]
        assert 64 < U < K
        need = int(env.lib.sgk_tabq_hash_consensus_workspace_bytes(agent._h))
        assert need == 768 * 1024 + 8 * 64 + (64 * n + 15) // 16 * 16
        arena = GA.Arena("cuda:%d" % env.device, pattern, 4 << 20)
        keys = arena.carve("keys", (K,), torch.int32)
        votes = arena.carve("votes", (K, 4), torch.int64)
        voters = arena.carve("voters", (K,), torch.int64)
        count = arena.carve("count", (1,), torch.int64)
        workspace = arena.carve("workspace", (need,), torch.uint8)
        mask = arena.adopt("mask", torch.ones(n, dtype=torch.uint8))
        arena.freeze("mask")
        assert arena.layout_ok() and arena.check() == []
        desc = _lib.SgkTabqHashVotes(keys.data_ptr(), votes.data_ptr(), voters.data_ptr(), count.data_ptr(), K, workspace.data_ptr(), need)
        env._sync_torch_to_lib()
        _lib.check(env.lib.sgk_tabq_hash_consensus(agent._h, ctypes.c_void_p(mask.data_ptr()), ctypes.byref(desc)))
        env._sync_lib_to_torch()
        torch.cuda.synchronize()
        assert arena.check() == []
        for name in ("keys", "votes", "voters", "count"):
            assert arena.unwritten(name) == 0, name
        got = (keys.cpu().numpy().view(np.uint32), votes.cpu().numpy(), voters.cpu().numpy(), int(count.item()))
        _same_vote(got, plain, "arena == plain tensors")
        # the load: keys, rows and count are inputs now, the workspace is scratch again
        rows = arena.adopt("rows", votes.to(torch.float64))
        for name in ("keys", "rows", "count"):
            arena.freeze(name)
        pick = arena.adopt("pick", torch.as_tensor((np.arange(n) % 2).astype(np.uint8)))
        arena.freeze("pick")
        keys0, tab0 = agent.keys_host(), agent.table_host()
        env._sync_torch_to_lib()
        _lib.check(env.lib.sgk_tabq_hash_load_shared(agent._h, ctypes.c_void_p(pick.data_ptr()), ctypes.c_void_p(keys.data_ptr()),
                                                     ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(count.data_ptr()), K, ctypes.byref(desc)))
        env._sync_lib_to_torch()
        torch.cuda.synchronize()
        assert arena.check() == []
        want_keys, want_rows, over = HC.host_load(got[0], got[1].astype(np.float64), 64, count=U)
        keys1, tab1 = agent.keys_host(), agent.table_host()
        assert over == 1
        for e in range(n):
            if e % 2:
                assert keys1[e].tobytes() == want_keys.tobytes() and tab1[e].tobytes() == want_rows.tobytes(), e
            else:
                assert keys1[e].tobytes() == keys0[e].tobytes() and tab1[e].tobytes() == tab0[e].tobytes(), e
    finally:
        _close((env, agent))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_a_perfect_hash_level_and_wrong_tensors_are_refused():
    torch = _torch()
    env, agent = _make(0, n=70, name="IslandNavigation-v0")
    henv, hashed = _make(64, n=70)
    try:
        lib = env.lib
        buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        k, v, c = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros((8, 4), dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        r = torch.zeros((8, 4), dtype=torch.float64, device="cuda")
        desc = _lib.SgkTabqHashVotes(k.data_ptr(), v.data_ptr(), None, c.data_ptr(), 8, buf.data_ptr(), buf.numel())
        assert lib.sgk_tabq_hash_consensus_workspace_bytes(agent._h) == _lib.ERR_INVALID and b"perfect hash" in lib.sgk_last_error()
        assert lib.sgk_tabq_hash_consensus(agent._h, None, ctypes.byref(desc)) == _lib.ERR_INVALID and b"perfect hash" in lib.sgk_last_error()
        assert lib.sgk_tabq_hash_load_shared(agent._h, None, k.data_ptr(), r.data_ptr(), c.data_ptr(), 8, ctypes.byref(desc)) == _lib.ERR_INVALID
        assert b"perfect hash" in lib.sgk_last_error()
        for call in (agent.hash_consensus, agent.hash_consensus_agent, lambda: agent.evaluate_hash_consensus(10),
                     lambda: agent.load_shared_hash_table(k, r)):
            with pytest.raises(ValueError, match="perfect hash"):
                call()
        # a workspace that is too small
        need = int(lib.sgk_tabq_hash_consensus_workspace_bytes(hashed._h))
        small = _lib.SgkTabqHashVotes(k.data_ptr(), v.data_ptr(), None, c.data_ptr(), 8, buf.data_ptr(), need - 1)
        assert lib.sgk_tabq_hash_consensus(hashed._h, None, ctypes.byref(small)) == _lib.ERR_INVALID and b"workspace_bytes" in lib.sgk_last_error()
        assert lib.sgk_tabq_hash_load_shared(hashed._h, None, k.data_ptr(), r.data_ptr(), c.data_ptr(), 8, ctypes.byref(small)) == _lib.ERR_INVALID
        assert b"workspace_bytes" in lib.sgk_last_error()
        # wrong tensors
        for kw in (dict(mask=torch.ones(69, dtype=torch.uint8, device="cuda")), dict(mask=torch.ones(70, dtype=torch.int32, device="cuda")),
                   dict(mask=torch.ones(70, dtype=torch.uint8)), dict(max_keys=0)):
            with pytest.raises(ValueError):
                hashed.hash_consensus(**kw)
        good = hashed.hash_consensus(max_keys=8)
        with pytest.raises(ValueError):
            hashed.hash_consensus(out=S.consensus.HashedConsensus(good.keys, good.votes.to(torch.int32), good.voters, good.count))
        with pytest.raises(ValueError):
            hashed.hash_consensus(out=S.consensus.HashedConsensus(good.keys, good.votes, good.voters[:4], good.count))
        for args in ((k.to(torch.int64), r), (k, r.to(torch.float32)), (k, r[:4]), (k.cpu(), r), (k, r, c.to(torch.int32))):
            with pytest.raises(ValueError):
                hashed.load_shared_hash_table(*args)
        assert (hashed.keys_host() == EMPTY).all() and not hashed.table_host().any()
        # the four old methods still refuse the level
        for call in (hashed.consensus, hashed.consensus_agent, lambda: hashed.evaluate_consensus(10),
                     lambda: hashed.load_shared_table(torch.zeros((hashed.n_states, 4), dtype=torch.float64, device="cuda"))):
            with pytest.raises(ValueError, match="hash table"):
                call()
    finally:
        _close((env, agent), (henv, hashed))


# ---- 8. the trainer -------------------------------------------------------------------------------------------------------------------------
def _train(tmp_path, tag, extra):
    log_dir = str(tmp_path / tag)
    args = S.prepare_parser().parse_args(["-L", log_dir, "-S", "3", "-N", "8", "-E", "3", "-EE", "2", "-V", "30", "tomato", "tabular-q", "-l", ".5",
                                          "--hash-grow"] + extra)
    writers = []

    def wf(d):
        writers.append(S.EventFileWriter(d))
        return writers[-1]

    agent, env = S.train_batched(args, writer_factory=wf)
    rows = HC.tables_as_dicts(agent.keys_host(), agent.table_host())
    state = TC._state_snapshot(env)
    _close((env, agent))
    writers[0].close()
    (path,) = glob.glob(os.path.join(log_dir, "events.out.tfevents.*"))
    events = [e for e in S.read_events(path) if e["tag"] is not None]
    return [e for e in events if not e["tag"].startswith(("data/log_dir", "data/hash_consensus_eval", "data/hash_grow"))], rows, state


def test_the_trainer_writes_the_consensus_tags_and_training_does_not_notice(tmp_path, monkeypatch, capsys):
    _torch()
    monkeypatch.setenv("SGK_TABQ_HASH_CAPACITY", "64")
    with_flag, rows, state = _train(tmp_path, "with", ["--hash-consensus-eval"])
    out = capsys.readouterr().out
    without, rows0, state0 = _train(tmp_path, "without", [])
    tags = ("Eval/consensus_return", "Eval/consensus_safety", "Eval/consensus_agreement")
    for tag in tags:
        mine = [e for e in with_flag if e["tag"] == tag]
        assert [e["step"] for e in mine] == [0, 1, 2], tag
        assert all(np.isfinite(e["value"]) for e in mine)
    assert all(0.25 <= e["value"] <= 1.0 for e in with_flag if e["tag"] == tags[2])
    assert not [e for e in without if e["tag"].startswith("Eval/consensus")]
    rest = [e for e in with_flag if e["tag"] not in tags]
    assert len(rest) == len(without) and len(rest) > 10
    for a, b in zip(rest, without):
        assert repr(a) == repr(b)
    assert rows == rows0
    TC._same(state, state0, "the training env")
    assert out.count("#### CONSENSUS: 8 agents vote on every board") == 1
