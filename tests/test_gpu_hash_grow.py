"""sgk_tabq_hash_grow on the device: the hashed Q-tables of TomatoWatering rehashed into larger ones in the middle of a run, against
the dictionary restatement that "grows" by assignment (tests/hash_grow_plans.py over tests/hashed_tabq_reference.py, which never
evaluates the product's hash function; tests/test_hash_grow_cpu.py asserts what the plans must provide). 322 agents, seed 5.

Held for EVERY agent, after every leg of a plan and through each driving path: the action sequence (where the path hands it out),
the set of keys = the set of admitted boards, every admitted board's row as float64 bit patterns, zero rows in unclaimed slots,
hash_info() = (new capacity, fullest, sticky flag) and the env state.

A growth that loses a row, moves a row to a slot its key's probe sequence does not reach, leaves a stale pending slot in a tag,
keeps a hipGraph that carries the old pointers, or skips agents past the first grid fails here."""
import ctypes
import glob
import os
import types

import numpy as np
import pytest

import hash_grow_plans as G
import hashed_tabq_reference as HR
import safe_grid_agents_amd as S
import test_gpu_parity as P
from safe_grid_agents_amd import _lib

pytestmark = pytest.mark.gpu

EMPTY = G.EMPTY
PATHS = ["calls", "step", "learn_steps", "rollout"]


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _make(capacity, n=HR.N, layout="compact", env_index_base=0, name=HR.NAME):
    _torch()
    env = S.BatchedGridworldEnv(name, n, seed=HR.SEED, layout=layout, env_index_base=env_index_base)
    agent = S.BatchedTabularQAgent(env, types.SimpleNamespace(hash_capacity=capacity, **HR.ARGS))
    return env, agent


def _close(env, agent):
    agent.close()
    env.close()


def _drive(path, env, agent, steps, acts=None, t0=0):
    """`steps` lockstep steps through one driving path; the per-step paths hold every step's actions to acts[t0 + k]."""
    torch = _torch()
    if path == "calls":
        for k in range(steps):
            a = agent.act_explore()
            if acts is not None:
                assert a.cpu().numpy().tobytes() == acts[t0 + k].tobytes(), (path, t0 + k)
            env.step(a, auto_reset=False)
            agent.learn(action=a)
            env.reset_done()
        torch.cuda.synchronize()
    elif path == "step":
        for k in range(steps):
            a, _ = agent.step()
            if acts is not None:
                assert a.cpu().numpy().tobytes() == acts[t0 + k].tobytes(), (path, t0 + k)
    elif path == "learn_steps":
        agent.learn_steps(steps, write_boards=True)
    else:
        agent.rollout(steps, kernel="hbm")


def _rows_by_key(agent, first=0, count=None):
    """[{key: row as four uint64}] per agent, after the checks that need no reference: a board owns one slot, unclaimed slots hold
    zero rows."""
    keys = agent.keys_host(first, count)
    tab = agent.table_host(first, count).view(np.uint64)
    assert keys.shape[1] == agent.n_states == agent.hash_capacity and tab.shape == keys.shape + (4,)
    out = []
    for i in range(keys.shape[0]):
        occ = np.nonzero(keys[i] != EMPTY)[0]
        rows = {int(keys[i, s]): tab[i, s].tolist() for s in occ}
        assert len(rows) == len(occ), (i, "a board owns one slot")
        assert not tab[i][keys[i] == EMPTY].any(), (i, "an unclaimed slot's row is not all zero")
        out.append(rows)
    return out


def _sorted_by_key(agent):
    """(keys uint32 [n, cap] ascending per agent -- the empty marker, the largest word, last --, rows uint64 [n, cap, 4] in that order)"""
    keys, tab = agent.keys_host(), agent.table_host().view(np.uint64)
    order = np.argsort(keys, axis=1, kind="stable")
    return np.take_along_axis(keys, order, axis=1), np.take_along_axis(tab, order[:, :, None], axis=1)


def _assert_tables(agent, ref, where):
    """Every agent's table against its dictionary: keys, rows, empty slots; then hash_info() against the whole population."""
    R = G.rules()
    got = _rows_by_key(agent)
    assert len(got) == len(ref)
    for i, (rows, a) in enumerate(zip(got, ref)):
        by_board = {G.board_of_key(R, k): v for k, v in rows.items()}
        assert len(by_board) == len(rows) == a.n_rows, (where, i, len(rows), a.n_rows)
        missing, extra = set(a.rows) - set(by_board), set(by_board) - set(a.rows)
        assert not missing and not extra, (where, i, "missing", len(missing), "extra", len(extra))
        for board, row in a.rows.items():
            assert by_board[board] == np.array(row, dtype=np.float64).view(np.uint64).tolist(), (where, i, row)
    assert agent.hash_info() == HR.hash_info(ref), (where, agent.hash_info(), HR.hash_info(ref))


def _assert_leg(env, agent, leg, where):
    assert agent.t == leg.t_end and agent.n_states == agent.hash_capacity == leg.capacity
    P.assert_same_state(env, leg.snapshot, where)
    _assert_tables(agent, leg.agents, where)


# ---- 1. the plans through every driving path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("plan", ["A", "B", "C"])
def test_a_grown_run_equals_the_dictionary_after_every_leg(plan, path):
    """A: tables grown while below capacity, exactly full, and after refusals, then room for all. B: a second overflow behind the
    growth. C: two growths, never a refusal. The per-step calls follow the reference's order around an episode boundary, the fused
    ones their own (include/sgk.h), as in test_gpu_hashed_tabq.py."""
    legs = G.run_plan(G.PLANS[plan], claim_start_on_reset=path != "calls")
    env, agent = _make(legs[0].capacity, layout="pitched" if path == "calls" else "compact")
    try:
        for k, leg in enumerate(legs):
            if k:
                assert agent.grow_hash(leg.capacity) == leg.capacity
                # the growth itself: nothing but the capacity changed
                _assert_tables(agent, [_at(a, leg.capacity) for a in legs[k - 1].agents], "plan %s %s: behind growth %d" % (plan, path, k))
            _drive(path, env, agent, leg.steps, leg.acts, 0)
            _assert_leg(env, agent, leg, "plan %s %s: leg %d" % (plan, path, k))
    finally:
        _close(env, agent)


def _at(a, capacity):
    """A dictionary as it is, at another capacity (a shallow stand-in: the rows are shared and only read)."""
    b = HR.CappedTabQ(a.lr, a.discount, capacity)
    b.rows, b.overflowed, b.refused = a.rows, a.overflowed, a.refused
    return b


def test_evaluate_behind_a_growth_claims_what_the_dictionary_claims():
    """Plan A's first leg, the growth to 128, then evaluate(1): a reset and one greedy episode, whose act() claims slots of its own
    in the grown tables -- rows of zeros, the ones the dictionary admits -- and leaves every learnt row, t and epsilon alone."""
    import copy

    leg1 = G.run_plan(G.PLANS["A"], True)[0]
    envs = HR.O.EnvBatch(HR.NAME, HR.N, seed=HR.SEED, env_begin=0)
    ref = [_at(a, 128) for a in copy.deepcopy(leg1.agents)]
    env, agent = _make(64)
    try:
        agent.rollout(leg1.steps, kernel="hbm")
        agent.grow_hash(128)
        before = _rows_by_key(agent)
        eps0 = agent.epsilon
        got = agent.evaluate(1, kernel="hbm")
        # (the oracle's envs stand at their initial state: H.evaluate resets every env first, as evaluate() does; tomato watering's own
        # draws are keyed by the env's step count, which the device carries on from the training steps)
        for e in range(HR.N):
            for a in leg1.acts[:, e]:
                if envs.step(e, int(a))[2]:
                    envs.reset(e)
        HR.evaluate(envs, ref, 0, int(env.info.max_iterations))
        assert got.episodes == HR.N and agent.t == leg1.t_end and float(agent.epsilon).hex() == float(eps0).hex()
        after = _rows_by_key(agent)
        claimed = 0
        for b, a in zip(before, after):
            assert all(a[k] == v for k, v in b.items())
            assert all(v == [0, 0, 0, 0] for k, v in a.items() if k not in b)
            claimed += len(a) - len(b)
        assert claimed == sum(r.n_rows - a.n_rows for r, a in zip(ref, leg1.agents)) > 0
        P.assert_same_state(env, envs, "after the evaluation")
        _assert_tables(agent, ref, "after the evaluation")
    finally:
        _close(env, agent)


# ---- 2. the claim behind --hash-grow ------------------------------------------------------------------------------------------------------
def test_a_run_grown_before_any_refusal_equals_one_created_large():
    """Plan D on the device against a device agent created at capacity 256: the same actions at every step, the same rows by key --
    and both equal the dictionary."""
    legs = G.run_plan(G.PLANS["D"], True)
    acts = np.concatenate([l.acts for l in legs])
    env, agent = _make(64)
    env2, agent2 = _make(256)
    try:
        _drive("step", env, agent, legs[0].steps, acts, 0)
        agent.grow_hash(256)
        _drive("step", env, agent, legs[1].steps, acts, legs[0].steps)
        _drive("step", env2, agent2, legs[1].t_end, acts, 0)
        assert _rows_by_key(agent) == _rows_by_key(agent2)
        assert agent.hash_info() == agent2.hash_info() == (256, 117, False)
        _assert_leg(env, agent, legs[1], "plan D, grown")
        _assert_leg(env2, agent2, legs[1], "plan D, created at 256")
    finally:
        _close(env, agent)
        _close(env2, agent2)


# ---- 3. an action chosen before the growth is learnt from behind it ---------------------------------------------------------------------
def test_a_pending_action_survives_the_growth():
    """30 steps at capacity 64 (nobody refused yet), then act_explore(), grow_hash(256), env.step, learn, reset_done and 20 more
    steps: learn() finds the row its act() chose from through the tag's pending slot, which has to name the board's NEW slot."""
    legs = G.run_plan([(64, 30), (256, 21)], claim_start_on_reset=False)
    assert not any(any(l.refused_in_leg) for l in legs)
    env, agent = _make(64, layout="pitched")
    try:
        _drive("calls", env, agent, 30, legs[0].acts, 0)
        a = agent.act_explore()
        assert a.cpu().numpy().tobytes() == legs[1].acts[0].tobytes()
        assert agent.grow_hash(256) == 256
        env.step(a, auto_reset=False)
        agent.learn(action=a)
        env.reset_done()
        _drive("calls", env, agent, 20, legs[1].acts, 1)
        _assert_leg(env, agent, legs[1], "pending action")
    finally:
        _close(env, agent)


# ---- 4. the recorded hipGraphs carry the old pointers -------------------------------------------------------------------------------------
def _tabq_graphs(env, agent):
    n = ctypes.c_int32(-1)
    _lib.check(env.lib.sgk_debug_graph_count(env.handle, agent._h, None, ctypes.byref(n)))
    return n.value


def test_the_growth_drops_the_recorded_graphs():
    legs = G.run_plan([(64, 48), (128, 8)], claim_start_on_reset=True)
    env, agent = _make(64)
    try:
        agent.rollout(40, kernel="hbm")
        agent.learn_steps(8, write_boards=True)
        assert _tabq_graphs(env, agent) == 1
        _assert_leg(env, agent, legs[0], "before the growth")
        agent.grow_hash(128)
        # a graph left here would be replayed by the next call -- same key -- with the freed arrays as its arguments: stop first
        assert _tabq_graphs(env, agent) == 0, "the growth left a hipGraph that carries the old pointers"
        agent.learn_steps(8, write_boards=True)
        assert _tabq_graphs(env, agent) == 1
        _assert_leg(env, agent, legs[1], "replay behind the growth")
    finally:
        _close(env, agent)


# ---- 5. more agents than one grid of lanes ------------------------------------------------------------------------------------------------
def test_the_growth_reaches_every_agent_of_a_grid_stride_launch(monkeypatch):
    """16 384 + 322 agents on a handle whose grids are capped at 64 workgroups (SGK_MAX_GRID, read at sgk_create): the growth kernel
    walks them in a grid-stride loop. 60 steps, grow_hash(256), 40 more; the last 322 agents equal a 322-agent handle created at
    env_index_base 16 384 that did the same (the counter RNG is keyed by global env id)."""
    base = 16384
    monkeypatch.setenv("SGK_MAX_GRID", "64")
    env, agent = _make(64, n=base + HR.N)
    monkeypatch.delenv("SGK_MAX_GRID")
    env2, agent2 = _make(64, env_index_base=base)
    try:
        for steps in (60, 40):
            for _ in range(steps):
                a, _ = agent.step()
                a2, _ = agent2.step()
                assert a[base:].cpu().numpy().tobytes() == a2.cpu().numpy().tobytes(), agent.t
            if steps == 60:
                before = _sorted_by_key(agent)
                assert agent.grow_hash(256) == 256 and agent2.grow_hash(256) == 256
                after = _sorted_by_key(agent)
                # EVERY agent of the large handle came through the growth: its keys and, key by key, its rows (at most 64 each)
                assert (before[0] != EMPTY).any(axis=1).all() and after[0].shape == (base + HR.N, 256)
                assert (after[0][:, :64] == before[0]).all() and (after[0][:, 64:] == EMPTY).all()
                assert (after[1][:, :64] == before[1]).all() and not after[1][:, 64:].any()
        tail, small = _rows_by_key(agent, base, HR.N), _rows_by_key(agent2)
        assert tail == small and max(len(r) for r in small) > 64  # (somebody crossed the old capacity)
        assert agent.hash_info()[0] == 256 and not agent2.hash_info()[2]
    finally:
        _close(env, agent)
        _close(env2, agent2)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing():
    """A smaller capacity, a non-power of two, out-of-range capacities: SGK_ERR_INVALID with a message; keys, table and hash_info()
    as bytes afterwards, and -- no call reads the tags -- the action that was pending is still learnt from: the run goes on to equal
    the dictionary. An equal capacity is a no-op."""
    legs = G.run_plan([(128, 40), (128, 11)], claim_start_on_reset=False)
    env, agent = _make(128, layout="pitched")
    try:
        _drive("calls", env, agent, 40, legs[0].acts, 0)
        a = agent.act_explore()
        keys0, tab0, info0 = agent.keys_host(), agent.table_host(), agent.hash_info()
        for capacity, word in [(64, b"below the current"), (96, b"power of two"), (192, b"power of two"), (0, b"power of two"),
                               (-128, b"power of two"), (1 << 25, b"power of two")]:
            assert env.lib.sgk_tabq_hash_grow(agent._h, capacity) == _lib.ERR_INVALID, capacity
            assert word in env.lib.sgk_last_error(), (capacity, env.lib.sgk_last_error())
            with pytest.raises(RuntimeError):
                agent.grow_hash(capacity)
        assert agent.grow_hash(128) == 128  # a no-op
        assert agent.n_states == agent.hash_capacity == 128 and agent.hash_info() == info0
        assert agent.keys_host().tobytes() == keys0.tobytes() and agent.table_host().tobytes() == tab0.tobytes()
        env.step(a, auto_reset=False)
        agent.learn(action=a)
        env.reset_done()
        _drive("calls", env, agent, 10, legs[1].acts, 1)
        _assert_leg(env, agent, legs[1], "behind the refused calls")
    finally:
        _close(env, agent)


def test_a_perfect_hash_level_is_refused():
    env, agent = _make(0, n=70, name="IslandNavigation-v0")
    try:
        agent.rollout(20)
        tab0, ns = agent.table_host(), agent.n_states
        assert env.lib.sgk_tabq_hash_grow(agent._h, 128) == _lib.ERR_INVALID and b"perfect hash" in env.lib.sgk_last_error()
        with pytest.raises(RuntimeError):
            agent.grow_hash(128)
        with pytest.raises(RuntimeError):
            agent.reserve_hash(10)
        assert agent.n_states == ns and agent.hash_info() == (0, 0, False) and agent.table_host().tobytes() == tab0.tobytes()
    finally:
        _close(env, agent)


def test_reserve_hash_grows_to_the_bound_and_no_further():
    env, agent = _make(64)
    try:
        assert agent.reserve_hash(31) == 64 and agent.hash_info() == (64, 0, False)  # 0 + 62 + 1 fits
        assert agent.reserve_hash(32) == 128  # 0 + 64 + 1 does not
        agent.rollout(30, kernel="hbm")
        used = agent.hash_info()[1]
        assert 1 <= used <= 61  # (a step admits two boards at most)
        assert agent.reserve_hash(10) == 128 and agent.reserve_hash((256 - used - 1) // 2) == 256
        assert agent.reserve_hash((256 - used - 1) // 2 + 1) == 512 == agent.n_states == agent.hash_info()[0]
        with pytest.raises(RuntimeError, match="2\\^24"):
            agent.reserve_hash(1 << 23)
        assert agent.hash_info() == (512, used, False)
    finally:
        _close(env, agent)


# ---- 7. the trainer -----------------------------------------------------------------------------------------------------------------------
def _train(tmp_path, tag, extra):
    log_dir = str(tmp_path / tag)
    args = S.prepare_parser().parse_args(["-L", log_dir, "-S", "5", "-N", str(HR.N), "-E", "3", "-EE", "2", "-V", "30", "tomato", "tabular-q",
                                          "-l", ".4", "-e", ".3", "-dl", "400"] + extra)
    writers = []

    def wf(d):
        writers.append(S.EventFileWriter(d))
        return writers[-1]

    agent, env = S.train_batched(args, writer_factory=wf)
    rows, info = _rows_by_key(agent), agent.hash_info()
    _close(env, agent)
    writers[0].close()
    (path,) = glob.glob(os.path.join(log_dir, "events.out.tfevents.*"))
    events = [e for e in S.read_events(path) if e["tag"] is not None]  # (the file_version record carries none)
    return [e for e in events if not e["tag"].startswith(("data/log_dir", "data/hash_grow"))], rows, info


def test_the_trainer_grows_where_it_stopped_before(tmp_path, monkeypatch):
    """Three training periods of 100 steps and three evaluations from SGK_TABQ_HASH_CAPACITY=64: without --hash-grow the run stops
    with the overflow message at the first period; with it the run finishes, nobody was ever refused, and its event files and final
    tables, by key, are those of the same run started at a capacity it never reaches."""
    _torch()
    monkeypatch.setenv("SGK_TABQ_HASH_CAPACITY", "64")
    with pytest.raises(RuntimeError, match="re-run with a larger table"):
        _train(tmp_path, "stops", [])
    events, rows, info = _train(tmp_path, "grows", ["--hash-grow"])
    monkeypatch.setenv("SGK_TABQ_HASH_CAPACITY", str(1 << 12))
    events0, rows0, info0 = _train(tmp_path, "large", [])
    assert info[0] > 64 and info[1] == info0[1] > 64 and not info[2] and not info0[2] and info0[0] == 1 << 12
    assert len(events) == len(events0) > 10
    for a, b in zip(events, events0):
        assert repr(a) == repr(b)
    assert rows == rows0
