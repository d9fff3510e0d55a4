"""The hashed Q-tables of TomatoWatering under load, against a dictionary with a capacity (tests/hashed_tabq_reference.py, which
never evaluates the product's hash function): 322 private agents at capacity 64 for 99 steps, after which 184 tables have room, 16
are EXACTLY full without ever having refused a board and 122 have overflowed (test_hashed_tabq_reference_cpu.py asserts those
conditions on the reference alone). Every path that can reach a hashed table is held to it, for EVERY agent:

  the action sequence, where the path hands it out; the set of keys = the set of admitted boards (no duplicates, 0xffffffff
  elsewhere, used = min(64, admitted)), each key rendered to its board through the product's level tables; every admitted board's
  row as float64 bit patterns; every unclaimed slot's row all zero; hash_info(); the env state at the end.

A probe loop one slot short loses the last board of an exactly full table whose chain wraps; a full-table lookup that answers
some occupied slot learns into another board's row; a hand-off (tags / row_cache) that keeps a row for a board that got none
(si = -1) acts or learns on stale values: each changes an action, a key set or a row here.

One case crosses the episode boundary at capacity 64 with agents created one env step into the episode, so that the next episode's
start board is NEW to them: the fused calls claim it in the step that ends the episode, the per-step calls at the next act
(include/sgk.h), and a run that stops on the boundary differs between the two in 156 agents' tables. One case runs at capacity 128,
where nobody overflows and the fullest table is above 60 % load."""
import types

import numpy as np
import pytest

import hashed_tabq_reference as HR
import hostlib
import safe_grid_agents_amd as S
import test_gpu_parity as P
import test_tables_cpu as TT

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
ROOMY = 1 << 20


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _make(capacity, layout="compact", pre_step=False):
    torch = _torch()
    env = S.BatchedGridworldEnv(HR.NAME, HR.N, seed=HR.SEED, layout=layout)
    if pre_step:  # the envs move before their agents exist: the episode's start board is a board no agent has looked up
        env.step(torch.as_tensor(HR.pre_actions(HR.N), device="cuda"), auto_reset=False)
    agent = S.BatchedTabularQAgent(env, types.SimpleNamespace(hash_capacity=capacity, **HR.ARGS))
    assert agent.n_states == capacity and agent.hash_info() == (capacity, 0, False)
    return env, agent


_BOARDS = {}


def _board_of_key(R, key):
    """The board a slot's key names (sgk.h: agent cell | shown watered set << 8, 0x2000 = the bucket's delusion board), rendered
    from the product's level tables as _assert_hashed_tables_equal of test_gpu_parity.py renders it."""
    if key not in _BOARDS:
        cell, shown = key & 0xFF, key >> 8
        assert (shown == 0x2000) == (cell == R.aux_cell), hex(key)  # the delusion board shows exactly on the bucket
        ti = R.tomato_index[cell]
        assert shown == 0x2000 or ti == 255 or not (shown >> ti) & 1, hex(key)  # the tomato under the agent does not show
        _BOARDS[key] = TT._product_board(HR.NAME, R, cell, shown & 0x1FFF, 0).astype(np.int8).tobytes()
    return _BOARDS[key]


def _assert_tables(agent, ref, where):
    """Every agent's table against its dictionary: keys, rows, empty slots; then hash_info() against the whole population."""
    R = TT._rules(hostlib.load(), S.ENV_IDS[HR.NAME])
    keys, tab = agent.keys_host(), agent.table_host().view(np.uint64)
    cap = ref[0].capacity
    assert keys.shape == (len(ref), cap) and tab.shape == (len(ref), cap, 4)
    for i, a in enumerate(ref):
        occ = np.nonzero(keys[i] != EMPTY)[0]
        held = [int(k) for k in keys[i, occ]]
        assert len(set(held)) == len(held), (where, i, "a board owns one slot")
        slot_of = {_board_of_key(R, k): int(s) for k, s in zip(held, occ)}
        assert len(slot_of) == len(held), (where, i)
        assert len(held) == a.n_rows == min(cap, a.n_rows), (where, i, len(held), a.n_rows)
        missing, extra = set(a.rows) - set(slot_of), set(slot_of) - set(a.rows)
        assert not missing and not extra, (where, i, "boards held", len(held), "missing", len(missing), "extra", len(extra))
        for board, row in a.rows.items():
            got = tab[i, slot_of[board]]
            assert got.tolist() == np.array(row, dtype=np.float64).view(np.uint64).tolist(), (where, i, slot_of[board], row)
        assert not tab[i][keys[i] == EMPTY].any(), (where, i, "an unclaimed slot's row is not all zero")
    assert agent.hash_info() == HR.hash_info(ref), (where, agent.hash_info(), HR.hash_info(ref))


def _assert_outcomes(ref, steps=HR.T, claim=False, pre_steps=0):
    """Each agent's own outcome, on the reference the device was just held to: the exactly full are full and were never refused,
    the overflowed hold exactly the first `capacity` boards the unbounded agent admits."""
    _, roomy, _ = HR.run(ROOMY, steps, claim_start_on_reset=claim, pre_steps=pre_steps)
    below, full, over = HR.classes(ref)
    cap = ref[0].capacity
    for i in full:
        assert ref[i].n_rows == cap == roomy[i].n_rows and ref[i].refused == 0
    for i in over:
        assert ref[i].refused > 0 and list(ref[i].rows) == list(roomy[i].rows)[:cap]
    for i in below:
        assert list(ref[i].rows) == list(roomy[i].rows)
    return below, full, over


def _finish(env, agent, orc, ref, where, steps=HR.T):
    assert agent.t == steps
    P.assert_same_state(env, orc, where)
    _assert_tables(agent, ref, where)
    agent.close()
    env.close()


@pytest.mark.parametrize("capacity", [64, 128])
def test_act_explore_env_step_learn_as_separate_calls(capacity):
    torch = _torch()
    orc, ref, acts = HR.run(capacity)
    below, full, over = _assert_outcomes(ref)
    assert (capacity == 64 and len(full) >= 3 and len(over) >= 8) or (capacity == 128 and not over and not full)
    env, agent = _make(capacity, layout="pitched")
    for t in range(HR.T):
        a = agent.act_explore()
        got = a.cpu().numpy()
        assert got.tobytes() == acts[t].tobytes(), (t, np.nonzero(got != acts[t])[0][:5])
        env.step(a, auto_reset=False)
        agent.learn(action=a)
        env.reset_done()
    torch.cuda.synchronize()
    _finish(env, agent, orc, ref, "separate calls, capacity %d" % capacity)


@pytest.mark.parametrize("layout", ["pitched", "compact"])
def test_agent_step(layout):
    orc, ref, acts = HR.run(64)
    env, agent = _make(64, layout)
    for t in range(HR.T):
        a, _ = agent.step()
        got = a.cpu().numpy()
        assert got.tobytes() == acts[t].tobytes(), (t, np.nonzero(got != acts[t])[0][:5])
    _finish(env, agent, orc, ref, "agent.step")


def test_learn_steps_from_the_graph():
    orc, ref, _ = HR.run(64)
    env, agent = _make(64)
    agent.learn_steps(HR.T, write_boards=True)
    _finish(env, agent, orc, ref, "learn_steps")


@pytest.mark.parametrize("capacity", [64, 128])
def test_rollout_with_the_hbm_kernel(capacity):
    orc, ref, _ = HR.run(capacity)
    env, agent = _make(capacity)
    agent.rollout(40, kernel="hbm")  # (two launches: the second comes in with tables in use)
    agent.rollout(HR.T - 40, kernel="hbm")
    _finish(env, agent, orc, ref, "rollout hbm, capacity %d" % capacity)


@pytest.mark.parametrize("path", ["calls", "step", "learn_steps", "rollout"])
def test_across_the_episode_boundary(path):
    """The envs take one step, THEN the agents are created: nobody has looked the episode's start board up when the episode ends
    at agent step 99. The fused calls look the next episode's start board up in the step that ends the episode, behind s'; the
    per-step calls (act_explore, env.step, learn, reset_done) at the next act. No lookup lies in between, so the order of admission
    is the same and a run that stops ON the boundary tells the two apart: on the reference 156 agents hold one board more under
    the first order, and 15 that are exactly full and never refused under the second have been refused under the first. Compared
    there, then 31 steps on (T = 130), where both orders have come to the same tables."""
    torch = _torch()
    claim = path != "calls"
    _, other, _ = HR.run(64, 99, claim_start_on_reset=not claim, pre_steps=1)
    env, agent = _make(64, layout="pitched" if path == "calls" else "compact", pre_step=True)
    for steps in (99, 130):
        orc, ref, acts = HR.run(64, steps, claim_start_on_reset=claim, pre_steps=1)
        _assert_outcomes(ref, steps, claim=claim, pre_steps=1)
        more = steps - agent.t
        if path == "calls":
            for t in range(agent.t, steps):
                a = agent.act_explore()
                assert a.cpu().numpy().tobytes() == acts[t].tobytes(), t
                env.step(a, auto_reset=False)
                agent.learn(action=a)
                env.reset_done()
            torch.cuda.synchronize()
        elif path == "step":
            for t in range(agent.t, steps):
                a, _ = agent.step()
                assert a.cpu().numpy().tobytes() == acts[t].tobytes(), t
        elif path == "learn_steps":
            agent.learn_steps(more, write_boards=True)
        else:
            agent.rollout(more, kernel="hbm")
        assert agent.t == steps
        P.assert_same_state(env, orc, "%s at step %d" % (path, steps))
        _assert_tables(agent, ref, "%s at step %d" % (path, steps))
        if steps == 99:  # the other order would have failed just now: the inputs tell the two apart, a full agent among them
            differ = [i for i, (a, b) in enumerate(zip(ref, other)) if set(a.rows) != set(b.rows)]
            flips = [i for i, (a, b) in enumerate(zip(ref, other)) if a.overflowed != b.overflowed]
            assert len(differ) >= 8 and len(flips) >= 1, (len(differ), len(flips))
            assert (env.last_episode_host()["n_episodes"] == 1).all()
    agent.close()
    env.close()


def test_evaluate_with_the_hbm_kernel_claims_what_the_reference_claims():
    """80 learning steps leave 316 tables below the limit, the fullest at it; evaluate(1) -- a reset and one greedy episode --
    looks up boards of its own and fills and overflows dozens more. It leaves tables, t and epsilon as bytes apart from the slots
    it claims, and those are the ones the reference claims (rows of zeros)."""
    train = 80
    orc, trained, ref = HR.run_then_evaluate(64, train)
    env, agent = _make(64)
    agent.rollout(train, kernel="hbm")
    _assert_tables(agent, trained, "before the evaluation")
    keys0, tab0 = agent.keys_host().copy(), agent.table_host().view(np.uint64).copy()
    t0, eps0 = agent.t, agent.epsilon
    got = agent.evaluate(1, kernel="hbm")
    assert got.episodes == HR.N and agent.t == t0 == train and float(agent.epsilon).hex() == float(eps0).hex()
    keys1, tab1 = agent.keys_host(), agent.table_host().view(np.uint64)
    was = keys0 != EMPTY
    assert (keys1[was] == keys0[was]).all() and tab1.tobytes() == tab0.tobytes()  # claimed slots hold rows of zeros, as they did empty
    claimed = (keys1 != EMPTY) & ~was
    assert claimed.sum() == sum(b.n_rows - a.n_rows for a, b in zip(trained, ref)) > 0
    P.assert_same_state(env, orc, "after the evaluation")
    _assert_tables(agent, ref, "after the evaluation")
    agent.close()
    env.close()
