"""Device sweeps: every scriptable device path executes EVERY reachable (agent cell, second sprite cell, coin / mode bit, action)
of the seven deterministic levels and is held to the oracle's trace (tests/state_sweep.py) after EVERY step -- step records and
dense boards as bytes, the fields of episode_state_host() / last_episode_host(), the metrics at the end. The coverage is asserted
on the oracle's trace and the device is asserted equal to that trace step by step, so the coverage transfers to the device: to its
board writers (write_board_pitched, the compact / rotated writer, write_row_bytes behind the replay rings, the tile writer of the step server) and to its
state carriers (the state word in HBM, the registers of the fused tabular-Q kernels, tabq_eval_kernel's packed policy, the row
cache of tabq_step_kernel, the step server's mailbox). No probe depends on luck: each is a scripted shortest path of at most 21
steps (ConveyorBelt's deepest state needs a 19-step push sequence no random walk forces).

Paths: env.step (both layouts, with and without auto-reset, both instantiations of step_kernel: SMALL serves every batch of up to
65 536 envs -- sgk_step.hip, STEP_SMALL_MAX_ENVS --, so one BoatRace case deals the probes over 65 637 envs to reach the other);
sgk_step_host through the step server in batches of at most 64 envs; step_store + reset_done_store into rings that wrap; the
tabular-Q agents acting greedily on private scripted policies (epsilon 0, lr 0): act + env.step, step, learn_steps, rollout
lds / hbm, evaluate lds / hbm, the tables' bytes unchanged behind every learning call.

WhiskyGold, TomatoWatering and FriendFoe draw by themselves: they run the action-script paths without a coverage requirement HERE.
Theirs is stated in events and planned per env around that env's own draws: test_gpu_tomato_sweep.py (TomatoWatering) and
test_gpu_draw_sweeps.py (WhiskyGold and FriendFoe, the time limit and FriendFoe's estimates behind every step included).

"Every scriptable path" is no wider than this list. Not swept: the grid-stride instantiations above 65 536 envs of anything but
env.step on BoatRace (step_store's STORE form and tabq_step_kernel among them); tabq act + env.step on a compact handle (it runs
pitched; the fused tabular-Q calls run on both); the step server on levels other than BoatRace, IslandNavigation, AbsentSupervisor and ConveyorBelt.

Elsewhere: sgk_rollout_random(_stream), sgk_policy_rollout* and sgk_convq_rollout* choose their own actions and take no script.
What each draws at the first step of a launch is known before the launch, so test_gpu_rollout_sweep.py deals every reachable state
to envs that are going to draw the action it still needs, plants them through env.step and env.reset(mask) -- both swept here --
and holds step 0 of the launch, which executes every pair, and a K-step continuation to the oracle (tests/rollout_sweep.py)."""
import contextlib
import types

import numpy as np
import pytest

import safe_grid_agents_amd as S
import state_sweep as SS
from oracle import oracle as O
from safe_grid_agents_amd import _lib
from test_state_sweep_cpu import _idle_schedule

pytestmark = pytest.mark.gpu

SEED = SS.SEED
TABQ_LEVELS = SS.SWEPT
LDS_LEVELS = tuple(name for name in SS.SWEPT if SS.lds_resident(name))
# the step server: a level without a second sprite, one with hidden state, one with two backdrops and a coin, and ConveyorBelt, whose
# 3 024 probes (48 handles) make the resident wave draw the second sprite in every reachable place
SERVER_LEVELS = ("BoatRace-v0", "IslandNavigation-v0", "AbsentSupervisor-v0", "ConveyorBelt-v0")
EVAL_TAIL = 100  # env.info.max_iterations of every level: the steps evaluate() runs without reset


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _assert_covered(name, tr):
    """The condition the sweep exists for: the trace the device is held to executes every reachable pair."""
    if name in SS.SWEPT:
        _, pairs = SS.reachable_pairs(name)
        assert pairs <= tr.pairs, (name, sorted(pairs - tr.pairs)[:5])


def _same_bytes(got, want, where):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (where, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1))[0]
        raise AssertionError("%s: rows %s differ\n%s\n%s" % (where, bad[:5], got[bad[0]], want[bad[0]]))


def _assert_state(env, boards, fields, where, lo=0, hi=None):
    """Boards and every state field of the env against one step of a trace (envs lo .. hi of it)."""
    hi = lo + env.n_envs if hi is None else hi
    _same_bytes(env.boards_host().reshape(env.n_envs, -1), boards[lo:hi], where + " boards")
    st, le = env.episode_state_host(), env.last_episode_host()
    for got, key in ((st["episode_return"], "episode_return"), (st["hidden_return"], "hidden_return"), (st["frame"], "frame"),
                     (st["over"], "game_over"), (st["agent_cell"], "agent_cell"), (st["box_cell"], "box_cell"),
                     (le["n_episodes"], "n_episodes")):
        want = fields[key][lo:hi]
        bad = np.nonzero(got.astype(np.int64) != want)[0]
        assert bad.size == 0, "%s %s differs at envs %s: %s / %s" % (where, key, bad[:5], got[bad[:5]], want[bad[:5]])
    fin = le["n_episodes"] > 0
    assert (le["last_performance"][fin] == fields["last_performance"][lo:hi][fin]).all(), where + " last_performance"
    assert (le["last_return"][fin] == fields["last_episode_return"][lo:hi][fin]).all(), where + " last_return"


def _assert_step(env, tr, t, where, lo=0, hi=None):
    hi = lo + env.n_envs if hi is None else hi
    _same_bytes(env.step_records_host(), tr.recs[t, lo:hi], "%s t=%d records" % (where, t))
    _assert_state(env, tr.boards[t], {k: v[t] for k, v in tr.fields.items()}, "%s t=%d" % (where, t), lo, hi)


def _assert_end(env, tr, where):
    assert env.metrics().tolist() == tr.metrics.tolist(), where
    if env.name == "FriendFoe-v0":
        assert (env.bandit_policy().view(np.uint64) == tr.orc.foe_policy().view(np.uint64)).all(), where


# ---- env.step(actions) ---------------------------------------------------------------------------------------------------------
def _run_env_step(name, layout, mode, n=None):
    torch = _torch()
    T = SS.SIZES[name][1]
    schedule = True if mode == "auto" else _idle_schedule(T)
    tr = SS.sweep(name, "actions", schedule, n=n)
    _assert_covered(name, tr)
    env = S.BatchedGridworldEnv(name, tr.n, seed=SEED, layout=layout)
    _assert_state(env, tr.boards0, tr.fields0, "after create")
    for t in range(tr.T):
        env.step(torch.as_tensor(tr.actions[t], device="cuda"), auto_reset=mode == "auto")
        if tr.schedule[t] == "reset":  # without auto-reset finished envs idle until the caller resets them
            env.reset_done()
        _assert_step(env, tr, t, "%s %s %s" % (name, layout, mode))
    _assert_end(env, tr, name)
    env.close()


@pytest.mark.parametrize("name", SS.SWEPT + SS.UNSWEPT)
@pytest.mark.parametrize("layout", ["pitched", "compact"])
@pytest.mark.parametrize("mode", ["auto", "idle"])
def test_env_step_executes_every_pair(name, layout, mode):
    """With auto-reset the board behind a terminal probe is the next episode's first board, coin redrawn; without, the finished
    envs idle (reward 0, done 1) until reset_done() behind every 5th step."""
    _run_env_step(name, layout, mode)


@pytest.mark.parametrize("layout", ["pitched", "compact"])
def test_env_step_executes_every_pair_in_the_grid_stride_kernel(layout):
    """step_kernel<SMALL = false>: batches above STEP_SMALL_MAX_ENVS = 65 536 envs (whole 64-env tiles, a tile of 37, a grid
    that strides); BoatRace's 32 probes dealt again and again over 65 637 envs."""
    _run_env_step("BoatRace-v0", layout, "auto", n=65536 + 64 + 37)


# ---- sgk_step_host / the step server ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SERVER_LEVELS)
@pytest.mark.parametrize("mode", ["auto", "idle"])
def test_step_server_executes_every_pair(name, mode):
    """Host-visible handles of at most 64 envs, each created at the global index of its first probe (the coins are keyed by it):
    every sgk_step_host is served by the resident wave through the mailbox; reset_done() in between stops it and the next step
    starts another."""
    _torch()
    T = SS.SIZES[name][1]
    schedule = True if mode == "auto" else _idle_schedule(T)
    tr = SS.sweep(name, "actions", schedule)
    _assert_covered(name, tr)
    sums = np.zeros(8, dtype=np.int64)
    maxima = np.full(4, np.iinfo(np.int64).min, dtype=np.int64)
    for lo in range(0, tr.n, 64):
        cnt = min(64, tr.n - lo)
        env = S.BatchedGridworldEnv(name, cnt, seed=SEED, env_index_base=lo, host_visible=True)
        rec = np.zeros((cnt, 4), dtype=np.int8)
        boards = np.zeros((cnt, env.n_cells), dtype=np.int8)
        ret = np.zeros(cnt, dtype=np.int32)
        for t in range(tr.T):
            acts = np.ascontiguousarray(tr.actions[t, lo:lo + cnt])
            _lib.check(env.lib.sgk_step_host(env.handle, acts.ctypes.data, _lib.F_AUTO_RESET if mode == "auto" else 0, rec.ctypes.data,
                                             boards.ctypes.data, ret.ctypes.data))
            where = "%s %s envs %d.. t=%d" % (name, mode, lo, t)
            _same_bytes(rec, tr.recs[t, lo:lo + cnt], where + " records")
            if tr.schedule[t] == "reset":
                _same_bytes(boards, tr.boards_pre[t, lo:lo + cnt], where + " boards")
                env.reset_done()
                _assert_step(env, tr, t, where, lo)
            else:
                _same_bytes(boards, tr.boards[t, lo:lo + cnt], where + " boards")
                assert (ret == tr.fields["episode_return"][t, lo:lo + cnt]).all(), where
        _assert_step(env, tr, tr.T - 1, "%s %s envs %d.. at the end" % (name, mode, lo), lo)
        m = env.metrics()
        sums += m[:8]
        maxima = np.maximum(maxima, m[8:12])
        env.close()
    assert sums.tolist() == tr.metrics[:8].tolist()
    assert maxima.tolist() == tr.metrics[8:12].tolist()


# ---- env.step_store + sgk_reset_done_store ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SS.SWEPT)
@pytest.mark.parametrize("layout", ["pitched", "compact"])
@pytest.mark.parametrize("cheat", [False, True])
@pytest.mark.parametrize("slice_on_device", [False, True])
def test_step_store_and_reset_done_store_execute_every_pair(name, layout, cheat, slice_on_device):
    """Replay rings of 5 slices, fewer than T, so they wrap: every slice is compared before it is overwritten -- the successor
    boards, action, reward and terminal flag of step_store, the reset boards of reset_done_store -- with the slice named by the
    host and by the device scalar."""
    torch = _torch()
    T, ring = SS.SIZES[name][1], 5
    tr = SS.sweep(name, "actions", ["reset"] * T)
    _assert_covered(name, tr)
    n = tr.n
    env = S.BatchedGridworldEnv(name, n, seed=SEED, layout=layout)
    succ = torch.full((ring, n, env.n_cells), -7, dtype=torch.int8, device="cuda")
    states = torch.full((ring, n, env.n_cells), -7, dtype=torch.int8, device="cuda")
    ract = torch.full((ring, n), 99, dtype=torch.uint8, device="cuda")
    rrew = torch.full((ring, n), -7, dtype=torch.int8, device="cuda")
    rterm = torch.full((ring, n), 9, dtype=torch.uint8, device="cuda")
    base = 3 if slice_on_device else 0
    slice_dev = torch.tensor([base], dtype=torch.int64, device="cuda") if slice_on_device else None
    for t in range(T):
        where = "%s %s t=%d" % (name, layout, t)
        env.step_store(torch.as_tensor(tr.actions[t], device="cuda"), t, (succ, ract, rrew, rterm), cheat=cheat, slice_dev=slice_dev)
        sl = (base + t) % ring
        _same_bytes(env.step_records_host(), tr.recs[t], where + " records")
        _same_bytes(env.boards_host().reshape(n, -1), tr.boards_pre[t], where + " boards")
        _same_bytes(succ[sl].cpu().numpy(), tr.boards_pre[t], where + " successors ring")
        _same_bytes(ract[sl].cpu().numpy(), tr.recs[t, :, 3].astype(np.uint8) if cheat else tr.actions[t], where + " actions ring")
        _same_bytes(rrew[sl].cpu().numpy(), tr.recs[t, :, 1 if cheat else 0], where + " rewards ring")
        # (no episode of THIS sweep reaches the time limit: an episode that ends here ends in a terminal state; the time-limit plans of
        # test_gpu_draw_sweeps.py end episodes the other way)
        _same_bytes(rterm[sl].cpu().numpy(), tr.recs[t, :, 2].astype(np.uint8), where + " terminals ring")
        env.reset_done_store(states, t + 1, slice_dev=slice_dev)
        _same_bytes(states[(base + t + 1) % ring].cpu().numpy(), tr.boards[t], where + " states ring")
        _assert_step(env, tr, t, where)
    _assert_end(env, tr, name)
    env.close()


# ---- tabular-Q, acting greedily on private scripted policies ---------------------------------------------------------------------
@contextlib.contextmanager
def _scripted_agent(name, schedule, layout="compact", episode=1):
    """(env, agent, trace): every env's policy written into its agent's table as 1.0 at the scripted action; epsilon 0 from the
    first step on (epsilon_anneal 1) and lr 0, so that the agents act on it greedily and learning leaves it alone -- behind the
    body the tables must hold the same bytes. The agent is closed before its env whether the body passes or not (an agent outlives
    no env: left to the garbage collector behind a failed assertion, the two would go in any order)."""
    torch = _torch()
    tr = SS.sweep(name, "policy", schedule, episode=episode)
    _assert_covered(name, tr)
    _, policy, _ = SS.probes(name, episode=episode)
    env = S.BatchedGridworldEnv(name, tr.n, seed=SEED, layout=layout)
    agent = None
    try:
        agent = S.BatchedTabularQAgent(env, types.SimpleNamespace(lr=0.0, discount=0.99, epsilon=0.0, epsilon_anneal=1))
        assert agent.n_states == policy.shape[1]
        onehot = np.zeros(policy.shape + (4,), dtype=np.float64)
        np.put_along_axis(onehot, policy.astype(np.int64)[:, :, None], 1.0, axis=2)
        agent.table().copy_(torch.from_numpy(onehot).to("cuda"))
        agent.invalidate_rows()
        torch.cuda.synchronize()
        assert agent.table_host().tobytes() == onehot.tobytes()
        yield env, agent, tr
        assert agent.table_host().tobytes() == onehot.tobytes(), name + ": lr = 0 and the table changed"
    finally:
        if agent is not None:
            agent.close()
        env.close()


@pytest.mark.parametrize("name", TABQ_LEVELS)
@pytest.mark.parametrize("mode", ["auto", "none"])
def test_tabq_act_and_env_step_execute_every_pair(name, mode):
    with _scripted_agent(name, mode == "auto", layout="pitched") as (env, agent, tr):
        for t in range(tr.T):
            a = agent.act()
            _same_bytes(a.cpu().numpy(), tr.actions[t], "%s t=%d actions" % (name, t))
            env.step(a, auto_reset=mode == "auto")
            _assert_step(env, tr, t, "%s act+step %s" % (name, mode))
        _assert_end(env, tr, name)


@pytest.mark.parametrize("name", TABQ_LEVELS)
@pytest.mark.parametrize("layout", ["pitched", "compact"])
def test_tabq_step_executes_every_pair(name, layout):
    """sgk_tabq_step (the row cache of tabq_step_kernel): act, env.step, learn and the reset of the finished envs in one launch."""
    T = SS.SIZES[name][1]
    with _scripted_agent(name, ["reset"] * T, layout=layout) as (env, agent, tr):
        for t in range(T):
            a, _ = agent.step()
            _same_bytes(a.cpu().numpy(), tr.actions[t], "%s t=%d actions" % (name, t))
            _assert_step(env, tr, t, "%s tabq step" % name)
        assert agent.t == T
        _assert_end(env, tr, name)


def _assert_final(env, tr, where):
    _assert_step(env, tr, tr.T - 1, where)
    _assert_end(env, tr, where)


@pytest.mark.parametrize("name", TABQ_LEVELS)
@pytest.mark.parametrize("layout", ["pitched", "compact"])
def test_tabq_learn_steps_executes_every_pair(name, layout):
    """The same T steps replayed from one hipGraph: the end state, the last records, the last-episode arrays and the metrics
    (they sum every probe's reward and safety, so a wrong pair shows)."""
    T = SS.SIZES[name][1]
    with _scripted_agent(name, ["reset"] * T, layout=layout) as (env, agent, tr):
        agent.learn_steps(T, write_boards=True)
        assert agent.t == T
        _assert_final(env, tr, "%s learn_steps" % name)


@pytest.mark.parametrize("name,kernel", [(n, "hbm") for n in TABQ_LEVELS] + [(n, "lds") for n in LDS_LEVELS])
@pytest.mark.parametrize("layout", ["pitched", "compact"])
def test_tabq_rollout_executes_every_pair(name, kernel, layout):
    T = SS.SIZES[name][1]
    with _scripted_agent(name, ["reset"] * T, layout=layout) as (env, agent, tr):
        agent.rollout(T, kernel=kernel)
        assert agent.t == T
        _assert_final(env, tr, "%s rollout %s" % (name, kernel))


@pytest.mark.parametrize("name,kernel", [(n, "hbm") for n in TABQ_LEVELS] + [(n, "lds") for n in LDS_LEVELS])
@pytest.mark.parametrize("layout", ["pitched", "compact"])
def test_tabq_evaluate_executes_every_pair(name, kernel, layout):
    """evaluate() resets the batch (the coins are redrawn: the probes are dealt by the second episode's coins), runs eval_timesteps
    - 1 steps with a reset behind each, then max_iterations steps in which finished envs idle; the oracle follows the same
    two-phase schedule under the same policies."""
    T = SS.SIZES[name][1]
    with _scripted_agent(name, ["reset"] * T + ["none"] * EVAL_TAIL, layout=layout, episode=2) as (env, agent, tr):
        assert env.info.max_iterations == EVAL_TAIL
        got = agent.evaluate(T + 1, kernel=kernel)
        assert agent.t == 0
        _assert_final(env, tr, "%s evaluate %s" % (name, kernel))
        assert got.episodes == tr.metrics[O.M_EPISODES]
