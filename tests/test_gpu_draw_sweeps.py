"""The planned sweeps of WhiskyGold and FriendFoe on the device (tests/whisky_sweep.py, tests/foe_sweep.py): the scriptable device
paths play the committed plans and are held to the oracle's records of them after EVERY step -- step records and dense boards as
bytes, every state field that episode_state_host() / last_episode_host() expose, on FriendFoe env.bandit_policy() as uint64 against
the record's six estimates per env, the metrics at the end -- with the assertions of test_gpu_state_sweep.py. The records execute
every required event (asserted on them here, before a device is touched), the device equals the records step by step, so the events
reach the device: env_actual_action's replacement draws keyed by reset count and frame, the second arrival on the empty whisky cell,
begin_episode_with's first maximum / first minimum over estimates that have moved, both holders of the estimates -- AuxMem (HBM at
every step: env.step, the step server, step_store, tabq act / step / learn_steps) and AuxRegs (loaded once per launch, bit blends,
stored if dirty: tabq rollout and evaluate, kernel "hbm") -- and the hand-over between the two.

Paths: env.step under both layouts, auto-reset and idle (reset_done() behind every 5th step), and in the grid-stride step kernel (the
script dealt over 65 637 envs); sgk_step_host through the step server on FriendFoe; step_store + reset_done_store into rings of 5 that
wrap, with and without cheat (WhiskyGold: the ring holds the EXECUTED action); the tabular-Q agents on the policy phases (epsilon 0,
lr 0, the tables rewritten and invalidate_rows() between the phases): act + env.step, step, learn_steps, rollout hbm (one launch per
phase: the estimates cross launches, the quiet ones included), evaluate hbm behind a training phase, and one handle that alternates
rollout phases with per-step phases; the time-limit plans through env.step, step_store and rollout hbm.

Not covered: the step server on WhiskyGold. sgk_rollout_random*, sgk_policy_rollout* and sgk_convq_rollout* choose their own actions
and take no script: test_gpu_rollout_sweep.py plays these plans to a mid-plan step at which an env is drunk / has estimates that moved
and holds the rollouts' launches from there to the oracle, without an event requirement of its own."""
import contextlib
import types

import numpy as np
import pytest

import foe_sweep as FS
import safe_grid_agents_amd as S
import state_sweep as SS
import whisky_sweep as WS
from oracle import oracle as O
from safe_grid_agents_amd import _lib
from test_gpu_state_sweep import _assert_state, _assert_step, _same_bytes, _torch

pytestmark = pytest.mark.gpu

MODS = pytest.mark.parametrize("mod", [WS, FS], ids=["WhiskyGold", "FriendFoe"])
LAYOUTS = pytest.mark.parametrize("layout", ["pitched", "compact"])
GRID_N = 65536 + 64 + 37  # above STEP_SMALL_MAX_ENVS = 65 536 (sgk_step.hip): whole 64-env tiles, a tile of 37, a grid that strides
EVAL_TAIL = 100  # env.info.max_iterations: the steps evaluate() runs without reset


def _covered(mod, form, schedule="auto"):
    """The condition the sweeps exist for, on the record the device is about to be held to."""
    tr = mod.record(form, schedule)
    if mod is WS:
        got = WS.events_of(tr, WS.SEED)
        missing = [ev for ev in WS.required() if not got.get(ev)]
    else:
        got, depth = FS.events_of(tr)
        missing = [ev for ev in FS.required(form) if not got.get(ev)]
        assert depth == FS.DEPTH[form]
    assert not missing, missing
    assert tr.n == mod.N and tr.n % 64 != 0
    return tr


def _timeout_covered(mod, form, schedule):
    tr = mod.timeout_record(form, schedule)
    got = WS.events_of(tr, WS.SEED) if mod is WS else FS.events_of(tr)[0]
    missing = [ev for ev in mod.required_timeout() if not got.get(ev)]
    assert not missing, missing
    return tr


def _assert_aux(env, tr, t, where, lo=0, hi=None):
    """FriendFoe's six estimates of every env, as bit patterns, against the record behind step t (t = -1: before the first)."""
    if tr.name != FS.NAME:
        return
    hi = lo + env.n_envs if hi is None else hi
    got = env.bandit_policy().reshape(env.n_envs, 6).view(np.uint64)
    want = (tr.aux0 if t < 0 else tr.aux[t])[lo:hi]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s t=%d estimates differ at envs %s: %s / %s" % (where, t, bad[:5], got[bad[:3]].view(np.float64),
                                                                             want[bad[:3]].view(np.float64))


def _assert_all(env, tr, t, where, lo=0):
    _assert_step(env, tr, t, where, lo)
    _assert_aux(env, tr, t, where, lo)


def _assert_metrics(env, want, where):
    assert env.metrics().tolist() == want.tolist(), where


# ---- env.step(actions) ---------------------------------------------------------------------------------------------------------
def _run_env_step(mod, tr, layout, where):
    torch = _torch()
    env = S.BatchedGridworldEnv(mod.NAME, tr.n, seed=mod.SEED, layout=layout)
    try:
        _assert_state(env, tr.boards0, tr.fields0, "after create")
        _assert_aux(env, tr, -1, where)
        for t in range(tr.T):
            env.step(torch.as_tensor(tr.actions[t], device="cuda"), auto_reset=tr.schedule[t] == "auto")
            if tr.schedule[t] == "reset":  # without auto-reset finished envs idle until the caller resets them
                env.reset_done()
            _assert_all(env, tr, t, where)
        _assert_metrics(env, tr.metrics, where)
    finally:
        env.close()


@MODS
@LAYOUTS
@pytest.mark.parametrize("mode", ["auto", "idle"])
def test_env_step_executes_every_event(mod, layout, mode):
    """idle: the record of the same script with reset_done() behind every 5th step (explained by the draws like the other; the events
    are required of the auto-reset record)."""
    tr = _covered(mod, "actions") if mode == "auto" else mod.record("actions", "idle")
    _run_env_step(mod, tr, layout, "%s %s %s" % (mod.NAME, layout, mode))


@MODS
@LAYOUTS
def test_env_step_executes_every_event_in_the_grid_stride_kernel(mod, layout):
    """step_kernel<SMALL = false>: the script dealt again and again over 65 637 envs created at env index 0; the first N are the
    planned ones (test_draw_sweeps_cpu.py holds them to the record that executes every event)."""
    small = _covered(mod, "actions")
    tr = mod.record("actions", copies=-(-GRID_N // mod.N), n=GRID_N)
    assert tr.n == GRID_N and (tr.recs[:, :mod.N] == small.recs).all() and (tr.aux[:, :mod.N] == small.aux).all()
    _run_env_step(mod, tr, layout, "%s %s grid-stride" % (mod.NAME, layout))


# ---- sgk_step_host / the step server ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "idle"])
def test_step_server_executes_every_event_on_friend_foe(mode):
    """Host-visible handles of at most 64 envs, each created at the global index of its first env (the draws are keyed by it): every
    sgk_step_host is served by the resident wave through the mailbox; the estimates are compared behind every call."""
    _torch()
    tr = _covered(FS, "actions") if mode == "auto" else FS.record("actions", "idle")
    sums = np.zeros(8, dtype=np.int64)
    maxima = np.full(4, np.iinfo(np.int64).min, dtype=np.int64)
    for lo in range(0, tr.n, 64):
        cnt = min(64, tr.n - lo)
        env = S.BatchedGridworldEnv(FS.NAME, cnt, seed=FS.SEED, env_index_base=lo, host_visible=True)
        try:
            rec = np.zeros((cnt, 4), dtype=np.int8)
            boards = np.zeros((cnt, env.n_cells), dtype=np.int8)
            ret = np.zeros(cnt, dtype=np.int32)
            for t in range(tr.T):
                acts = np.ascontiguousarray(tr.actions[t, lo:lo + cnt])
                _lib.check(env.lib.sgk_step_host(env.handle, acts.ctypes.data, _lib.F_AUTO_RESET if mode == "auto" else 0, rec.ctypes.data,
                                                 boards.ctypes.data, ret.ctypes.data))
                where = "%s envs %d.. t=%d" % (mode, lo, t)
                _same_bytes(rec, tr.recs[t, lo:lo + cnt], where + " records")
                if tr.schedule[t] == "reset":
                    _same_bytes(boards, tr.boards_pre[t, lo:lo + cnt], where + " boards")
                    env.reset_done()
                    _assert_step(env, tr, t, where, lo)
                else:
                    _same_bytes(boards, tr.boards[t, lo:lo + cnt], where + " boards")
                    assert (ret == tr.fields["episode_return"][t, lo:lo + cnt]).all(), where
                _assert_aux(env, tr, t, where, lo)
            _assert_all(env, tr, tr.T - 1, "%s envs %d.. at the end" % (mode, lo), lo)
            m = env.metrics()
            sums += m[:8]
            maxima = np.maximum(maxima, m[8:12])
        finally:
            env.close()
    assert sums.tolist() == tr.metrics[:8].tolist()
    assert maxima.tolist() == tr.metrics[8:12].tolist()


# ---- env.step_store + sgk_reset_done_store ----------------------------------------------------------------------------------------
def _run_step_store(mod, tr, layout, cheat, slice_on_device):
    torch = _torch()
    n, ring = tr.n, 5
    env = S.BatchedGridworldEnv(mod.NAME, n, seed=mod.SEED, layout=layout)
    try:
        succ = torch.full((ring, n, env.n_cells), -7, dtype=torch.int8, device="cuda")
        states = torch.full((ring, n, env.n_cells), -7, dtype=torch.int8, device="cuda")
        ract = torch.full((ring, n), 99, dtype=torch.uint8, device="cuda")
        rrew = torch.full((ring, n), -7, dtype=torch.int8, device="cuda")
        rterm = torch.full((ring, n), 9, dtype=torch.uint8, device="cuda")
        base = 3 if slice_on_device else 0
        slice_dev = torch.tensor([base], dtype=torch.int64, device="cuda") if slice_on_device else None
        for t in range(tr.T):
            where = "%s %s t=%d" % (mod.NAME, layout, t)
            env.step_store(torch.as_tensor(tr.actions[t], device="cuda"), t, (succ, ract, rrew, rterm), cheat=cheat, slice_dev=slice_dev)
            sl = (base + t) % ring
            _same_bytes(env.step_records_host(), tr.recs[t], where + " records")
            _same_bytes(env.boards_host().reshape(n, -1), tr.boards_pre[t], where + " boards")
            _same_bytes(succ[sl].cpu().numpy(), tr.boards_pre[t], where + " successors ring")
            _same_bytes(ract[sl].cpu().numpy(), tr.recs[t, :, 3].astype(np.uint8) if cheat else tr.actions[t], where + " actions ring")
            _same_bytes(rrew[sl].cpu().numpy(), tr.recs[t, :, 1 if cheat else 0], where + " rewards ring")
            # the terminal flag is the record's done bit, at a time limit too (the time-limit plans below end episodes that way)
            _same_bytes(rterm[sl].cpu().numpy(), tr.recs[t, :, 2].astype(np.uint8), where + " terminals ring")
            env.reset_done_store(states, t + 1, slice_dev=slice_dev)
            _same_bytes(states[(base + t + 1) % ring].cpu().numpy(), tr.boards[t], where + " states ring")
            _assert_all(env, tr, t, where)
        _assert_metrics(env, tr.metrics, mod.NAME)
    finally:
        env.close()


@MODS
@LAYOUTS
@pytest.mark.parametrize("cheat", [False, True])
@pytest.mark.parametrize("slice_on_device", [False, True])
def test_step_store_and_reset_done_store_execute_every_event(mod, layout, cheat, slice_on_device):
    """Replay rings of 5 slices, fewer than T, so they wrap: every slice is compared before it is overwritten, with the slice named
    by the host and by the device scalar. Under cheat the ring holds the executed action and the hidden reward: on WhiskyGold the
    replaced actions and the drink's missing +5."""
    tr = _covered(mod, "actions", "reset")
    if mod is WS:
        assert (tr.recs[:, :, 3] != tr.actions).any() and (tr.recs[:, :, 0] != tr.recs[:, :, 1]).any()
    _run_step_store(mod, tr, layout, cheat, slice_on_device)


# ---- tabular-Q on the policy phases -----------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _phased_agent(mod, tr, policies, layout):
    """(env, agent, load): load(p) writes phase p's policies into the agents' tables as 1.0 at the scripted action (and checks that
    the phase before left the bytes alone); epsilon 0 from the first step on (epsilon_anneal 1) and lr 0, so that the agents act on
    them greedily and learning leaves them alone."""
    torch = _torch()
    env = S.BatchedGridworldEnv(mod.NAME, tr.n, seed=mod.SEED, layout=layout)
    agent = None
    held = []
    try:
        agent = S.BatchedTabularQAgent(env, types.SimpleNamespace(lr=0.0, discount=0.99, epsilon=0.0, epsilon_anneal=1))

        def unchanged():
            if held:
                assert agent.table_host().tobytes() == held[0].tobytes(), mod.NAME + ": lr = 0 and the table changed"

        def load(p):
            unchanged()
            policy = policies[p]
            assert agent.n_states == policy.shape[1]
            onehot = np.zeros(policy.shape + (4,), dtype=np.float64)
            np.put_along_axis(onehot, policy.astype(np.int64)[:, :, None], 1.0, axis=2)
            agent.table().copy_(torch.from_numpy(onehot).to("cuda"))
            agent.invalidate_rows()
            torch.cuda.synchronize()
            held[:] = [onehot]
            unchanged()

        yield env, agent, load
        unchanged()
    finally:
        if agent is not None:
            agent.close()
        env.close()


def _phases(mod, tr):
    """[(first step, last step, policy)] of the record's phases."""
    pols = [pol for _, pol in mod.plan_policies()]
    first = [0] + [e + 1 for e in tr.phase_end[:-1]]
    return list(zip(first, tr.phase_end, pols)), pols


@MODS
def test_tabq_act_and_env_step_execute_every_event(mod):
    tr = _covered(mod, "policy")
    phases, pols = _phases(mod, tr)
    with _phased_agent(mod, tr, pols, "pitched") as (env, agent, load):
        for p, (t0, t1, _) in enumerate(phases):
            load(p)
            for t in range(t0, t1 + 1):
                a = agent.act()
                _same_bytes(a.cpu().numpy(), tr.actions[t], "%s t=%d actions" % (mod.NAME, t))
                env.step(a, auto_reset=True)
                _assert_all(env, tr, t, "%s act+step" % mod.NAME)
        _assert_metrics(env, tr.metrics, mod.NAME)


@MODS
@LAYOUTS
def test_tabq_step_executes_every_event(mod, layout):
    """sgk_tabq_step: act, env.step, learn and the reset of the finished envs in one launch."""
    tr = _covered(mod, "policy", "reset")
    phases, pols = _phases(mod, tr)
    with _phased_agent(mod, tr, pols, layout) as (env, agent, load):
        for p, (t0, t1, _) in enumerate(phases):
            load(p)
            for t in range(t0, t1 + 1):
                a, _ = agent.step()
                _same_bytes(a.cpu().numpy(), tr.actions[t], "%s t=%d actions" % (mod.NAME, t))
                _assert_all(env, tr, t, "%s tabq step" % mod.NAME)
        assert agent.t == tr.T
        _assert_metrics(env, tr.metrics, mod.NAME)


@MODS
@LAYOUTS
@pytest.mark.parametrize("call", ["learn_steps", "rollout_hbm"])
def test_tabq_fused_calls_execute_every_event(mod, layout, call):
    """One hipGraph of per-step launches (learn_steps: the estimates in HBM at every step) or ONE launch (rollout, kernel "hbm": the
    estimates in registers, stored if an episode of the launch opened a box) per phase: the state, the last records, the estimates
    and the metrics are compared behind every launch -- behind the quiet ones, in which some envs with moved estimates open nothing,
    too."""
    tr = _covered(mod, "policy", "reset")
    phases, pols = _phases(mod, tr)
    with _phased_agent(mod, tr, pols, layout) as (env, agent, load):
        for p, (t0, t1, _) in enumerate(phases):
            load(p)
            if call == "learn_steps":
                agent.learn_steps(t1 - t0 + 1, write_boards=True)
            else:
                agent.rollout(t1 - t0 + 1, kernel="hbm")
            assert agent.t == t1 + 1
            _assert_all(env, tr, t1, "%s %s phase %d" % (mod.NAME, call, p))
            _assert_metrics(env, tr.metrics_at[p], "%s %s phase %d" % (mod.NAME, call, p))


@MODS
@LAYOUTS
def test_tabq_evaluate_behind_a_training_phase(mod, layout):
    """rollout (phase 0's policies), then evaluate() on phase 1's: it resets the whole batch and the metrics, runs eval_timesteps - 1
    steps with a reset behind each and max_iterations steps in which finished envs idle; the oracle follows the same schedule. On
    FriendFoe the estimates the training launch stored are what the evaluation's first levels come from, and the evaluation moves
    them on."""
    (s0, pol0), (s1, pol1) = mod.plan_policies()[:2]
    tr = SS.trace_phases(mod.NAME, mod.SEED, mod.N, [(pol0, ["reset"] * s0), (None, "reset_all"),
                                                     (pol1, ["reset"] * s1 + ["none"] * EVAL_TAIL)])
    if mod is FS:
        FS.explain(tr, FS.SEED)
        assert (tr.aux[s0 - 1] != tr.aux0).any() and (tr.aux[-1] != tr.aux[s0 - 1]).any()
    with _phased_agent(mod, tr, [pol0, pol1], layout) as (env, agent, load):
        assert env.info.max_iterations == EVAL_TAIL
        load(0)
        agent.rollout(s0, kernel="hbm")
        _assert_all(env, tr, s0 - 1, "%s training phase" % mod.NAME)
        load(1)
        got = agent.evaluate(s1 + 1, kernel="hbm")
        assert agent.t == s0
        _assert_all(env, tr, tr.T - 1, "%s evaluate" % mod.NAME)
        _assert_metrics(env, tr.metrics, "%s evaluate" % mod.NAME)
        assert got.episodes == tr.metrics[O.M_EPISODES]


@MODS
@LAYOUTS
def test_one_handle_alternates_fused_and_per_step_phases(mod, layout):
    """Mixed holders: rollout phases (AuxRegs: load, blend, store if dirty) alternate with per-step phases (act + env.step: AuxMem) on
    the same envs, compared at every switch and behind every step of the per-step phases."""
    tr = _covered(mod, "policy", "reset")
    phases, pols = _phases(mod, tr)
    with _phased_agent(mod, tr, pols, layout) as (env, agent, load):
        for p, (t0, t1, _) in enumerate(phases):
            load(p)
            if p % 2 == 0:
                agent.rollout(t1 - t0 + 1, kernel="hbm")
            else:
                for t in range(t0, t1 + 1):
                    a = agent.act()
                    _same_bytes(a.cpu().numpy(), tr.actions[t], "%s t=%d actions" % (mod.NAME, t))
                    env.step(a, auto_reset=True)
                    _assert_all(env, tr, t, "%s mixed, per step" % mod.NAME)
            _assert_all(env, tr, t1, "%s mixed, behind phase %d" % (mod.NAME, p))


# ---- the time-limit plans -------------------------------------------------------------------------------------------------------
@MODS
def test_the_time_limit_through_env_step(mod):
    tr = _timeout_covered(mod, "actions", "auto")
    _run_env_step(mod, tr, "compact", "%s time limit" % mod.NAME)


@MODS
def test_the_time_limit_through_step_store(mod):
    """The terminal ring at a time-limit end holds 1, the record's done bit (include/sgk.h does not tell the two ends apart: the
    oracle's behaviour is what is pinned)."""
    tr = _timeout_covered(mod, "actions", "reset")
    at = (tr.pre["frame"] == mod.MAX_ITERATIONS) & (tr.pre["game_over"] == 1)
    assert at.any() and (tr.recs[:, :, 2][at] == 1).all()
    _run_step_store(mod, tr, "pitched", False, True)


@MODS
@LAYOUTS
def test_the_time_limit_through_tabq_rollout(mod, layout):
    """One policy, one launch of 104 steps: the fused kernel's own frame counter ends the episodes; on FriendFoe a launch whose only
    episode end is a time limit stores nothing, and the next episode's type is the one of reset count + 1."""
    tr = _timeout_covered(mod, "policy", "reset")
    _, policy = mod.timeout_plan()
    with _phased_agent(mod, tr, [policy], layout) as (env, agent, load):
        load(0)
        agent.rollout(tr.T, kernel="hbm")
        _assert_all(env, tr, tr.T - 1, "%s time limit, rollout" % mod.NAME)
        _assert_metrics(env, tr.metrics, mod.NAME)
