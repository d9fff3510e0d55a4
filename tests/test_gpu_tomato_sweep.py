"""The planned sweep of TomatoWatering on the device (tests/tomato_sweep.py): the scriptable device paths play the committed plan
and are held to the oracle's record of it after EVERY step -- step records and dense boards as bytes, every state field that
episode_state_host() / last_episode_host() expose, the metrics at the end, with the assertions of test_gpu_state_sweep.py. (The
state word's `ext` bits -- tomatoes 8..12 -- are not among those fields: the device's are held through the dense boards, which show
every tomato but the one under the agent and none on the bucket, and through the hidden reward and return, which count all 13; the
host build of the same transition is held to `ext` itself in test_tomato_sweep_cpu.py.) The record
executes every required event (asserted on it here, before a device is touched: all 116 (agent cell, action) pairs, the four drying
events of each of the 13 tomatoes, two Philox blocks in one step, both halves of the mask in one step, the bucket's three), the
device equals the record step by step, so the events reach the device: transition<TOMATO> under env_actual_action's draws -- the
arrival on a tomato in the very step its own draw dries it included --, the board writers with every mask bit on and off, the state
word's `box` and `ext` halves.

Paths: env.step under both layouts, with auto-reset and idle (reset_done() behind every 5th step); the grid-stride instantiation
of step_kernel (the plan dealt again and again over 65 604 envs: the first 231 are the planned ones, the others dry by draws of
their own under the same scripts); step_store into a ring of 5 slices that wraps. The record is one episode of T <= 99 steps, so
nothing is reset in it and reset_done_store is not among the paths."""
import numpy as np
import pytest

import safe_grid_agents_amd as S
import tomato_sweep as TS
from test_gpu_state_sweep import _assert_end, _assert_state, _assert_step, _same_bytes, _torch

pytestmark = pytest.mark.gpu

GRID_COPIES = 284  # 284 * 231 = 65 604 envs = 1 025 whole tiles + 4 lanes, above STEP_SMALL_MAX_ENVS = 65 536 (sgk_step.hip)


def _covered(copies=1):
    """The condition the sweep exists for, on the record the device is about to be held to."""
    tr, rec = TS.record(copies=copies)
    got = TS.events_of(rec)
    missing = [ev for ev in TS.required() if not got.get(ev)]
    assert not missing, missing
    assert tr.n == copies * TS.N and tr.n % 64 != 0 and (rec.actions == tr.actions[:, :TS.N]).all()
    return tr


def _run_env_step(layout, mode, copies=1):
    torch = _torch()
    tr = _covered(copies)
    env = S.BatchedGridworldEnv(TS.NAME, tr.n, seed=TS.SEED, layout=layout)
    _assert_state(env, tr.boards0, tr.fields0, "after create")
    for t in range(tr.T):
        env.step(torch.as_tensor(tr.actions[t], device="cuda"), auto_reset=mode == "auto")
        if mode == "idle" and t % 5 == 4:  # nothing is over inside the episode: reset_done() must leave every env alone
            env.reset_done()
        _assert_step(env, tr, t, "%s %s" % (layout, mode))
    _assert_end(env, tr, TS.NAME)
    env.close()


@pytest.mark.parametrize("layout", ["pitched", "compact"])
@pytest.mark.parametrize("mode", ["auto", "idle"])
def test_env_step_executes_every_event(layout, mode):
    _run_env_step(layout, mode)


@pytest.mark.parametrize("layout", ["pitched", "compact"])
def test_env_step_executes_every_event_in_the_grid_stride_kernel(layout):
    """step_kernel<SMALL = false>: whole 64-env tiles, a tile of 4, a grid that strides."""
    assert GRID_COPIES * TS.N > 65536
    _run_env_step(layout, "auto", copies=GRID_COPIES)


@pytest.mark.parametrize("layout", ["pitched", "compact"])
@pytest.mark.parametrize("cheat", [False, True])
@pytest.mark.parametrize("slice_on_device", [False, True])
def test_step_store_executes_every_event(layout, cheat, slice_on_device):
    """A replay ring of 5 slices, fewer than T, so it wraps: every slice is compared before it is overwritten -- successor boards,
    action, reward (the hidden one under cheat: on the bucket they differ) and terminal flag --, with the slice named by the host
    and by the device scalar."""
    torch = _torch()
    tr = _covered()
    n, ring = tr.n, 5
    env = S.BatchedGridworldEnv(TS.NAME, n, seed=TS.SEED, layout=layout)
    succ = torch.full((ring, n, env.n_cells), -7, dtype=torch.int8, device="cuda")
    ract = torch.full((ring, n), 99, dtype=torch.uint8, device="cuda")
    rrew = torch.full((ring, n), -7, dtype=torch.int8, device="cuda")
    rterm = torch.full((ring, n), 9, dtype=torch.uint8, device="cuda")
    base = 3 if slice_on_device else 0
    slice_dev = torch.tensor([base], dtype=torch.int64, device="cuda") if slice_on_device else None
    for t in range(tr.T):
        where = "%s t=%d" % (layout, t)
        env.step_store(torch.as_tensor(tr.actions[t], device="cuda"), t, (succ, ract, rrew, rterm), cheat=cheat, slice_dev=slice_dev)
        sl = (base + t) % ring
        _same_bytes(succ[sl].cpu().numpy(), tr.boards[t], where + " successors ring")
        _same_bytes(ract[sl].cpu().numpy(), tr.recs[t, :, 3].astype(np.uint8) if cheat else tr.actions[t], where + " actions ring")
        _same_bytes(rrew[sl].cpu().numpy(), tr.recs[t, :, 1 if cheat else 0], where + " rewards ring")
        _same_bytes(rterm[sl].cpu().numpy(), tr.recs[t, :, 2].astype(np.uint8), where + " terminals ring")
        _assert_step(env, tr, t, where)
    assert (tr.recs[:, :, 0] != tr.recs[:, :, 1]).any()  # the two reward channels differ somewhere: cheat picked the right one
    _assert_end(env, tr, TS.NAME)
    env.close()
