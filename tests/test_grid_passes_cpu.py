"""What the plans of tests/grid_passes.py must provide for tests/test_gpu_grid_passes.py to mean something, asserted on the oracle
alone (no GPU): with 64 workgroups per launch the sizes put tiles into later passes and a partial tile into the last one (derived and
asserted when grid_passes is imported), and in those tiles episodes end, every action occurs, the replay rings' terminal flags take
both values and finished envs lie on both sides of the scan's slab boundary. A plan that misses one of these is replaced, not
skipped: a GPU case whose later-pass tiles all did the same thing would pass with a kernel that mixes them up."""
import numpy as np
import pytest

import grid_passes as GP
from oracle import oracle as O


def _covers(mask, region, what):
    assert (mask & region).any(), what


@pytest.mark.parametrize("name", GP.ENVS)
def test_the_step_plan_ends_episodes_and_uses_every_action_in_later_pass_tiles(name):
    later, part = GP.later_pass(GP.N_STEP), GP.partial_tile(GP.N_STEP)
    assert later.sum() == GP.N_STEP - 16384 and part.sum() == 37 and (later & part).sum() == 37
    _, m, t, facts = GP.run_step_plan(name)
    assert t == sum(k for op, k, _, _ in GP.STEP_PLAN) == 112 and len(facts) == len(GP.STEP_PLAN)
    for kind in ("given", "graph"):  # the RANDOM = false and RANDOM = true instantiations of step_kernel
        ended = np.zeros(GP.N_STEP, dtype=bool)
        for op, _, e in facts:
            if op == kind:
                ended |= e
        _covers(ended, later, (name, kind, "no episode ends in a later-pass tile"))
        _covers(ended, part, (name, kind, "no episode ends in the partial last tile"))
        assert not ended.all(), (name, kind)  # the masked reset keeps some envs out of step: a tile's envs differ
    for op, acts, _ in facts:
        if op in ("given", "repeat"):
            assert set(np.unique(acts[later])) == {0, 1, 2, 3}, (name, op)
            assert (acts[later][:16384] != acts[:16384]).any(), (name, op)  # a later tile's actions are not the first tile's
    # every wave's last pass sees episodes end in some given-action step: a wave that flushed its metrics early would lose them
    assert m[O.M_EPISODES] > 0


@pytest.mark.parametrize("n", GP.STREAM_SIZES)
@pytest.mark.parametrize("name", GP.ENVS)
def test_every_rollout_window_ends_episodes_in_later_pass_tiles(name, n):
    later, part = GP.later_pass(n), GP.partial_tile(n)
    assert later.sum() == n - 16384 and part.sum() == n % 64
    orc = O.EnvBatch(name, n, seed=GP.STREAM_SEED)
    t = GP.stream_prephase(None, orc)
    assert t == 100
    _, f = orc.export(boards=False)
    # no rollout starts where every tile's state words are alike: the first pass's tiles differ from the second pass's
    k = later.sum()
    assert (f["frame"][later] != f["frame"][:k]).any() or (f["agent_cell"][later] != f["agent_cell"][:k]).any(), name
    for w, steps in GP.stream_windows(orc, t):
        ended = np.zeros(n, dtype=bool)
        actions = set()
        for _, rec in steps:
            ended |= rec[:, 2] != 0
            actions |= set(np.unique(rec[later, 3]).tolist())
        _covers(ended, later, (name, n, w, "no episode ends in a later-pass tile"))
        if n % 64:
            _covers(ended, part, (name, n, w, "no episode ends in the partial last tile"))
        assert not ended[later].all(), (name, n, w)
        assert actions >= {0, 1, 2, 3}, (name, n, w, actions)


@pytest.mark.parametrize("name", ["SideEffectsSokoban-v0", "WhiskyGold-v0"])
def test_the_store_plan_writes_both_terminal_values_in_later_pass_tiles(name):
    later, part = GP.later_pass(GP.N_STEP), GP.partial_tile(GP.N_STEP)
    orc = O.EnvBatch(name, GP.N_STEP, seed=GP.STORE_SEED)
    seen = []
    assert GP.store_prephase(None, orc) == 98
    for i in range(GP.STORE_T):
        rec = orc.rollout(1, seed=GP.STORE_SEED, actions=GP.store_actions(i)[None], auto_reset=False)
        seen.append(rec[:, 2].copy())
        GP.oracle_reset(orc, np.flatnonzero(orc.export(boards=False)[1]["game_over"]))
    assert len(seen) == GP.STORE_T
    done = np.stack(seen)
    for region, what in ((later, "later-pass tiles"), (part, "the partial tile")):
        assert (done[:, region] == 1).any() and (done[:, region] == 0).any(), (name, what)
    assert any((d[later] == 1).any() and (d[later] == 0).any() for d in seen), name  # both values within one launch


@pytest.mark.parametrize("name", sorted(GP.SCAN_PLANS))
def test_the_scan_plan_leaves_finished_envs_in_both_slabs(name):
    orc = GP.run_scan_plan(name)
    done = orc.export(boards=False)[1]["game_over"] != 0
    first_slab = np.arange(GP.N_SCAN) < GP.SCAN_SLAB * GP.WG
    assert (~first_slab).sum() == 256 + 37
    for slab, what in ((first_slab, "first"), (~first_slab, "second")):
        assert done[slab].any() and not done[slab].all(), (name, what)
    # a carry that is dropped shows: the second slab's envs would be written from offset 0 on
    assert done[first_slab].sum() > done[~first_slab].sum() > 0
