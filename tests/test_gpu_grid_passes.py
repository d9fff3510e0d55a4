"""The later passes of the large-batch kernels, at the smallest sizes at which they exist (tests/grid_passes.py), bit for bit
against the oracle.

Every handle is created with SGK_MAX_GRID = SGK_STREAM_GRID = SGK_ROLLOUT_GRID = 64, and says so (sgk_debug_launch_grids) before
anything else is asserted: a launch then has 256 waves, and a wave that has worked its 64-env tile goes on to the tile 256 further.
With the default caps that happens from ~393 K envs (streamed rollout: 1 M) on, where the suite has a handful of cases. Here:
  (a) the per-step kernels in their large form (above 65 536 envs: 256-lane workgroups, prefetched next tile, metrics flushed on the
      wave's last tile) -- every level, both layouts, a schedule of given-action, graph-replayed, repeated steps and resets;
  (b) the fused replay stores (sgk_step_store, sgk_reset_done_store) and the two-phase sgk_replay_store;
  (c) the rollout kernels -- streamed into the env's own buffers, a slice-major ring, a tile-major ring, outputs once -- with the
      partial tile in the second pass, whole and aligned companions, and the non-temporal store path;
  (d) tabular-Q: the one-launch step, the four-call sequence, the HBM rollout and evaluation;
  (e) the draws, the discounted-returns scan, the members' vote and the finished-env compaction across its scan's slab boundary.
Outputs the test allocates carry a sentinel tail of GP.TAIL elements that must come back untouched.
tests/test_grid_passes_cpu.py asserts, without a GPU, that the plans end episodes, use every action and finish envs in the tiles of
the later passes and in the partial last tile."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import grid_passes as GP
import safe_grid_agents_amd as S
import test_gpu_parity as P
from oracle import oracle as O
from safe_grid_agents_amd import _lib
from test_gpu_ppo import BOUNDARY

pytestmark = pytest.mark.gpu

KNOBS = ("SGK_MAX_GRID", "SGK_STREAM_GRID", "SGK_ROLLOUT_GRID")
LAYOUTS = ["pitched", "compact"]


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def launch_grids(env):
    out = (ctypes.c_int32 * 4)()
    _lib.check(env.lib.sgk_debug_launch_grids(env.handle, out))
    return list(out)


@contextlib.contextmanager
def capped(monkeypatch, name, n, ring_nt=False, **kw):
    """A handle whose three launch caps are 64 workgroups (the knobs are read once, at sgk_create, and removed right behind it)."""
    _torch()
    for k in KNOBS:
        monkeypatch.setenv(k, str(GP.CAP))
    if ring_nt:
        monkeypatch.setenv("SGK_RING_NT", "1")
    env = S.BatchedGridworldEnv(name, n, **kw)
    for k in KNOBS + (("SGK_RING_NT",) if ring_nt else ()):
        monkeypatch.delenv(k)
    try:
        assert launch_grids(env)[1:] == [GP.CAP, GP.CAP, GP.CAP], "the handle ignored a grid knob: every case below would be empty"
        yield env
    finally:
        env.close()


def tailed(shape, dtype, fill):
    """(a contiguous device tensor of `shape`, the GP.TAIL sentinel elements allocated right behind it), all filled with `fill`."""
    torch = _torch()
    numel = int(np.prod(shape))
    flat = torch.full((numel + GP.TAIL,), fill, dtype=dtype, device="cuda")
    return flat[:numel].view(*shape), flat[numel:]


def untouched(tail, fill):
    return tail.numel() == GP.TAIL and bool((tail == fill).all())


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def test_an_uncapped_handle_keeps_the_default_grids():
    """With none of the knobs set: 6 / 16 / 12 workgroups per compute unit, as before the third knob existed."""
    _torch()
    env = S.BatchedGridworldEnv("BoatRace-v0", 64)
    try:
        cus, max_grid, stream_grid, rollout_grid = launch_grids(env)
        assert cus > 0 and [max_grid, stream_grid, rollout_grid] == [6 * cus, 16 * cus, 12 * cus]
    finally:
        env.close()


def test_each_knob_caps_its_own_grid_and_values_below_64_are_ignored(monkeypatch):
    _torch()
    for i, knob in enumerate(KNOBS):
        for value, kept in (("64", 64), ("100", 100), ("63", None), ("x", None)):
            monkeypatch.setenv(knob, value)
            env = S.BatchedGridworldEnv("BoatRace-v0", 64)
            monkeypatch.delenv(knob)
            try:
                g = launch_grids(env)
                want = [6 * g[0], 16 * g[0], 12 * g[0]]
                if kept is not None:
                    want[i] = kept
                assert g[1:] == want, (knob, value)
            finally:
                env.close()


# ---- (a) the per-step kernels at N_STEP ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", GP.ENVS)
def test_per_step_kernels_above_the_small_threshold_take_five_passes(name, layout, monkeypatch):
    """GP.STEP_PLAN at 66 341 envs: waves 0..12 work five tiles, the others four, the 37-env partial tile is wave 12's fifth. After
    every operation the whole batch -- boards (where the operation wrote them), every state field, the step records, the episode
    arrays -- and the metrics vector equal the oracle's; at the end so do obs_f32, render and the host copy of the boards."""
    torch = _torch()
    n = GP.N_STEP
    with capped(monkeypatch, name, n, seed=GP.STEP_SEED, layout=layout) as env:
        def check(i, op, orc, info, t, m, boards_written):
            where = "%s %s op %d %s at t=%d" % (name, layout, i, op, t)
            GP.assert_whole_batch(env, orc, where, boards=boards_written, rec=info["rec"])
            GP.assert_metrics(env, m, t, where)

        orc, m, t, _ = GP.run_step_plan(name, env=env, check=check)
        assert env.lockstep_t == t
        want = orc.export()[0]
        cells = env.n_cells
        obs, obs_tail = tailed((n, cells), torch.float32, -7.0)
        env.obs_f32(out=obs)
        assert (obs.cpu().numpy() == want.astype(np.float32)).all() and untouched(obs_tail, -7.0)
        rgb, rgb_tail = tailed((n, 3, env.H, env.W), torch.uint8, 201)
        env.render(out=rgb)
        want_rgb = np.stack([orc.render_rgb(i) for i in range(n)])
        assert (rgb.cpu().numpy() == want_rgb).all() and untouched(rgb_tail, 201)
        assert (env.boards_host().reshape(n, -1) == want).all()          # through dense_boards_kernel
        assert (env.boards().cpu().numpy().reshape(n, -1) == want).all()  # the zero-copy view


# ---- (b) the fused replay stores at N_STEP -------------------------------------------------------------------------------------------
def _rings(n, cells, slices):
    torch = _torch()
    spec = {"states": ((slices, n, cells), torch.int8, -7), "successors": ((slices, n, cells), torch.int8, -7),
            "actions": ((slices, n), torch.uint8, 99), "rewards": ((slices, n), torch.int8, -7), "terminals": ((slices, n), torch.uint8, 9)}
    rings = {k: tailed(*v) + (v[2],) for k, v in spec.items()}
    return rings


def _assert_slice(rings, key, sl, want, written, where):
    ring, tail, fill = rings[key]
    got = ring.cpu().numpy()
    assert (got[sl] == want).all(), (where, key, sl)
    written[key].add(sl)
    for other in range(got.shape[0]):
        if other not in written[key]:
            assert (got[other] == fill).all(), (where, key, "slice %d was not named" % other)
    assert untouched(tail, fill), (where, key)


@pytest.mark.parametrize("cheat", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["SideEffectsSokoban-v0", "WhiskyGold-v0"])
def test_fused_replay_stores_above_the_small_threshold(name, layout, cheat, monkeypatch):
    """sgk_step_store (step_kernel's STORE instantiation in its large form) and sgk_reset_done_store with the slice named by a device
    scalar so that it wraps, then the two-phase sgk_replay_store: all five rings against what the oracle's boards and records imply,
    slices no call named still at their fill value, nothing behind the rings touched."""
    torch = _torch()
    n, S_ = GP.N_STEP, GP.STORE_RING
    with capped(monkeypatch, name, n, seed=GP.STORE_SEED, layout=layout) as env:
        orc = O.EnvBatch(name, n, seed=GP.STORE_SEED)
        m = O.metrics_new()
        t = GP.store_prephase(env, orc, metrics=m)
        GP.assert_whole_batch(env, orc, "before the stores")
        rings = _rings(n, env.n_cells, S_)
        written = {k: set() for k in rings}
        four = tuple(rings[k][0] for k in ("successors", "actions", "rewards", "terminals"))
        sd = torch.tensor([GP.STORE_BASE], dtype=torch.int64, device="cuda")
        for i in range(GP.STORE_T):
            where = "%s %s cheat=%s store %d" % (name, layout, cheat, i)
            acts = GP.store_actions(i)
            env.step_store(torch.as_tensor(acts, device="cuda"), i, four, cheat=cheat, slice_dev=sd)
            rec = orc.rollout(1, seed=GP.STORE_SEED, actions=acts[None], auto_reset=False, metrics=m)
            t += 1
            sl = (GP.STORE_BASE + i) % S_
            _assert_slice(rings, "successors", sl, orc.export()[0], written, where)
            _assert_slice(rings, "actions", sl, (rec[:, 3].astype(np.uint8) & 3) if cheat else acts, written, where)
            _assert_slice(rings, "rewards", sl, rec[:, 1 if cheat else 0], written, where)
            _assert_slice(rings, "terminals", sl, rec[:, 2].astype(np.uint8), written, where)
            GP.assert_whole_batch(env, orc, where, rec=rec)
            env.reset_done_store(rings["states"][0], i + 1, slice_dev=sd)
            GP.oracle_reset(orc, np.flatnonzero(orc.export(boards=False)[1]["game_over"]))
            _assert_slice(rings, "states", (GP.STORE_BASE + i + 1) % S_, orc.export()[0], written, where + " reset")
            GP.assert_whole_batch(env, orc, where + " reset")
        assert written["successors"] == set(range(S_))  # the slice wrapped
        # the two-phase form into fresh rings, slice 1 named by the device scalar
        rings2 = _rings(n, env.n_cells, S_)
        written2 = {k: set() for k in rings2}
        sd2 = torch.tensor([1], dtype=torch.int64, device="cuda")
        acts = GP.store_actions(GP.STORE_T)
        a_dev = torch.as_tensor(acts, device="cuda")
        r5 = [_ptr(rings2[k][0]) for k in ("states", "successors", "actions", "rewards", "terminals")]
        before = orc.export()[0]
        env._sync_torch_to_lib()
        _lib.check(env.lib.sgk_replay_store(env.handle, 0, None, int(cheat), 0, _ptr(sd2), *r5))
        env._sync_lib_to_torch()
        env.step(a_dev, auto_reset=False)
        rec = orc.rollout(1, seed=GP.STORE_SEED, actions=acts[None], auto_reset=False, metrics=m)
        t += 1
        env._sync_torch_to_lib()
        _lib.check(env.lib.sgk_replay_store(env.handle, 1, _ptr(a_dev), int(cheat), 0, _ptr(sd2), *r5))
        env._sync_lib_to_torch()
        where = "%s %s cheat=%s two-phase" % (name, layout, cheat)
        _assert_slice(rings2, "states", 1, before, written2, where)
        _assert_slice(rings2, "successors", 1, orc.export()[0], written2, where)
        _assert_slice(rings2, "actions", 1, (rec[:, 3].astype(np.uint8) & 3) if cheat else acts, written2, where)
        _assert_slice(rings2, "rewards", 1, rec[:, 1 if cheat else 0], written2, where)
        _assert_slice(rings2, "terminals", 1, rec[:, 2].astype(np.uint8), written2, where)
        GP.assert_whole_batch(env, orc, where, rec=rec)
        GP.assert_metrics(env, m, t, where)


# ---- (c) the rollout kernels at the N_STREAM sizes -----------------------------------------------------------------------------------
def _rollout_case(monkeypatch, name, layout, n, dests, ring_nt=False):
    torch = _torch()
    ring, T, first = GP.STREAM_RING, GP.STREAM_T, GP.STREAM_FIRST
    with capped(monkeypatch, name, n, ring_nt=ring_nt, seed=GP.STREAM_SEED, layout=layout) as env:
        orc = O.EnvBatch(name, n, seed=GP.STREAM_SEED)
        m = O.metrics_new()
        t = GP.stream_prephase(env, orc, metrics=m)
        GP.assert_whole_batch(env, orc, "after the pre-phase")
        cells, tiles = env.n_cells, GP.n_tiles(n)
        for (w, steps), dest in zip(GP.stream_windows(orc, t, metrics=m, windows=len(dests)), dests):
            where = "%s %s n=%d window %d -> %s" % (name, layout, n, w, dest)
            if dest == "own":
                env.step_random(T, auto_reset=True, fused="stream")
            elif dest == "fused":
                env.step_random(T, auto_reset=True, fused=True)
            else:
                shape_b = (tiles, ring, 64, cells) if dest == "tile" else (ring, n, cells)
                shape_r = (tiles, ring, 64, 4) if dest == "tile" else (ring, n, 4)
                boards, tail_b = tailed(shape_b, torch.int8, -7)
                recs, tail_r = tailed(shape_r, torch.int8, -7)
                env.rollout_random_stream(T, boards=boards, recs=recs, first_slice=first, layout=dest)
                got_b = (env.ring_slices(boards) if dest == "tile" else boards).cpu().numpy()
                got_r = (env.ring_slices(recs) if dest == "tile" else recs).cpu().numpy()
                for k in range(T - ring, T):  # every slice still in the ring, step by step
                    sl = (first + k) % ring
                    bad = np.flatnonzero((got_b[sl] != steps[k][0]).any(axis=1))
                    assert bad.size == 0, (where, "boards of step %d, slice %d" % (k, sl), bad.size, bad[:5])
                    bad = np.flatnonzero((got_r[sl] != steps[k][1]).any(axis=1))
                    assert bad.size == 0, (where, "records of step %d, slice %d" % (k, sl), bad.size, bad[:5])
                if dest == "tile" and n % 64:  # the records of the padding rows stay the caller's
                    assert bool((recs[-1, :, n % 64:] == -7).all()), where
                assert untouched(tail_b, -7) and untouched(tail_r, -7), where
            t += T
            GP.assert_whole_batch(env, orc, where, rec=steps[-1][1])
            GP.assert_metrics(env, m, t, where)
        assert env.lockstep_t == t


@pytest.mark.parametrize("n", GP.STREAM_SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", GP.ENVS)
def test_rollout_kernels_take_a_second_pass(name, layout, n, monkeypatch):
    """269 tiles on 256 waves: waves 0..12 take a second tile, whose state word comes from memory and not from the word prefetched for
    the first one, and re-derive every ring pointer. 23 steps each into the env's own buffers, a slice-major ring of 7 from slice 5
    (wraps three times), a tile-major ring likewise, and outputs once; after a pre-phase that leaves no two tiles alike."""
    _rollout_case(monkeypatch, name, layout, n, GP.STREAM_DESTS)


@pytest.mark.parametrize("dest,n", [("slice", GP.N_STREAM_ALIGNED), ("tile", GP.N_STREAM)])
@pytest.mark.parametrize("name", ["BoatRace-v0", "SideEffectsSokoban-v0"])
def test_ring_tiles_through_the_nontemporal_store_path(name, dest, n, monkeypatch):
    """SGK_RING_NT=1: the board tiles go into the ring as non-temporal stores, which the size rule picks from 256 MiB on only. Where
    the ring takes whole tiles: aligned slices (with a partial last tile) and the tile-major layout."""
    _rollout_case(monkeypatch, name, "compact", n, (dest,), ring_nt=True)


# ---- (d) tabular-Q -------------------------------------------------------------------------------------------------------------------
TABQ_SEED = 21
TABQ_CASES = [("IslandNavigation-v0", True, 40, 0), ("BoatRace-v0", False, 103, 0), ("TomatoWatering-v0", False, 50, 64)]


@functools.lru_cache(maxsize=4)
def _tabq_oracle(name, n, steps, cheat):
    """(oracle envs, its dict agents, metrics, actions [steps, n]) after `steps` learning steps: computed once per level, read only."""
    return P._oracle_tabq(name, n, steps, TABQ_SEED, cheat)


def _tabq_args(capacity):
    a = P._tabq_args()
    if capacity:
        a.hash_capacity = capacity
    return a


def _assert_block_tables(env, agent, agents, where):
    """The float64 tables, as bit patterns, of 64-agent blocks from the first pass, every later pass and the tail, against the
    oracle's dictionaries: every row the device holds is the oracle's row for the board that state renders to."""
    n, seen = env.n_envs, 0
    hashed = env.name == "TomatoWatering-v0"
    if hashed:
        import hostlib
        import test_tables_cpu as TT

        R = TT._rules(hostlib.load(), S.ENV_IDS[env.name])
    for lo in GP.sample_blocks(n):
        tab = agent.table_host(lo, 64)
        keys = agent.keys_host(lo, 64) if hashed else None
        for i in range(64):
            ag = agents[lo + i]
            if hashed:
                occ = np.flatnonzero(keys[i] != 0xFFFFFFFF)
                assert len(set(keys[i, occ].tolist())) == len(occ) and ag.n_rows <= len(occ) <= ag.n_rows + 1, (where, lo + i)
                assert not np.abs(tab[i][keys[i] == 0xFFFFFFFF]).any(), (where, lo + i)
                rows = [(int(s), TT._product_board(env.name, R, int(keys[i, s]) & 0xFF, (int(keys[i, s]) >> 8) & 0x1FFF, 0)) for s in occ]
            else:
                nz = np.flatnonzero(np.abs(tab[i]).sum(axis=1))
                assert ag.n_rows >= len(nz), (where, lo + i)
                rows = [(int(s), P._board_of_state(env, int(s))) for s in nz]
            for s, board in rows:
                want = ag.lookup(board)
                assert (want.view(np.uint64) == tab[i, s].view(np.uint64)).all(), (where, lo + i, s, want, tab[i, s])
                seen += 1
    assert seen > 0, where


def _assert_tabq(env, agent, orc, agents, m, steps, where):
    assert agent.t == steps and env.lockstep_t == steps, where
    GP.assert_whole_batch(env, orc, where)
    GP.assert_metrics(env, m, steps, where)
    _assert_block_tables(env, agent, agents, where)


@pytest.mark.parametrize("path", ["step", "calls"])
@pytest.mark.parametrize("name,cheat,steps,capacity", TABQ_CASES)
def test_tabq_per_step_kernels_above_the_small_threshold(name, cheat, steps, capacity, path, monkeypatch):
    """66 341 private agents. "step": sgk_tabq_learn_steps (the one-launch tabq_step_kernel in its large form, replayed from a
    graph) and three agent.step() calls whose actions are the oracle's; "calls": tabq_act, env.step, tabq_learn, reset_done, one
    launch each and five passes each. Whole-batch env state, metrics, step counter; sampled tables."""
    _torch()
    n = GP.N_STEP
    orc, agents, m, acts = _tabq_oracle(name, n, steps, cheat)
    with capped(monkeypatch, name, n, seed=TABQ_SEED) as env:
        agent = S.BatchedTabularQAgent(env, _tabq_args(capacity))
        try:
            if path == "step":
                agent.learn_steps(steps - 3, cheat=cheat)
                for k in range(steps - 3, steps):
                    a, _ = agent.step(cheat=cheat)
                    assert a.cpu().numpy().tobytes() == acts[k].tobytes(), (name, "step", k)
            else:
                for k in range(steps):
                    a = agent.act_explore()
                    assert a.cpu().numpy().tobytes() == acts[k].tobytes(), (name, "calls", k)
                    env.step(a, auto_reset=False, write_boards=(k == steps - 1))
                    agent.learn(action=a, cheat=cheat)
                    env.reset_done()
            _assert_tabq(env, agent, orc, agents, m, steps, "%s %s" % (name, path))
        finally:
            agent.close()


def _oracle_greedy_eval(orc, agents, n_reset_steps, n_tail_steps, seed):
    """default_eval on the oracle with the dict agents acting greedily: reset, n_reset_steps steps with reset-on-done, n_tail_steps
    without. An agent is asked again only when its env's board changed (nothing learns: the same board gets the same action)."""
    n = orc.n
    orc.reset()
    m = O.metrics_new()
    acts = np.zeros(n, dtype=np.uint8)
    prev = None
    for k in range(n_reset_steps + n_tail_steps):
        boards, f = orc.export()
        ask = (f["game_over"] == 0) & (True if prev is None else (boards != prev).any(axis=1))
        for i in np.flatnonzero(ask):
            acts[i] = agents[i].act(boards[i])
        orc.rollout(1, seed=seed, actions=acts[None], auto_reset=k < n_reset_steps, metrics=m)
        prev = boards
    return m


def test_tabq_hbm_rollout_and_evaluation_take_a_second_pass(monkeypatch):
    """SideEffectsSokoban (tables of n_cells^2 rows: HBM-resident) at 17 189 agents: tabq_rollout_hbm_kernel for 104 steps, then
    tabq_eval_hbm_kernel, greedy, two steps with reset-on-done and the 100-step tail. The evaluation leaves tables and step counter
    alone."""
    _torch()
    name, n, steps = "SideEffectsSokoban-v0", GP.N_STREAM, 104
    orc, agents, m, _ = P._oracle_tabq(name, n, steps, TABQ_SEED, False)
    with capped(monkeypatch, name, n, seed=TABQ_SEED) as env:
        agent = S.BatchedTabularQAgent(env, _tabq_args(0))
        try:
            agent.rollout(steps, kernel="hbm")
            _assert_tabq(env, agent, orc, agents, m, steps, "hbm rollout")
            horizon = int(env.info.max_iterations)
            got = agent.evaluate(3, kernel="hbm")
            m_eval = _oracle_greedy_eval(orc, agents, 2, horizon, TABQ_SEED)
            assert got.steps == n * (2 + horizon) and agent.t == steps
            GP.assert_whole_batch(env, orc, "hbm evaluation")
            GP.assert_metrics(env, m_eval, 2 + horizon, "hbm evaluation")
            assert m_eval[O.M_EPISODES] >= n
            _assert_block_tables(env, agent, agents, "after the evaluation")
        finally:
            agent.close()


# ---- (e) the rest on a capped handle -------------------------------------------------------------------------------------------------
def test_draw_kernels_take_a_second_pass(monkeypatch):
    torch = _torch()
    n, seed, base = GP.N_STREAM, 31, 4096
    assert GP.lane_passes(n) == 2
    rng = np.random.RandomState(4)
    with capped(monkeypatch, "BoatRace-v0", n, seed=seed, env_index_base=base) as env:
        scores = rng.randn(n, 4).astype(np.float32)
        scores[::7, 1] = scores[::7, 3]  # ties: the first maximum wins
        sc = torch.as_tensor(scores, device="cuda")
        for eps, draw in ((0.0, 0), (0.3, 5), (1.0, 2 ** 31 + 9)):
            out, tail = tailed((n,), torch.uint8, 99)
            env.epsilon_greedy(sc, eps, draw, out=out)
            got = out.cpu().numpy()
            want = O.eps_greedy(scores, eps, seed, base, draw)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0 and untouched(tail, 99), (eps, draw, bad[:5])
        logits = (rng.randn(n, 4) * 1.5).astype(np.float32)
        lg = torch.as_tensor(logits, device="cuda")
        for draw in (0, 77):
            out, tail = tailed((n,), torch.uint8, 99)
            env.categorical_sample(lg, draw, out=out)
            got = out.cpu().numpy()
            want, margin = O.categorical_sample(logits, seed, base, draw)
            clear = margin > BOUNDARY  # (a draw this close to an interval boundary may flip with the last bit of expf: test_gpu_ppo.py)
            assert clear.mean() > 0.999 and clear[GP.later_pass(n)].any() and (got[clear] == want[clear]).all(), draw
            assert untouched(tail, 99)


def test_discounted_returns_scan_takes_a_third_pass(monkeypatch):
    """1 061 ragged trajectories on 2 x 64 workgroups of 4 waves: two whole passes and 37 trajectories of a third. Bit for bit the
    oracle's float32 sums, in the shared-discount form and with a discount per trajectory (1 061 members of one)."""
    torch = _torch()
    n, T = GP.N_RETURNS, 70
    rng = np.random.RandomState(1)
    rewards = rng.choice([-1.0, 2.0, 49.0, -51.0, 0.5], size=(n, T)).astype(np.float32)
    lengths = rng.randint(0, T + 1, size=n).astype(np.int32)
    lengths[[0, 511, 512, 1023, 1024, n - 1]] = [T, 1, T, 65, T, 64]
    discounts = [0.97, 0.9, 1.0]
    with capped(monkeypatch, "BoatRace-v0", 64) as env:
        r_dev, l_dev = torch.as_tensor(rewards, device="cuda"), torch.as_tensor(lengths, device="cuda")
        out, tail = tailed((n, T), torch.float32, 7.5)
        env.discounted_returns(r_dev, 0.97, lengths=l_dev, out=out)
        got = out.cpu().numpy()
        for i in range(n):
            want = O.discounted_returns(rewards[i, :lengths[i]], 0.97) if lengths[i] else np.zeros(0, np.float32)
            assert (got[i, :lengths[i]].view(np.uint32) == want.view(np.uint32)).all(), i
            assert (got[i, lengths[i]:] == 7.5).all(), i
        assert untouched(tail, 7.5)
        gp = torch.as_tensor(np.stack([_lib.discount_powers(discounts[i % 3], T) for i in range(n)]), device="cuda")
        out, tail = tailed((n, T), torch.float32, 7.5)
        env.discounted_returns_members(r_dev, gp, lengths=l_dev, out=out)
        got = out.cpu().numpy()
        for i in range(n):
            want = O.discounted_returns(rewards[i, :lengths[i]], discounts[i % 3]) if lengths[i] else np.zeros(0, np.float32)
            assert (got[i, :lengths[i]].view(np.uint32) == want.view(np.uint32)).all(), i
            assert (got[i, lengths[i]:] == 7.5).all(), i
        assert untouched(tail, 7.5)


def _vote_host(member_actions, members, live, dissent):
    a = np.ascontiguousarray(member_actions, dtype=np.uint8)
    M, n = a.shape
    ids = None if members is None else np.ascontiguousarray(members, dtype=np.int32)
    mask = np.ascontiguousarray(live, dtype=np.uint8)
    actions, votes = np.full(n, 9, dtype=np.uint8), np.full((n, 4), 77, dtype=np.uint16)
    _lib.check(_lib.load().sgk_members_vote_host(a.ctypes.data, M, n, None if ids is None else ids.ctypes.data,
                                                 0 if ids is None else len(ids), mask.ctypes.data, actions.ctypes.data,
                                                 votes.ctypes.data, dissent.ctypes.data))
    return actions, votes


def test_members_vote_takes_a_second_pass(monkeypatch):
    """sgk_members_vote at 17 189 envs, some of them over, against the host vote: all seven members and a listed subset, the counts
    and the dissent counters (which gain, and only over the envs whose episode is not over)."""
    torch = _torch()
    name, n, seed, M = "IslandNavigation-v0", GP.N_STREAM, 12, 7
    rng = np.random.RandomState(6)
    with capped(monkeypatch, name, n, seed=seed) as env:
        env.step_random(30, auto_reset=False)
        live = env.episode_state_host()["over"] == 0
        later = GP.later_pass(n)
        assert live[later].any() and not live[later].all() and live[~later].any() and not live[~later].all()
        ma = rng.randint(0, 4, size=(M, n)).astype(np.uint8)
        ma[:, ::11] = ma[0, ::11]  # unanimous envs
        ma_dev = torch.as_tensor(ma, device="cuda")
        for members in (None, [5, 0, 3]):
            want_d = np.array([5, 7], dtype=np.int64)
            want_a, want_v = _vote_host(ma, members, live, want_d)
            out, tail = tailed((n,), torch.uint8, 99)
            votes, vtail = tailed((n, 4), torch.int16, -7)
            dissent = torch.tensor([5, 7], dtype=torch.int64, device="cuda")
            ids = None if members is None else torch.tensor(members, dtype=torch.int32, device="cuda")
            env.members_vote(ma_dev, members=ids, out=out, votes_out=votes, dissent=dissent)
            assert (out.cpu().numpy() == want_a).all(), members
            assert (votes.cpu().numpy().view(np.uint16) == want_v).all(), members
            assert dissent.cpu().numpy().tolist() == want_d.tolist() and want_d[1] > 7, members
            assert untouched(tail, 99) and untouched(vtail, -7)


@pytest.mark.parametrize("name", sorted(GP.SCAN_PLANS))
def test_finished_scan_carries_into_a_second_slab(name, monkeypatch):
    """262 437 envs are 1 026 workgroup counts: the exclusive scan runs a second 1 024-wide slab and must carry the first one's total
    into it. ids / returns / performances of the finished envs, ascending, against the oracle's done flags; then a masked reset."""
    torch = _torch()
    n = GP.N_SCAN
    with capped(monkeypatch, name, n, seed=GP.SCAN_SEED) as env:
        orc = GP.run_scan_plan(name, env=env)
        _, f = orc.export(boards=False)
        want = np.flatnonzero(f["game_over"])
        assert 0 < want.size < n and want[-1] >= GP.SCAN_SLAB * GP.WG
        bufs = [tailed((n,), torch.int32, -7) for _ in range(3)]
        count = ctypes.c_int64(0)
        env._sync_torch_to_lib()
        _lib.check(env.lib.sgk_finished(env.handle, *[_ptr(b) for b, _ in bufs], ctypes.byref(count)))
        env._sync_lib_to_torch()
        k = count.value
        ids, ret, perf = (b.cpu().numpy() for b, _ in bufs)
        assert k == want.size
        assert (ids[:k] == want).all(), np.flatnonzero(ids[:k] != want)[:5]
        assert (ret[:k] == f["last_episode_return"][want]).all() and (perf[:k] == f["last_performance"][want]).all()
        for got, (_, tail) in zip((ids, ret, perf), bufs):
            assert (got[k:] == -7).all() and untouched(tail, -7)
        a, b, c = env.finished()  # the wrapper's own buffers
        assert (a.cpu().numpy() == want).all() and (b.cpu().numpy() == ret[:k]).all() and (c.cpu().numpy() == perf[:k]).all()
        GP.assert_whole_batch(env, orc, "before the masked reset")
        mask = (np.random.RandomState(8).rand(n) < 0.3).astype(np.uint8)
        env.reset(torch.as_tensor(mask, device="cuda"))
        GP.oracle_reset(orc, np.flatnonzero(mask))
        GP.assert_whole_batch(env, orc, "after the masked reset")
