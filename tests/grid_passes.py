"""Sizes, plans and comparisons for the grid-pass tests (tests/test_grid_passes_cpu.py, tests/test_gpu_grid_passes.py).

The large-batch kernels walk their envs in passes: a launch has at most `cap` workgroups (6 / 16 / 12 per compute unit for the
grid-stride kernels / the streamed rollout / the outputs-once rollout) and a wave or a lane that has finished a tile goes on to the
one `cap` workgroups further. Below ~393 K envs no kernel ever takes a second pass with the default caps. A handle created with
SGK_MAX_GRID = SGK_STREAM_GRID = SGK_ROLLOUT_GRID = 64 (read once, at sgk_create) takes them from 16 385 envs on, and the sizes
here are the smallest at which each path exists. Nothing in this module needs a GPU."""
import numpy as np

from oracle import oracle as O

CAP = 64                     # workgroups per launch on a capped handle (the smallest value the knobs accept)
WG = 256                     # lanes per workgroup of the large-batch kernels (csrc/sgk_kernels.h)
WAVES = CAP * WG // 64       # waves per launch: one 64-env tile each per pass
LANE_STRIDE = CAP * WG       # envs per pass of the one-lane-per-env kernels
STEP_SMALL_MAX_ENVS = 65536  # csrc/sgk_step.hip, csrc/sgk_tabq.hip: up to here the per-step kernels run their SMALL form (no loop)
SCAN_SLAB = 1024             # workgroup counts finished_scan_kernel scans per iteration; `carry` links the slabs
THREADS = 16                 # oracle threads (rollout_mt)
TAIL = 259                   # sentinel elements behind every over-allocated output: more than one workgroup of lanes

N_STEP = STEP_SMALL_MAX_ENVS + 3 * WG + 37
N_STREAM = LANE_STRIDE + 3 * WG + 37
N_STREAM_WHOLE = 269 * 64          # whole tiles, 16-byte aligned slices on every level
N_STREAM_ALIGNED = 268 * 64 + 48   # aligned slices, a partial last tile
N_SCAN = SCAN_SLAB * WG + WG + 37
N_RETURNS = 2 * 512 + 37           # trajectories: the returns scan runs 2 * cap workgroups of 4 waves, one trajectory per wave
STREAM_SIZES = (N_STREAM, N_STREAM_WHOLE, N_STREAM_ALIGNED)

ENVS = ["BoatRace-v0", "IslandNavigation-v0", "SideEffectsSokoban-v0", "DistributionalShift-v0", "WhiskyGold-v0",
        "AbsentSupervisor-v0", "SafeInterruptibility-v0", "ConveyorBelt-v0", "TomatoWatering-v0", "FriendFoe-v0"]


def n_tiles(n):
    return (n + 63) // 64


def tiles_of_wave(n, wave):
    """How many 64-env tiles wave `wave` of a capped launch works."""
    return len(range(wave, n_tiles(n), WAVES))


def later_pass(n):
    """bool [n]: the env lies in a tile that a wave reaches on its second or a later pass."""
    return np.arange(n) >= WAVES * 64


def partial_tile(n):
    """bool [n]: the env lies in the last tile and that tile is not whole (all False where n is a multiple of 64)."""
    return (np.arange(n) >= (n // 64) * 64) & (n % 64 != 0)


def lane_passes(n):
    return (n + LANE_STRIDE - 1) // LANE_STRIDE


def sample_blocks(n, block=64):
    """Starts of `block`-agent blocks: the first pass, every later pass of the one-lane-per-env kernels (= of the waves: 256 tiles
    are 16 384 envs), and the tail that ends at n."""
    return sorted({p * LANE_STRIDE for p in range(lane_passes(n))} | {n - block})


def _derive():
    # the per-step kernels: above the SMALL threshold, 1 037 wave tiles on 256 waves
    assert N_STEP == 66341 and N_STEP > STEP_SMALL_MAX_ENVS and n_tiles(N_STEP) == 1037 and WAVES == 256
    assert [tiles_of_wave(N_STEP, w) for w in (0, 12, 13, 255)] == [5, 5, 4, 4]
    assert (n_tiles(N_STEP) - 1) % WAVES == 12 and (n_tiles(N_STEP) - 1) // WAVES == 4  # the partial tile is wave 12's fifth ...
    assert N_STEP % 64 == 37 and partial_tile(N_STEP).sum() == 37                       # ... and holds 37 envs
    assert lane_passes(N_STEP) == 5 and LANE_STRIDE == 16384
    # the rollout kernels: 269 tiles, waves 0..12 take a second one, the partial tile lies in the second pass
    assert N_STREAM == 17189 and n_tiles(N_STREAM) == 269
    assert [tiles_of_wave(N_STREAM, w) for w in (0, 12, 13)] == [2, 2, 1]
    assert (n_tiles(N_STREAM) - 1) // WAVES == 1 and N_STREAM % 64 == 37 and N_STREAM % 2 == 1
    assert N_STREAM_WHOLE == 17216 and N_STREAM_WHOLE % 64 == 0 and n_tiles(N_STREAM_WHOLE) == 269
    assert N_STREAM_ALIGNED == 17200 and N_STREAM_ALIGNED % 64 == 48 and n_tiles(N_STREAM_ALIGNED) == 269
    # slices of a slice-major ring: at N_STREAM (odd) unaligned, so written row by row, on every level whose cell count is no multiple
    # of 16 -- all but the three 6 x 8 levels, whose rows are whole 16-byte chunks at any n --, and aligned at the two companions
    unaligned = []
    for name in ENVS:
        H, W = O.shape(name)
        assert H * W > 16 and ((N_STREAM * H * W) % 16 != 0) == ((H * W) % 16 != 0), name
        unaligned += [name] if (N_STREAM * H * W) % 16 else []
        assert (N_STREAM_WHOLE * H * W) % 16 == 0 and (N_STREAM_ALIGNED * H * W) % 16 == 0, name
    assert sorted(set(ENVS) - set(unaligned)) == ["AbsentSupervisor-v0", "IslandNavigation-v0", "WhiskyGold-v0"]
    # the finished-env scan: 1 026 workgroup counts, a second slab of two
    assert N_SCAN == 262437 and (N_SCAN + WG - 1) // WG == SCAN_SLAB + 2
    assert N_RETURNS == 1061 and (N_RETURNS + 3) // 4 > 2 * CAP and N_RETURNS % 4 == 1
    assert TAIL > WG


_derive()


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
def assert_whole_batch(env, orc, where, boards=True, rec=None):
    """Every env of the device batch against the oracle: boards, every state field, the episode arrays, FriendFoe's estimates, and
    the step records where the oracle's last step handed them out."""
    n = env.n_envs
    ob, f = orc.export(boards=boards)
    if boards:
        got = env.boards_host().reshape(n, -1)
        bad = np.flatnonzero((got != ob).any(axis=1))
        assert bad.size == 0, "%s: boards differ at %d envs, first %s" % (where, bad.size, bad[:5])
    st, le = env.episode_state_host(), env.last_episode_host()
    for key, name in (("episode_return", "episode_return"), ("hidden_return", "hidden_return"), ("frame", "frame"),
                      ("over", "game_over"), ("agent_cell", "agent_cell"), ("box_cell", "box_cell")):
        bad = np.flatnonzero(st[key] != f[name])
        assert bad.size == 0, "%s: %s differs at %d envs, first %s" % (where, key, bad.size, bad[:5])
    bad = np.flatnonzero(le["n_episodes"] != f["n_episodes"])
    assert bad.size == 0, "%s: n_episodes differs at %d envs, first %s" % (where, bad.size, bad[:5])
    fin = f["n_episodes"] > 0
    assert (le["last_return"][fin] == f["last_episode_return"][fin]).all(), where
    assert (le["last_performance"][fin] == f["last_performance"][fin]).all(), where
    if env.name == "FriendFoe-v0":
        assert (env.bandit_policy().view(np.uint64) == orc.foe_policy().view(np.uint64)).all(), where
    if rec is not None:
        got = env.step_records_host()
        bad = np.flatnonzero((got != rec).any(axis=1))
        assert bad.size == 0, "%s: step records differ at %d envs, first %s" % (where, bad.size, bad[:5])


def assert_metrics(env, m, steps, where):
    want = m.copy()
    want[O.M_STEPS] = env.n_envs * steps  # the library counts the lockstep env-steps it issued
    assert env.metrics().tolist() == want.tolist(), where


def oracle_random(orc, k, seed, t, auto_reset=True, metrics=None, threads=1, env_begin=0):
    """k random-action lockstep steps on the oracle from lockstep time t; the last step's records. With threads the first k - 1
    steps run threaded (that form hands out no records)."""
    if threads > 1 and k > 1:
        O.rollout_mt(orc, k - 1, threads, seed=seed, env_begin=env_begin, t_begin=t, auto_reset=auto_reset, metrics=metrics)
        t, k = t + k - 1, 1
    return orc.rollout(k, seed=seed, env_begin=env_begin, t_begin=t, auto_reset=auto_reset, metrics=metrics)


def oracle_reset(orc, ids):
    for i in ids:
        orc.reset(int(i))


# ---- one operation of a schedule -----------------------------------------------------------------------------------------------------
OPS = ["graph", "fused", "stream", "ring", "given", "repeat", "reset_done", "mask", "noreset"]


def schedule_op(env, orc, rng, op, k, t, seed, ring_b=None, ring_r=None, what="", auto=None, write_boards=True, metrics=None,
                threads=1):
    """One operation of a schedule of every kind of step, on the device batch `env` (None: the oracle alone, no GPU) and on the oracle
    `orc`, drawn from `rng` where the operation leaves something open: random-action steps as graph replays / the fused rollout / the
    streamed rollout (into the env's own buffers, or into the 5-slice rings ring_b / ring_r, which are compared here), given-action
    and repeated-action steps (auto: auto-reset, drawn when None), reset_done, a masked reset of a fifth of the batch, random steps
    without auto-reset. Returns (lockstep time after it, the steps it took, {"rec": the last step's records or None, "actions": the
    given actions or None})."""
    n = orc.n
    info = {"rec": None, "actions": None}
    torch = None
    if env is not None:
        import torch
    if op in ("graph", "fused", "stream", "noreset"):
        auto_r = op != "noreset"
        if env is not None:
            env.step_random(k, auto_reset=auto_r, fused={"graph": False, "noreset": False, "fused": True, "stream": "stream"}[op],
                            write_boards=write_boards)
        info["rec"] = oracle_random(orc, k, seed, t, auto_r, metrics, threads)
        return t + k, k, info
    if op == "ring":
        first = int(rng.randint(0, 5))
        if env is not None:
            env.rollout_random_stream(k, boards=ring_b, recs=ring_r, first_slice=first)
        for j in range(k):
            rec = orc.rollout(1, seed=seed, t_begin=t + j, auto_reset=True, metrics=metrics)
            if env is not None and j >= k - 5:  # the last five steps are still in the ring
                sl = (first + j) % 5
                assert (ring_b[sl].cpu().numpy() == orc.boards()).all(), what
                assert (ring_r[sl].cpu().numpy() == np.asarray(rec)).all(), what
        info["rec"] = rec
        return t + k, k, info
    if op == "given":
        acts = rng.randint(0, 4, size=n).astype(np.uint8)
        if auto is None:
            auto = bool(rng.randint(0, 2))
        if env is not None:
            env.step(torch.as_tensor(acts, device="cuda"), auto_reset=auto, write_boards=write_boards)
        info["rec"] = orc.rollout(1, seed=seed, actions=acts[None], auto_reset=auto, metrics=metrics)  # (the seed keys env-side draws)
        info["actions"] = acts
        return t + 1, 1, info
    if op == "repeat":
        k = min(k, 17)
        acts = rng.randint(0, 4, size=n).astype(np.uint8)
        if env is not None:
            env.step_repeat(torch.as_tensor(acts, device="cuda"), k, auto_reset=True, write_boards=write_boards)
        info["rec"] = orc.rollout(k, seed=seed, actions=np.repeat(acts[None], k, axis=0), auto_reset=True, metrics=metrics)
        info["actions"] = acts
        return t + k, k, info
    if op == "reset_done":
        if env is not None:
            env.reset_done()
        oracle_reset(orc, np.flatnonzero(orc.export(boards=False)[1]["game_over"]))
        return t, 0, info
    assert op == "mask", op
    m = (rng.rand(n) < 0.2).astype(np.uint8)
    if env is not None:
        env.reset(torch.as_tensor(m, device="cuda"))
    oracle_reset(orc, np.flatnonzero(m))
    return t, 0, info


# ---- (a) the per-step kernels: a shortened schedule at N_STEP ------------------------------------------------------------------------
# (operation, steps, auto-reset of a given-action step, boards written). 100 lockstep steps before the last given-action step: on
# the fixed-horizon levels (BoatRace, ConveyorBelt, TomatoWatering: every episode lasts 100 steps) that step ends the episode of
# every env the masked reset left alone, in every tile, and the graph replays behind it end those of the envs the masked reset
# restarted at step 10; elsewhere episodes end all along.
STEP_PLAN = [("graph", 5, None, True), ("given", 1, True, True), ("given", 1, False, False), ("repeat", 3, None, True),
             ("mask", 0, None, True), ("graph", 64, None, True), ("noreset", 17, None, True), ("reset_done", 0, None, True),
             ("given", 1, False, True), ("given", 1, True, False), ("graph", 6, None, False), ("given", 1, True, True),
             ("graph", 12, None, True)]
STEP_SEED = 211


def run_step_plan(name, env=None, check=None, threads=THREADS):
    """STEP_PLAN on the oracle (and on `env`); check(op index, op, orc, info, t, metrics, boards written) after every operation.
    Returns the per-operation facts the CPU test asserts on: [(op, given actions or None, bool [n] an episode ended during the op)]."""
    orc = O.EnvBatch(name, N_STEP, seed=STEP_SEED)
    rng = np.random.RandomState(len(name) + 17)
    m = O.metrics_new()
    t, facts = 0, []
    for i, (op, k, auto, wb) in enumerate(STEP_PLAN):
        before = orc.export(boards=False)[1]["n_episodes"].copy()
        t, _, info = schedule_op(env, orc, rng, op, k, t, STEP_SEED, auto=auto, write_boards=wb, metrics=m, threads=threads)
        ended = orc.export(boards=False)[1]["n_episodes"] != before
        facts.append((op, info["actions"], ended))
        if check is not None:
            check(i, op, orc, info, t, m, wb)
    return orc, m, t, facts


# ---- (b) the fused replay stores at N_STEP -------------------------------------------------------------------------------------------
STORE_SEED, STORE_T, STORE_RING, STORE_BASE = 23, 4, 3, 2  # slice (STORE_BASE + i) % STORE_RING: the second store wraps


def store_prephase(env, orc, metrics=None, threads=THREADS):
    """98 random steps: the second of the stores that follow is every untouched episode's 100th step (the time limit of both levels),
    so a launch writes terminal flags of both values into every tile. Returns the lockstep time."""
    if env is not None:
        env.step_random(98, auto_reset=True)
    O.rollout_mt(orc, 98, threads, seed=STORE_SEED, t_begin=0, auto_reset=True, metrics=metrics)
    return 98


def store_actions(i, n=N_STEP):
    return np.random.RandomState(1000 + i).randint(0, 4, size=n).astype(np.uint8)


# ---- (c) the rollout kernels at the N_STREAM sizes -----------------------------------------------------------------------------------
STREAM_SEED, STREAM_T, STREAM_RING, STREAM_FIRST = 9, 23, 7, 5
STREAM_DESTS = ("own", "slice", "tile", "fused")
assert STREAM_FIRST + STREAM_T > 3 * STREAM_RING  # the ring wraps three times


def stream_prephase(env, orc, metrics=None, seed=STREAM_SEED, threads=THREADS):
    """100 random steps with a masked reset of the envs i % 5 == j after every 20: the envs' episodes end up 20 steps apart, so that
    every 23-step window that follows ends episodes in every tile on the fixed-horizon levels too -- and no rollout starts from
    the reset state, where every tile's state words are alike. Returns the lockstep time."""
    n, t = orc.n, 0
    for j in range(5):
        if env is not None:
            env.step_random(20, auto_reset=True)
        O.rollout_mt(orc, 20, threads, seed=seed, t_begin=t, auto_reset=True, metrics=metrics)
        t += 20
        mask = (np.arange(n) % 5 == j).astype(np.uint8)
        if env is not None:
            import torch

            env.reset(torch.as_tensor(mask, device="cuda"))
        oracle_reset(orc, np.flatnonzero(mask))
    return t


def stream_windows(orc, t, metrics=None, seed=STREAM_SEED, windows=len(STREAM_DESTS)):
    """The oracle through `windows` rollouts of STREAM_T steps, step by step: yields (window, [(boards, records)] of its steps)."""
    for w in range(windows):
        steps = []
        for k in range(STREAM_T):
            rec = orc.rollout(1, seed=seed, t_begin=t, auto_reset=True, metrics=metrics)
            t += 1
            steps.append((orc.export()[0], rec))
        yield w, steps


# ---- (e) finished() at N_SCAN --------------------------------------------------------------------------------------------------------
SCAN_SEED = 5
SCAN_PLANS = {"BoatRace-v0": (60, 40), "IslandNavigation-v0": (0, 30)}  # (steps before a masked reset of ~half the envs, steps after it)


def run_scan_plan(name, env=None, threads=THREADS):
    """Random steps without auto-reset around a masked reset of about half the batch: afterwards a part of the envs is done, in both
    slabs of the scan. Returns the oracle."""
    pre, post = SCAN_PLANS[name]
    orc = O.EnvBatch(name, N_SCAN, seed=SCAN_SEED)
    t = 0
    if pre:
        if env is not None:
            env.step_random(pre, auto_reset=False)
        O.rollout_mt(orc, pre, threads, seed=SCAN_SEED, t_begin=0, auto_reset=False)
        t = pre
        mask = (np.random.RandomState(3).rand(N_SCAN) < 0.5).astype(np.uint8)
        if env is not None:
            import torch

            env.reset(torch.as_tensor(mask, device="cuda"))
        oracle_reset(orc, np.flatnonzero(mask))
    if env is not None:
        env.step_random(post, auto_reset=False)
    O.rollout_mt(orc, post, threads, seed=SCAN_SEED, t_begin=t, auto_reset=False)
    return orc
