"""The two-channel conv body (sgk_convq_act_trans, sgk_convq_sample_trans, sgk_convq_rollout_trans) on the CPU: a float64 forward on the
observation of a transition env, [previous board, board], and an emulation of the fused rollout -- the oracle (oracle/, the C restatement
the step kernels are pinned to) steps the envs, the float64 forward chooses greedily. Plain torch on .double() tensors; nothing here
calls the product's code. tests/test_transition_cpu.py asserts the conditions the GPU tests stand on; tests/test_gpu_transition_body.py
compares the kernels with what this file computes.

The weight families are those of tests/forward_reference.py: "integer" (every partial sum of every accumulation is an integer below
2^24 in any order, so float32 is exact and the kernel's scores must EQUAL float64's) and "real" (torch's default ranges, biases in
+-0.3), with w1 [C, 2, 3, 3] and wb [C, 2, 1, 1]: channel 0 = the previous board, channel 1 = the current one."""
import functools

import numpy as np
import torch

import learner_reference as R

LEVEL = "BoatRace-v0"             # the level TransitionBoatRace wraps, and the one board (5 x 5) the two-channel kernels exist for
SHAPE = (5, 5)
CELLS = 25
CHANNELS = (4, 5, 8)              # 5: the lone fifth channel on the VALU (its first-convolution row is w1 + 4 * 18)
ENVS_PER_PASS = 512 // (SHAPE[0] * (SHAPE[1] + 1))  # 17 (ConvQGeom::ENVS)
N = 40                            # passes of 17, 17 and 6 envs
ENV_SEED = 23
PRE_STEPS = 9                     # random lockstep steps first: the envs differ, and the 100-step episodes end 91 steps into a rollout
EXACT_LIMIT = 2 ** 24
DEFAULT_CUS = 256

# per channel count the seed of the integer weights the rollout tests use: the first draw (8200 + 1000 j + C) under which the emulated
# runs meet test_transition_cpu.py's conditions (a) - (d) -- few do: a greedy policy with arbitrary weights soon stands still, and then
# [previous, current] is [current, current]; `python tests/transition_reference.py` prints the table anew (minutes)
ROLLOUT_SEEDS = {4: 22204, 5: 152205, 8: 120208}


def second_pass_n(cus=DEFAULT_CUS):
    """Envs of the grid-stride case: one pass more than the largest grid the launch code can choose on `cus` compute units (at most
    four workgroups per compute unit), and a partial one -- as forward_reference.case_n sizes its "multi" cases."""
    return ENVS_PER_PASS * (4 * cus) + 23


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def weights(family, channels, seed):
    """w1 [C,2,3,3], b1, w2 [C,C,3,3], b2, wb [C,2,1,1], bb, wh [C,C,3,3], bh, wl [4, C * cells], bl: float32, torch's layouts."""
    rng = np.random.default_rng(seed)
    C = channels
    if family == "integer":
        return [_ints(rng, -2, 2, (C, 2, 3, 3)), _ints(rng, -3, 3, (C,)), _ints(rng, -1, 1, (C, C, 3, 3)), _ints(rng, -3, 3, (C,)),
                _ints(rng, -2, 2, (C, 2, 1, 1)), _ints(rng, -3, 3, (C,)), _ints(rng, -1, 1, (C, C, 3, 3)), _ints(rng, -3, 3, (C,)),
                _ints(rng, -1, 1, (4, C * CELLS)), _ints(rng, -3, 3, (4,))]
    out = []
    for shape in ((C, 2, 3, 3), (C, C, 3, 3), (C, 2, 1, 1), (C, C, 3, 3), (4, C * CELLS)):
        k = 1.0 / np.sqrt(float(np.prod(shape[1:])))  # torch's default bound; the biases from U(-0.3, 0.3): a dropped bias must show
        out += [rng.uniform(-k, k, shape).astype(np.float32), rng.uniform(-0.3, 0.3, shape[:1]).astype(np.float32)]
    return out


def _T(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)


def _obs(prev, cur, dtype):
    n = len(cur)
    return torch.stack((_T(np.asarray(prev).reshape((n,) + SHAPE), dtype), _T(np.asarray(cur).reshape((n,) + SHAPE), dtype)), dim=1)


def forward(prev, cur, w, dtype=torch.float64):
    """Scores float64 [n, 4] of the observations [previous board, board] (int8 [n, cells] each), computed in `dtype`:
    trunk = relu(conv3x3(relu(conv3x3(x, 2 -> C)), C -> C)) + conv1x1(x, 2 -> C); out = linear(flatten(relu(conv3x3(trunk))))."""
    w = [_T(p, dtype) for p in w]
    with torch.no_grad():
        return R.cnn_head(R.cnn_trunk(_obs(prev, cur, dtype), w), *w[6:10]).double().numpy()


def abs_sum_bound(prev, cur, w):
    """The largest sum of absolute terms (bias included) of any accumulation of any env, in float64 (forward_reference.abs_sum_bound
    for two input channels): below 2^24 with integer weights and boards, float32 is exact in every order."""
    w = [_T(p, torch.float64) for p in w]
    F = torch.nn.functional
    conv = lambda t, wt, b: F.conv2d(t, wt, b.reshape(-1), padding=wt.shape[-1] // 2)  # noqa: E731
    with torch.no_grad():
        x = _obs(prev, cur, torch.float64)
        h1 = torch.relu(conv(x, w[0], w[1]))
        tops = [conv(x.abs(), w[0].abs(), w[1].abs()), conv(h1, w[2].abs(), w[3].abs()), conv(x.abs(), w[4].abs(), w[5].abs())]
        trunk = R.cnn_trunk(x, w)
        tops.append(torch.relu(conv(h1, w[2], w[3])) + tops[2])  # the residual add
        hh = torch.relu(conv(trunk, w[6], w[7]))
        tops += [conv(trunk.abs(), w[6].abs(), w[7].abs()), hh.flatten(1) @ w[8].abs().t() + w[9].abs()]
        return max(float(t.max()) for t in tops)


def top2_gap(scores):
    srt = np.sort(scores, axis=1)
    return srt[:, -1] - srt[:, -2]


def start_batch(n, pre_steps=PRE_STEPS, seed=ENV_SEED):
    """The oracle's envs where BatchedGridworldEnv(LEVEL, n, seed=seed).step_random(pre_steps, auto_reset=True) leaves the product's."""
    from oracle import oracle as O

    batch = O.EnvBatch(LEVEL, n, seed=seed)
    if pre_steps:
        batch.rollout(pre_steps, seed=seed, auto_reset=True)
    return batch


def act_inputs(n, seed=ENV_SEED):
    """(prev int8 [n, cells], cur int8 [n, cells]) of the acting cases: the boards after PRE_STEPS and PRE_STEPS + 1 random steps;
    the odd envs are "fresh" (previous = current), the even ones have stepped."""
    prev = start_batch(n, PRE_STEPS, seed).export()[0]
    cur = start_batch(n, PRE_STEPS + 1, seed).export()[0]
    prev = prev.copy()
    prev[1::2] = cur[1::2]
    return prev, cur


def emulate_rollout(w, n, n_steps, auto_reset, mask_finished=False, pre_steps=PRE_STEPS, prev=None, batch=None, metrics=None,
                    t_begin=None):
    """The fused rollout, greedy, on the CPU. prev None: fresh (previous := current at entry), else the previous boards int8 [n, cells];
    `batch` / `metrics`: continue a run (two launches). Returns a dict: states / prev_states int8 [T, n, cells] (zeros for an env whose
    episode is over when mask_finished), actions uint8 [T, n], recs int8 [T, n, 4], prev_boards (what the launch leaves in the
    caller's array), boards and fields (the oracle's export at the end), metrics, batch, and for the CPU suite gap [T, n] (top two
    scores), actions_cc [T, n] (the same weights fed [current, current]) and behind_reset bool [T, n] (the env was reset by the step
    before: its observation is [board, board]), stale_prev int8 [T, n, cells] (channel 0 had the reset not been honoured)."""
    from oracle import oracle as O

    batch = batch if batch is not None else start_batch(n, pre_steps)
    metrics = metrics if metrics is not None else O.metrics_new()
    t0 = pre_steps if t_begin is None else t_begin
    cur = batch.export()[0]
    fresh = np.ones(n, dtype=bool) if prev is None else np.zeros(n, dtype=bool)
    prev = cur.copy() if prev is None else np.asarray(prev, dtype=np.int8).copy()
    out = {k: [] for k in ("states", "prev_states", "actions", "recs", "gap", "actions_cc", "behind_reset", "stale_prev")}
    behind = np.zeros(n, dtype=bool)
    for k in range(n_steps):
        over = batch.export(boards=False)[1]["game_over"].astype(bool) & bool(mask_finished)
        stale = prev.copy()
        p = np.where(fresh[:, None], cur, prev)
        s = forward(p, cur, w)
        a = s.argmax(1).astype(np.uint8)  # the first maximum
        out["gap"].append(top2_gap(s))
        out["actions_cc"].append(forward(cur, cur, w).argmax(1).astype(np.uint8))
        out["behind_reset"].append(behind.copy())
        out["stale_prev"].append(stale)
        out["states"].append(np.where(over[:, None], 0, cur).astype(np.int8))
        out["prev_states"].append(np.where(over[:, None], 0, p).astype(np.int8))
        out["actions"].append(np.where(over, 0, a).astype(np.uint8))
        frame_before = batch.export(boards=False)[1]["frame"].copy()
        rec = batch.rollout(1, seed=ENV_SEED, t_begin=t0 + k, auto_reset=auto_reset, actions=a[None], metrics=metrics)
        out["recs"].append(rec.copy())
        prev = cur  # current -> previous, idle envs included
        cur, f = batch.export()
        behind = bool(auto_reset) & (rec[:, 2] != 0) & (f["game_over"] == 0) & (f["frame"] == 0) & (frame_before > 0)
        fresh = behind.copy()
    res = {k: np.stack(v) for k, v in out.items()}
    res["prev_boards"] = np.where(fresh[:, None], cur, prev).astype(np.int8)
    res["boards"], res["fields"] = batch.export()
    res["metrics"], res["batch"] = metrics, batch
    return res


def rollout_weights(channels):
    return weights("integer", channels, ROLLOUT_SEEDS[channels])


@functools.lru_cache(maxsize=None)
def emulated(channels, n, n_steps, auto_reset, mask_finished):
    """emulate_rollout of the rollout tests' weights from the fresh start, once per process and left unchanged."""
    return emulate_rollout(rollout_weights(channels), n, n_steps, auto_reset, mask_finished)


def rollout_conditions(res):
    """What a seed of ROLLOUT_SEEDS is chosen for, of one emulated auto-reset run: (smallest top-two gap, actions taken, share of
    (env, step) pairs whose decision differs from the one on [current, current], envs with a step behind an auto-reset whose
    observation differs from [the old episode's last board, board])."""
    differs = (res["actions"] != res["actions_cc"]).mean()
    b = res["behind_reset"]
    shows = b & (res["stale_prev"] != res["prev_states"]).any(2)
    return float(res["gap"].min()), int((np.bincount(res["actions"].reshape(-1), minlength=4) > 0).sum()), float(differs), int(shows.any(0).sum())


def seed_ok(channels, seed, n=N):
    w = weights("integer", channels, seed)
    long = emulate_rollout(w, n, 103, True)
    gap, taken, differs, shown = rollout_conditions(long)
    if not (gap >= 1.0 and taken >= 2 and differs >= 0.25 and shown == n):
        return False
    short = emulate_rollout(w, n, 12, False)
    return rollout_conditions(short)[0] >= 1.0 and float(emulate_rollout(w, n, 103, False, True)["gap"].min()) >= 1.0


if __name__ == "__main__":
    print({c: next(8200 + 1000 * j + c for j in range(1000) if seed_ok(c, 8200 + 1000 * j + c)) for c in CHANNELS})
