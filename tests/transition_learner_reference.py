"""Float64 reference and seeded inputs for the two-board conv learner (sgk_ppo_cnn_epochs_trans), shared by
tests/test_transition_learner_cpu.py and tests/test_gpu_transition_learn.py. tests/learner_reference.py's recipe for the one-board
learner with a second input plane; its trunk, heads, Adam, error measure, bound and cap are used as they are (cnn_trunk, cnn_head,
adam64, rel_err, bound, CAP): nothing here restates them, and nothing here calls the product's learner code.

  trans_epoch64   one epoch of PPOCNNAgent on observations [B, 2, H, W] (previous board, board): the three logged scalars, the gradients
                  of the 14 tensors (w1 [C, 2, 3, 3], wb [C, 2, 1, 1]), the ratios, values and normalised advantages.
  trans_inputs    the synthetic rollout of 3 steps x 37 trajectories on BoatRace's 5 x 5 board: `states` AND `prev_states` hold seeded
                  integers 0..5 in every cell, drawn independently (a swapped, dropped or duplicated plane changes w1's and wb's
                  gradients), the old policy at default initialisation, the current network perturbed by CNN_PERTURB; rows 0..7 of a
                  minibatch as in ppo_cnn_inputs (the four clamp branches, a row inside, the last row, row 0, a duplicate).
"""
import functools

import numpy as np
import torch

import learner_reference as R

ENV = "BoatRace-v0"
SHAPE = (5, 5)
T, N = R.CNN_T, R.CNN_N
TENSORS = R.CNN_TENSORS
STATS = ("policy_loss", "value_loss", "entropy")
Case = R.PpoCnnCase  # (env, channels, batch, seed, variant): ppo_cnn_hyper, cnn_stat_pair and cnn_case_id apply as they are

# seeds replaced because torch-float32's own error on one quantity was above CAP / 8 = 1.25e-6 with the first draw (that err_t in the
# comment); tests/test_transition_learner_cpu.py asks for inputs below it
RESEED = {
    (4, 64, "clip"): 4020,      # policy_loss 1.13e-05
    (8, 64, "clip"): 4022,      # policy_loss 2.19e-06
    (8, 37, "defaults"): 4025,  # (not an error figure: only one of the 111 ratios lay below 1 - clipping - 5 RATIO_MARGIN; two are needed)
}


def _cases():
    out = []

    def add(channels, batch, variant="clip"):
        out.append(Case(ENV, channels, batch, 4000 + len(out), variant))

    for channels in R.CNN_CHANNELS:
        add(channels, 64)
    add(5, 2)
    add(5, 37)
    add(8, 37, "defaults")
    add(4, 64, "tie")
    return [c._replace(seed=RESEED.get((c.channels, c.batch, c.variant), c.seed)) for c in out]


CASES = _cases()
PLUMBING_CASES = [c for c in CASES if c.batch == 37]  # C = 5 and C = 8, both under a full minibatch of 37


def case_id(c):
    return "trans-" + R.cnn_case_id(c)


def loss_kw(case):
    h = R.ppo_cnn_hyper(case)
    return {k: h[k] for k in ("clipping", "critic_coeff", "entropy_bonus")}


def param_shapes(channels, cells=SHAPE[0] * SHAPE[1]):
    C = channels
    return [(C, 2, 3, 3), (C,), (C, C, 3, 3), (C,), (C, 2, 1, 1), (C,), (C, C, 3, 3), (C,), (4, C * cells), (4,), (C, C, 3, 3), (C,),
            (1, C * cells), (1,)]


def _init(rng, channels):
    """torch's default Conv2d / Linear initialisation for the two-channel PPOCNNAgent's 14 tensors (weights U(-k, k), k = 1 /
    sqrt(fan_in)), the biases from U(-0.3, 0.3) instead (a dropped bias must show), and k per tensor: learner_reference._cnn_init's
    recipe with fan-ins 18 and 2 for conv1 and the bottleneck."""
    params, bounds = [], []
    shapes = param_shapes(channels)
    for w, b in zip(shapes[0::2], shapes[1::2]):
        k = 1.0 / np.sqrt(float(np.prod(w[1:])))
        params += [rng.uniform(-k, k, w).astype(np.float32), rng.uniform(-0.3, 0.3, b).astype(np.float32)]
        bounds += [k, 0.3]
    return params, bounds


def gather(d, rows):
    """Observations [B, 2, H, W] (previous board first), actions and returns of the flat rollout rows t * N + trajectory."""
    rows = np.asarray(rows)
    t, n = rows // N, rows % N
    obs = np.stack((d["prev_states"][t, n], d["states"][t, n]), axis=1).reshape((len(rows), 2) + SHAPE)
    return obs, d["actions"][t, n], d["returns"][n, t]


def trans_epoch64(params, old_params, obs, actions, returns, clipping, critic_coeff, entropy_bonus, dtype=torch.float64):
    """learner_reference.ppo_cnn_epoch64 on observations [B, 2, H, W]: the same surrogate loss on the same trunk and heads."""
    cast = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)  # noqa: E731
    p = [cast(x).requires_grad_(True) for x in params]
    o = [cast(x) for x in old_params]
    x, r = cast(obs), cast(returns)
    assert x.dim() == 4 and x.shape[1] == 2, tuple(x.shape)
    a = torch.as_tensor(np.asarray(actions, dtype=np.int64)).unsqueeze(1)

    tr = R.cnn_trunk(x, p)
    logp_all = torch.log_softmax(R.cnn_head(tr, *p[6:10]), dim=-1)
    values = R.cnn_head(tr, *p[10:14]).reshape(-1)
    advantage = r - values
    advantage = (advantage - advantage.mean()) / advantage.std()
    with torch.no_grad():
        old_logp = torch.log_softmax(R.cnn_head(R.cnn_trunk(x, o), *o[6:10]), dim=-1).gather(1, a).squeeze(1)
    ratio = torch.exp(logp_all.gather(1, a).squeeze(1) - old_logp)
    entropy = -(logp_all.exp() * logp_all).sum(-1).mean()
    value_loss = ((values - r) ** 2).mean()
    policy_loss = -torch.min(advantage * ratio, advantage * ratio.clamp(1 - clipping, 1 + clipping)).mean()
    loss = policy_loss + critic_coeff * value_loss - entropy_bonus * entropy
    grads = torch.autograd.grad(loss, p)
    return {"stats": [float(policy_loss.detach()), float(value_loss.detach()), float(entropy.detach())], "grads": [g.double().numpy() for g in grads],
            "ratio": ratio.detach().double().numpy(), "values": values.detach().double().numpy(),
            "advantage": advantage.detach().double().numpy()}


def row_conditions(case, d):
    """learner_reference.ppo_cnn_row_conditions for the two-plane inputs, evaluated in float64: named booleans, all of which must be True."""
    h = R.ppo_cnn_hyper(case)
    lo, hi = 1 - h["clipping"], 1 + h["clipping"]
    rows, n = d["rows"], T * N
    r64 = trans_epoch64(d["cur"], d["old"][:10], *gather(d, rows), **loss_kw(case))
    ratio, adv = r64["ratio"], r64["advantage"]
    above, below = ratio >= hi + R.RATIO_MARGIN, ratio <= lo - R.RATIO_MARGIN
    inside = (ratio >= lo + R.RATIO_MARGIN) & (ratio <= hi - R.RATIO_MARGIN)
    pos, neg = adv >= R.ADV_MARGIN, adv <= -R.ADV_MARGIN
    out = {"rows in the rollout": bool((rows >= 0).all() and (rows < n).all()), "batch": len(rows) == case.batch,
           "the planes differ": bool((d["prev_states"] != d["states"]).mean() > 0.5)}
    if case.variant == "tie":
        out["old == current"] = all((a == b).all() for a, b in zip(d["cur"], d["old"])) and bool((ratio == 1.0).all())
    elif case.batch == 2:
        out["one row outside"] = bool((above | below)[0])
        out["one row inside"] = bool(inside[1])
        out["two different rows"] = rows[0] != rows[1] and not (gather(d, rows[:1])[0] == gather(d, rows[1:])[0]).all()
    if case.batch >= 8:
        if case.variant != "tie":
            out["above, positive advantage"] = bool(above[0] and pos[0])
            out["above, negative advantage"] = bool(above[1] and neg[1])
            out["below, positive advantage"] = bool(below[2] and pos[2])
            out["below, negative advantage"] = bool(below[3] and neg[3])
            out["inside"] = bool(inside[4] and (pos | neg)[4])
        out["last row"] = rows[5] == n - 1
        out["row 0"] = rows[6] == 0
        out["a duplicate"] = rows[7] == rows[1]
    return out


def trans_inputs(case):
    """learner_reference.ppo_cnn_inputs with a second plane: "prev_states" beside "states", drawn independently of it; "rows2" (a second
    minibatch) and "ragged_lengths" (a seeded mix of 0..3 with a 0 in it) as there."""
    assert case.env == ENV
    rng = np.random.default_rng(case.seed)
    C, n, cells = case.channels, T * N, SHAPE[0] * SHAPE[1]
    d = {"shape": SHAPE, "states": rng.integers(0, 6, (T, N, cells)).astype(np.int8),
         "prev_states": rng.integers(0, 6, (T, N, cells)).astype(np.int8),
         "actions": rng.integers(0, 4, (T, N)).astype(np.uint8),
         "returns": rng.uniform(-5.0, 5.0, (N, T)).astype(np.float32),
         "lengths": np.full((N,), T, dtype=np.int32)}
    old, bounds = _init(rng, C)
    noise = [rng.standard_normal(p.shape).astype(np.float32) for p in old]
    d["old"] = old
    if case.variant == "tie":
        d["cur"] = [p.copy() for p in old]
    else:
        d["cur"] = [(p + np.float32(R.CNN_PERTURB * k) * z).astype(np.float32) for p, k, z in zip(old, bounds, noise)]
    rows = rng.integers(0, n, case.batch)
    d["rows2"] = rng.integers(0, n, case.batch).astype(np.int64)
    lengths = rng.integers(0, T + 1, N).astype(np.int32)
    lengths[case.seed % N] = 0
    d["ragged_lengths"] = lengths
    assert 3 * int(lengths.sum()) >= n and set(lengths.tolist()) == {0, 1, 2, 3}
    if case.variant != "tie":
        obs, actions, _ = gather(d, np.arange(n))
        full = trans_epoch64(d["cur"], old[:10], obs, actions, np.zeros(n), **loss_kw(case))
        ratio, values = full["ratio"], full["values"]  # (neither depends on the returns)
        h = R.ppo_cnn_hyper(case)
        lo, hi = 1 - h["clipping"], 1 + h["clipping"]
        above, below = np.flatnonzero(ratio >= hi + 5 * R.RATIO_MARGIN), np.flatnonzero(ratio <= lo - 5 * R.RATIO_MARGIN)
        inside = np.flatnonzero((ratio >= lo + 5 * R.RATIO_MARGIN) & (ratio <= hi - 5 * R.RATIO_MARGIN))
        assert len(above) >= 2 and len(below) >= 2 and len(inside) >= 1, (case, len(above), len(below), len(inside))
        if case.batch == 2:
            rows[:] = [(above if case.seed % 2 else below)[0], inside[0]]
        else:
            rows[:5] = [above[0], above[1], below[0], below[1], inside[0]]
            for row, sign in zip(rows[:4], (4.0, -4.0, 4.0, -4.0)):
                d["returns"][row % N, row // N] = np.float32(values[row] + sign)
    if case.batch >= 8:
        rows[5:8] = [n - 1, 0, rows[1]]
    d["rows"] = rows.astype(np.int64)
    bad = [k for k, ok in row_conditions(case, d).items() if not ok]
    assert not bad, (case, bad)
    return d


@functools.lru_cache(maxsize=None)
def yardstick(case):
    """(inputs, float64 reference, err_t per tensor and per scalar: the same function in float32) of a case; once per process."""
    d = trans_inputs(case)
    args, kw = (d["cur"], d["old"][:10]) + gather(d, d["rows"]), loss_kw(case)
    r64, r32 = trans_epoch64(*args, **kw), trans_epoch64(*args, dtype=torch.float32, **kw)
    err_t = {k: R.rel_err(a, b) for k, a, b in zip(TENSORS, r32["grads"], r64["grads"])}
    for i, k in enumerate(STATS):
        err_t[k] = R.cnn_stat_err(case, r64, i, r32["stats"][i])
    return d, r64, err_t


def workspace_bytes(channels, batch):
    """include/sgk.h's formula for sgk_ppo_cnn_trans_workspace_bytes: 4 (1088 + batch (5 C 25 + P2)), P2 = P + 10 C, P = 27 C^2 + 140 C + 5."""
    C = int(channels)
    return 4 * (1088 + int(batch) * (5 * C * 25 + 27 * C * C + 140 * C + 5 + 10 * C))
