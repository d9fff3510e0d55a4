"""Float64 references for the fused learners (sgk_dqn_sgd_step, sgk_ppo_epochs, sgk_ppo_cnn_epochs), on the CPU, and the seeded inputs
that tests/test_learner_reference_cpu.py, tests/test_gpu_learner_gradients.py and tests/test_gpu_ppo_cnn_gradients.py share. Plain
torch on .double() tensors with autograd (or on .float() ones: the float32 yardstick); nothing here calls the product's learner code.

  dqn_step64    DeepQAgent.learn's loss and gradients (value.py:113-136): target y = discount * max target_Q(s') * (1 - terminal) +
                float32(reward * reward_scale), mse_loss over the [B,1]-vs-[B] broadcast (the default) or per sample, the gradients of
                the six tensors, their total norm and clip_grad_norm_'s coef = min(max_norm / (norm + 1e-6), 1).
  ppo_epoch64   one epoch of PPOBaseAgent (ppo.py's surrogate_loss): minibatch-normalised advantages (unbiased std), the ratio against
                the old policy clipped to 1 +- clipping, critic_coeff x the critic's MSE, entropy_bonus x the entropy; the three logged
                scalars and the gradients of the eight tensors.
  ppo_cnn_epoch64  the same epoch for PPOCNNAgent's body (ppo.py: conv3x3 1 -> C, conv3x3 C -> C, the 1x1 bottleneck on the board added to
                the trunk, conv3x3 + linear actor and critic heads): the three scalars, the gradients of the 14 tensors, the ratios.
  adam64        one element-wise Adam step with torch's formulas (the comment above adam_scalar in csrc/sgk_learn.hip), amsgrad when
                a vmax is given. lr, beta1, beta2 and eps are taken as the float32 values the kernels receive; 1 - beta is then exact
                in float32 (Sterbenz), so (1 - beta1) here is the kernel's own factor.
  ppo_chain64   n epochs of ppo_epoch64 + adam64 in a row, as one sgk_ppo_epochs launch of n epochs runs them (the yardstick: the
                epochs in float32 with torch.optim.Adam itself; stale=True: the emulation of a launch whose epochs read the previous
                update too early), with the seeded rows, Adam state and ragged / sparse rollouts (ppo_ragged_inputs) of
                tests/test_gpu_ppo_epoch_chain.py.

The discount is taken as its float32 value as well: torch's float32 run and the kernel both multiply by float32(discount).
"""
import collections
import functools

import numpy as np
import torch

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
MAX_NORM = 10.0
N_ENVS, SLICES = 64, 2            # the replay ring / the rollout the cases draw from: SLICES x N_ENVS transitions
ULP = 2.0 ** -23
CAP = 1e-5                        # x max|g|: the cap tests/test_gpu_ppo_cnn_learn.py::test_fused_cnn_learner_gradients uses

ENV_CELLS = collections.OrderedDict([
    ("BoatRace-v0", 25), ("FriendFoe-v0", 30), ("SideEffectsSokoban-v0", 36), ("IslandNavigation-v0", 48), ("ConveyorBelt-v0", 49),
    ("SafeInterruptibility-v0", 56), ("DistributionalShift-v0", 63), ("TomatoWatering-v0", 63)])
REWARD_SCALE = {"TomatoWatering-v0": 0.02}  # what one unit of the int8 reward is worth (1 elsewhere)

DQN_LR, DQN_DISCOUNT = 1e-2, 0.9
PPO_HYPER = dict(lr=1e-3, clipping=0.1, critic_coeff=0.5, entropy_bonus=0.02)

DQN_TENSORS = ("w1", "b1", "w2", "b2", "w3", "b3")
PPO_TENSORS = ("w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc")

# rows: "mixed" = seeded rows with a duplicate, a terminal and a non-terminal transition; "terminal" / "nonterminal": the B = 1 forms
DqnCase = collections.namedtuple("DqnCase", "env hidden batch clipped broadcast rows seed wscale")
PpoCase = collections.namedtuple("PpoCase", "env hidden batch seed")


def _dqn_cases():
    out = []

    def add(env, hidden, batch, clipped=True, broadcast=True, wscale=None):
        env = env + "-v0"
        for rows in (("terminal", "nonterminal") if batch == 1 else ("mixed",)):
            c = DqnCase(env, hidden, batch, clipped, broadcast, rows, 1000 + len(out), wscale if wscale is not None else (2.0 if clipped else 0.25))
            if not any(c[:6] == o[:6] for o in out):
                out.append(c)

    for env in ENV_CELLS:
        for hidden in (64, 100):
            add(env[:-3], hidden, 64)
    for batch in (1, 17):
        add("BoatRace", 100, batch)
        add("SafeInterruptibility", 64, batch)
    add("IslandNavigation", 100, 64, clipped=False)
    add("DistributionalShift", 64, 64, clipped=False)
    add("SideEffectsSokoban", 100, 64, broadcast=False)
    add("IslandNavigation", 64, 17)
    add("IslandNavigation", 64, 17, broadcast=False)
    # the cases for the in-kernel Adam of SGK_DQN_ONE_LAUNCH=1 (CHILD_CASES below: that form needs a process of its own)
    add("SideEffectsSokoban", 64, 17)
    add("DistributionalShift", 100, 1)
    return out


DQN_CASES = _dqn_cases()
CHILD_KEYS = (("BoatRace-v0", 100, 64), ("SideEffectsSokoban-v0", 64, 17), ("SafeInterruptibility-v0", 100, 64), ("DistributionalShift-v0", 100, 1))
CHILD_CASES = [c for c in DQN_CASES if c[:3] in CHILD_KEYS and c.clipped and c.broadcast]
RESET_STORE_CASE = next(c for c in DQN_CASES if c[:3] == ("SideEffectsSokoban-v0", 100, 64) and c.broadcast)


def _ppo_cases():
    out = []
    for env in list(ENV_CELLS)[:7]:  # the seven distinct K0
        for hidden in (64, 100):
            out.append(PpoCase(env, hidden, 64, 2000 + len(out)))
    for env, hidden in (("SafeInterruptibility-v0", 64), ("BoatRace-v0", 100)):
        for batch in (2, 33):
            out.append(PpoCase(env, hidden, batch, 2000 + len(out)))
    # three seeds replaced: with the first draw torch-float32's own error on the policy loss (a sum that nearly cancels) or on the critic
    # bias's one-element gradient was above 1e-5 / 8 (2.3e-6 to 4.0e-6): tests/test_learner_reference_cpu.py asks for inputs below it
    reseed = {("BoatRace-v0", 64, 64): 2200, ("ConveyorBelt-v0", 100, 64): 2209, ("SafeInterruptibility-v0", 64, 33): 2215}
    return [c._replace(seed=reseed.get(c[:3], c.seed)) for c in out]


PPO_CASES = _ppo_cases()


def case_id(c):
    if isinstance(c, PpoCase):
        return "%s-h%d-b%d" % (c.env[:-3], c.hidden, c.batch)
    return "%s-h%d-b%d-%s-%s%s" % (c.env[:-3], c.hidden, c.batch, "clipped" if c.clipped else "unclipped",
                                    "broadcast" if c.broadcast else "persample", "" if c.rows == "mixed" else "-" + c.rows)


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------
def _linear(rng, n_out, n_in):
    """torch.nn.Linear's default initialisation: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias."""
    k = 1.0 / np.sqrt(n_in)
    return [rng.uniform(-k, k, (n_out, n_in)).astype(np.float32), rng.uniform(-k, k, (n_out,)).astype(np.float32)]


def dqn_inputs(case):
    """The replay tensors [SLICES, N_ENVS, ...], both networks' parameters (float32) and the minibatch rows of a DQN case."""
    rng = np.random.default_rng(case.seed)
    k0, h, n = ENV_CELLS[case.env], case.hidden, SLICES * N_ENVS
    d = {"states": rng.integers(0, 6, (SLICES, N_ENVS, k0)).astype(np.int8),
         "successors": rng.integers(0, 6, (SLICES, N_ENVS, k0)).astype(np.int8),
         "actions": rng.integers(0, 4, (SLICES, N_ENVS)).astype(np.uint8),
         "terminals": rng.random((SLICES, N_ENVS)) < 0.3}
    d["rewards"] = (rng.integers(-50, 51, (SLICES, N_ENVS)) if case.clipped else rng.integers(-1, 2, (SLICES, N_ENVS))).astype(np.int8)
    q = _linear(rng, h, k0) + _linear(rng, h, h) + _linear(rng, 4, h)
    t = _linear(rng, h, k0) + _linear(rng, h, h) + _linear(rng, 4, h)
    d["q"] = [(p * np.float32(case.wscale)).astype(np.float32) for p in q]  # the Q-network away from the target network, as in
    d["t"] = [(p + np.float32(0.05) * rng.standard_normal(p.shape).astype(np.float32)).astype(np.float32) for p in t]  # test_gpu_deepq.py
    term = d["terminals"].reshape(-1)
    if case.rows == "mixed":
        rows = rng.integers(0, n, case.batch)
        rows[1] = rows[0]                                 # a duplicate
        rows[2] = np.flatnonzero(term)[case.seed % 7]     # a terminal transition
        rows[3] = np.flatnonzero(~term)[case.seed % 11]   # a non-terminal one
    else:
        rows = np.array([np.flatnonzero(term if case.rows == "terminal" else ~term)[case.seed % 5]])
    d["rows"] = rows.astype(np.int64)
    assert case.batch == 1 or (len(set(rows.tolist())) < case.batch and term[rows].any() and not term[rows].all())
    d["reward_scale"] = REWARD_SCALE.get(case.env, 1.0)
    return d


def ppo_inputs(case):
    """A full rollout [T = SLICES, N = N_ENVS] (every pair valid), the current network (perturbed away from the old policy so that
    ratios leave the clip range) and the old policy, float32, and the minibatch rows t * N + env: row 0 has a ratio outside the clip
    range and row 1 one inside it (both branches of the clamp's gradient), rows 2 and 3 are equal where the batch has room."""
    rng = np.random.default_rng(case.seed)
    k0, h, n = ENV_CELLS[case.env], case.hidden, SLICES * N_ENVS
    d = {"states": rng.integers(0, 6, (SLICES, N_ENVS, k0)).astype(np.int8),
         "actions": rng.integers(0, 4, (SLICES, N_ENVS)).astype(np.uint8),
         "returns": rng.uniform(-5.0, 5.0, (N_ENVS, SLICES)).astype(np.float32),
         "lengths": np.full((N_ENVS,), SLICES, dtype=np.int32)}
    old = _linear(rng, h, k0) + _linear(rng, h, h) + _linear(rng, 4, h) + _linear(rng, 1, h)
    d["old"] = old
    d["cur"] = [(p + np.float32(0.05) * rng.standard_normal(p.shape).astype(np.float32)).astype(np.float32) for p in old]
    s, a, _ = ppo_gather(d, np.arange(n))
    ratio = ppo_epoch64(d["cur"], d["old"][:6], s, a, np.zeros(n), **_ppo_loss_kw())["ratio"]  # (the ratios do not depend on the returns)
    out = (ratio < 1 - PPO_HYPER["clipping"]) | (ratio > 1 + PPO_HYPER["clipping"])
    rows = rng.integers(0, n, case.batch)
    rows[0] = np.flatnonzero(out)[case.seed % 3]
    rows[1] = np.flatnonzero(~out)[case.seed % 3]
    if case.batch >= 4:  # (two equal rows of two would make the advantages' std 0)
        rows[3] = rows[2]
    d["rows"] = rows.astype(np.int64)
    return d


def _ppo_loss_kw():
    return {k: PPO_HYPER[k] for k in ("clipping", "critic_coeff", "entropy_bonus")}


def dqn_gather(d, rows):
    flat = lambda t: t.reshape((SLICES * N_ENVS,) + t.shape[2:])  # noqa: E731
    return tuple(flat(d[k])[rows] for k in ("states", "successors", "actions", "rewards", "terminals"))


def ppo_gather(d, rows):
    t, n = rows // N_ENVS, rows % N_ENVS
    return d["states"][t, n], d["actions"][t, n], d["returns"][n, t]


# ---- the references ------------------------------------------------------------------------------------------------------------------
def _mlp(x, w1, b1, w2, b2):
    return torch.relu(torch.relu(x @ w1.t() + b1) @ w2.t() + b2)


def dqn_step64(q_params, t_params, states, successors, actions, rewards, terminals, discount, reward_scale, broadcast=True,
               max_norm=MAX_NORM, dtype=torch.float64):
    """Loss, gradients, total norm and clip coefficient of one DeepQAgent.learn on the given minibatch (arrays of B rows)."""
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)  # noqa: E731
    q = [T(p).requires_grad_(True) for p in q_params]
    t = [T(p) for p in t_params]
    s, s2 = T(np.asarray(states).reshape(len(actions), -1)), T(np.asarray(successors).reshape(len(actions), -1))
    act = torch.as_tensor(np.asarray(actions, dtype=np.int64))
    qs = (_mlp(s, *q[:4]) @ q[4].t() + q[5]).gather(1, act.unsqueeze(1))  # [B, 1], as value.py:119
    with torch.no_grad():
        nq = (_mlp(s2, *t[:4]) @ t[4].t() + t[5]).max(1)[0]
        nq = nq * T(1.0 - np.asarray(terminals, dtype=np.float64))
        r = T((np.asarray(rewards, dtype=np.float64) * float(reward_scale)).astype(np.float32))
        y = float(np.float32(discount)) * nq + r
    diff = (qs - y.unsqueeze(0)) if broadcast else (qs.squeeze(1) - y)  # [B, B] (Qs [B,1] against expected_Qs [B]) or [B]
    loss = (diff * diff).mean()
    grads = torch.autograd.grad(loss, q)
    norm = torch.sqrt(sum((g * g).sum() for g in grads))
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return {"loss": float(loss.detach()), "grads": [g.double().numpy() for g in grads], "norm": float(norm.detach()), "coef": float(coef.detach()),
            "clipped_grads": [(g * coef.detach()).double().numpy() for g in grads]}


def ppo_epoch64(params, old_params, states, actions, returns, clipping, critic_coeff, entropy_bonus, dtype=torch.float64):
    """The three logged scalars (policy loss, value loss, entropy) and the gradients of the eight tensors for one minibatch."""
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)  # noqa: E731
    p = [T(x).requires_grad_(True) for x in params]
    o = [T(x) for x in old_params]
    s, r = T(np.asarray(states).reshape(len(actions), -1)), T(returns)
    a = torch.as_tensor(np.asarray(actions, dtype=np.int64)).unsqueeze(1)
    trunk = _mlp(s, *p[:4])
    logp_all = torch.log_softmax(trunk @ p[4].t() + p[5], dim=-1)
    values = (trunk @ p[6].t() + p[7]).reshape(-1)
    advantage = r - values
    advantage = (advantage - advantage.mean()) / advantage.std()
    with torch.no_grad():
        old_logp = torch.log_softmax(_mlp(s, *o[:4]) @ o[4].t() + o[5], dim=-1).gather(1, a).squeeze(1)
    ratio = torch.exp(logp_all.gather(1, a).squeeze(1) - old_logp)
    entropy = -(logp_all.exp() * logp_all).sum(-1).mean()
    value_loss = ((values - r) ** 2).mean()
    policy_loss = -torch.min(advantage * ratio, advantage * ratio.clamp(1 - clipping, 1 + clipping)).mean()
    loss = policy_loss + critic_coeff * value_loss - entropy_bonus * entropy
    grads = torch.autograd.grad(loss, p)
    return {"stats": [float(policy_loss.detach()), float(value_loss.detach()), float(entropy.detach())], "grads": [g.double().numpy() for g in grads],
            "ratio": ratio.detach().double().numpy()}


def adam64(w, m, v, vmax, g, step, lr, beta1=BETA1, beta2=BETA2, eps=EPS):
    """Adam step number `step` (1-based) in float64: returns (w', m', v', vmax'); vmax None = no amsgrad (vmax' None)."""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, beta1, beta2, eps))
    w, m, v, g = (np.asarray(x, dtype=np.float64) for x in (w, m, v, g))
    m2 = m + (1.0 - b1) * (g - m)
    v2 = b2 * v + (1.0 - b2) * g * g
    x2 = None if vmax is None else np.maximum(np.asarray(vmax, dtype=np.float64), v2)
    denom = np.sqrt(v2 if x2 is None else x2) / np.sqrt(1.0 - b2 ** step) + eps
    return w - lr / (1.0 - b1 ** step) * m2 / denom, m2, v2, x2


def one_minus_beta1():
    return float(np.float32(1.0) - np.float32(BETA1))


def one_minus_beta2():
    return float(np.float32(1.0) - np.float32(BETA2))


# ---- the float32 yardstick -----------------------------------------------------------------------------------------------------------
def rel_err(got, want):
    """max|got - want| / max|want|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def bound(err_t):
    """What a kernel's err_k may be: 8 x torch-float32's own error (both are fp32 sums of the same terms, in other orders and chunk
    sizes), at least 16 ulp, and never above the cap."""
    return min(max(8.0 * err_t, 16.0 * ULP), CAP)


@functools.lru_cache(maxsize=None)
def dqn_yardstick(case):
    """(inputs, float64 reference, err_t per compared quantity) of a DQN case; computed once per process."""
    d = dqn_inputs(case)
    args = (d["q"], d["t"]) + dqn_gather(d, d["rows"]) + (DQN_DISCOUNT, d["reward_scale"], case.broadcast)
    r64, r32 = dqn_step64(*args), dqn_step64(*args, dtype=torch.float32)
    err_t = {k: rel_err(a, b) for k, a, b in zip(DQN_TENSORS, r32["clipped_grads"], r64["clipped_grads"])}
    err_t["loss"] = rel_err(r32["loss"], r64["loss"])
    return d, r64, err_t


@functools.lru_cache(maxsize=None)
def ppo_yardstick(case):
    d = ppo_inputs(case)
    args = (d["cur"], d["old"][:6]) + ppo_gather(d, d["rows"])
    r64, r32 = ppo_epoch64(*args, **_ppo_loss_kw()), ppo_epoch64(*args, dtype=torch.float32, **_ppo_loss_kw())
    err_t = {k: rel_err(a, b) for k, a, b in zip(PPO_TENSORS, r32["grads"], r64["grads"])}
    for i, k in enumerate(("policy_loss", "value_loss", "entropy")):
        err_t[k] = rel_err(r32["stats"][i], r64["stats"][i])
    return d, r64, err_t


def inject_adam_state(g_c, seed, amsgrad):
    """Seeded Adam state around the kernel's own clipped gradient g_c (float64 arrays, one per tensor): m ~ N(0, max|g_c|), v = u g_c^2
    with u log-uniform in [1e-3, 1e3], vmax = v x {0.5, 2} alternating from a seeded offset (both in every tensor of two or more
    elements). Where g_c is exactly 0 (a unit dead on the whole minibatch; three of b3's four elements at batch 1) v = u max|g_c|^2
    instead of 0: with v = vmax = 0 the maximum would be no choice. All float32."""
    rng = np.random.default_rng(seed)
    ms, vs, xs = [], [], []
    for g in g_c:
        top = np.abs(g).max()
        u = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), g.shape))
        v = (u * np.where(g == 0.0, top, g) ** 2).astype(np.float32)
        half = ((np.arange(g.size) + int(rng.integers(0, 2))) % 2 == 0).reshape(g.shape)
        ms.append((rng.standard_normal(g.shape) * top).astype(np.float32))
        vs.append(v)
        xs.append((v * np.where(half, np.float32(0.5), np.float32(2.0))).astype(np.float32))
    return (ms, vs, xs) if amsgrad else (ms, vs, None)


# ---- the conv body: sgk_ppo_cnn_epochs (csrc/sgk_ppo_cnn.hip) ------------------------------------------------------------------------
# one level per board shape the kernels are instantiated for (height, width); x CNN_CHANNELS = the 21 instantiations
CNN_SHAPES = collections.OrderedDict([
    ("BoatRace-v0", (5, 5)), ("FriendFoe-v0", (6, 5)), ("SideEffectsSokoban-v0", (6, 6)), ("IslandNavigation-v0", (6, 8)),
    ("ConveyorBelt-v0", (7, 7)), ("SafeInterruptibility-v0", (7, 8)), ("DistributionalShift-v0", (7, 9))])
CNN_CHANNELS = (4, 5, 8)
CNN_T, CNN_N = 3, 37              # the synthetic rollout: a short horizon and an odd number of trajectories
# PPOCNNAgent's parameters in registration order (BatchedPPOAgent.CNN_PARAMS): conv1, conv2, the 1x1 bottleneck, the actor's conv and
# linear layer, the critic's conv and linear layer; the old policy's ten actor-path tensors are the first ten
CNN_TENSORS = ("w1", "b1", "w2", "b2", "wb", "bb", "wa", "ba", "la", "lab", "wv", "bv", "lv", "lvb")
CNN_DEFAULT_HYPER = dict(lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01)  # the agent's defaults (variant "defaults")
# The current network = the old one + CNN_PERTURB x (the tensor's initialisation bound) x N(0, 1), element by element. With 0.25 the
# log-ratios of the 111 rollout rows have a standard deviation of 0.11 to 0.48 over the cases and the ratios lie in 0.27 .. 2.2: at
# least two rows above 1 + clipping, two below 1 - clipping and one inside for both clippings (0.1, 0.2), which ppo_cnn_inputs asserts,
# and 31 to 57 of a minibatch's 64 rows outside the range (27 and 28 of 37 in the two batch-37 cases, 1 of 2 at batch 2).
CNN_PERTURB = 0.25
RATIO_MARGIN, ADV_MARGIN = 1e-3, 1e-2  # how far the branch rows stay from the clip bounds / from a zero advantage

# variant: "clip" = PPO_HYPER, current network perturbed; "defaults" = the same under CNN_DEFAULT_HYPER; "tie" = old == current
PpoCnnCase = collections.namedtuple("PpoCnnCase", "env channels batch seed variant")


def _ppo_cnn_cases():
    out = []

    def add(env, channels, batch, variant="clip"):
        out.append(PpoCnnCase(env + "-v0", channels, batch, 3000 + len(out), variant))

    for env in CNN_SHAPES:
        for channels in CNN_CHANNELS:
            add(env[:-3], channels, 64)
    add("SideEffectsSokoban", 8, 2)
    add("SafeInterruptibility", 5, 2)
    add("FriendFoe", 5, 37)
    add("DistributionalShift", 8, 37, "defaults")
    add("IslandNavigation", 4, 64, "tie")
    reseed = CNN_RESEED
    return [c._replace(seed=reseed.get((c.env, c.channels, c.batch, c.variant), c.seed)) for c in out]


# seeds replaced because torch-float32's own error on one quantity was above 1e-5 / 8 with the first draw (the measured 8 err_t in
# the comment); tests/test_learner_reference_cpu.py asks for inputs below it
CNN_RESEED = {
    ("SideEffectsSokoban-v0", 4, 64, "clip"): 3220,    # policy_loss 1.3e-05
    ("SideEffectsSokoban-v0", 8, 64, "clip"): 3260,    # policy_loss 1.7e-05
    ("ConveyorBelt-v0", 4, 64, "clip"): 3340,          # policy_loss 9.4e-05
    ("SafeInterruptibility-v0", 5, 64, "clip"): 3423,  # bb 1.0e-05
    ("SideEffectsSokoban-v0", 8, 2, "clip"): 3521,     # policy_loss 1.0e-05
    ("SafeInterruptibility-v0", 5, 2, "clip"): 3541,   # policy_loss 1.1e-04
    ("FriendFoe-v0", 5, 37, "clip"): 3560,             # lvb 3.3e-05
}
PPO_CNN_CASES = _ppo_cnn_cases()
# the cases of the epoch-plumbing and ragged-rollout tests: one with C = 5 and one with C = 8, both under a full minibatch of 37
PLUMBING_CASES = [c for c in PPO_CNN_CASES if c.batch == 37]


def cnn_case_id(c):
    return "%s-c%d-b%d%s" % (c.env[:-3], c.channels, c.batch, "" if c.variant == "clip" else "-" + c.variant)


def ppo_cnn_hyper(case):
    return dict(CNN_DEFAULT_HYPER if case.variant == "defaults" else PPO_HYPER)


def _loss_kw(hyper):
    return {k: hyper[k] for k in ("clipping", "critic_coeff", "entropy_bonus")}


def _cnn_init(rng, channels, cells):
    """torch's default Conv2d / Linear initialisation for PPOCNNAgent's 14 tensors (weights U(-k, k), k = 1 / sqrt(fan_in)), the biases
    from U(-0.3, 0.3) instead (a dropped bias must show), and k per tensor."""
    C = channels
    shapes = [(C, 1, 3, 3), (C, C, 3, 3), (C, 1, 1, 1), (C, C, 3, 3), (4, C * cells), (C, C, 3, 3), (1, C * cells)]
    params, bounds = [], []
    for shape in shapes:
        k = 1.0 / np.sqrt(float(np.prod(shape[1:])))
        params += [rng.uniform(-k, k, shape).astype(np.float32), rng.uniform(-0.3, 0.3, shape[:1]).astype(np.float32)]
        bounds += [k, 0.3]
    return params, bounds


def ppo_cnn_gather(d, rows):
    """Boards [B, H, W], actions and returns of the flat rollout rows t * N + trajectory."""
    rows = np.asarray(rows)
    t, n = rows // CNN_N, rows % CNN_N
    return d["states"][t, n].reshape((len(rows),) + d["shape"]), d["actions"][t, n], d["returns"][n, t]


def cnn_trunk(x, w):
    """PPOCNNAgent's trunk on boards x [B, 1, H, W]: relu(conv3x3(relu(conv3x3(x)))) + conv1x1(x); w = (w1, b1, w2, b2, wb, bb, ...)."""
    F = torch.nn.functional
    h = torch.relu(F.conv2d(x, w[0], w[1], padding=1))
    return torch.relu(F.conv2d(h, w[2], w[3], padding=1)) + F.conv2d(x, w[4], w[5])


def cnn_head(t, wc, bc, wl, bl):
    """One head on the trunk t: linear(flatten(relu(conv3x3(t)))). Shared with tests/forward_reference.py's cnn_forward."""
    return torch.relu(torch.nn.functional.conv2d(t, wc, bc, padding=1)).flatten(1) @ wl.t() + bl


def ppo_cnn_epoch64(params, old_params, boards, actions, returns, clipping, critic_coeff, entropy_bonus, dtype=torch.float64):
    """One epoch of PPOCNNAgent (ppo.py: PPOCNNAgent.forward + PPOBaseAgent.surrogate_loss) on a minibatch of boards [B, H, W]: the three
    logged scalars, the gradients of the 14 tensors in CNN_TENSORS order, the ratios and the critic's values."""
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)  # noqa: E731
    p = [T(x).requires_grad_(True) for x in params]
    o = [T(x) for x in old_params]
    x, r = T(boards).unsqueeze(1), T(returns)
    a = torch.as_tensor(np.asarray(actions, dtype=np.int64)).unsqueeze(1)

    tr = cnn_trunk(x, p)
    logp_all = torch.log_softmax(cnn_head(tr, *p[6:10]), dim=-1)
    values = cnn_head(tr, *p[10:14]).reshape(-1)
    advantage = r - values
    advantage = (advantage - advantage.mean()) / advantage.std()
    with torch.no_grad():
        old_logp = torch.log_softmax(cnn_head(cnn_trunk(x, o), *o[6:10]), dim=-1).gather(1, a).squeeze(1)
    ratio = torch.exp(logp_all.gather(1, a).squeeze(1) - old_logp)
    entropy = -(logp_all.exp() * logp_all).sum(-1).mean()
    value_loss = ((values - r) ** 2).mean()
    policy_loss = -torch.min(advantage * ratio, advantage * ratio.clamp(1 - clipping, 1 + clipping)).mean()
    loss = policy_loss + critic_coeff * value_loss - entropy_bonus * entropy
    grads = torch.autograd.grad(loss, p)
    return {"stats": [float(policy_loss.detach()), float(value_loss.detach()), float(entropy.detach())], "grads": [g.double().numpy() for g in grads],
            "ratio": ratio.detach().double().numpy(), "values": values.detach().double().numpy(),
            "advantage": advantage.detach().double().numpy()}


def ppo_cnn_row_conditions(case, d):
    """What the minibatch d["rows"] of a case holds, evaluated in float64: a dict of named booleans, all of which must be True."""
    h = ppo_cnn_hyper(case)
    lo, hi = 1 - h["clipping"], 1 + h["clipping"]
    rows, n = d["rows"], CNN_T * CNN_N
    r64 = ppo_cnn_epoch64(d["cur"], d["old"][:10], *ppo_cnn_gather(d, rows), **_loss_kw(h))
    ratio, adv = r64["ratio"], r64["advantage"]
    above, below = ratio >= hi + RATIO_MARGIN, ratio <= lo - RATIO_MARGIN
    inside = (ratio >= lo + RATIO_MARGIN) & (ratio <= hi - RATIO_MARGIN)
    pos, neg = adv >= ADV_MARGIN, adv <= -ADV_MARGIN
    out = {"rows in the rollout": bool((rows >= 0).all() and (rows < n).all()), "batch": len(rows) == case.batch}
    if case.variant == "tie":
        out["old == current"] = all((a == b).all() for a, b in zip(d["cur"], d["old"])) and bool((ratio == 1.0).all())
    elif case.batch == 2:
        out["one row outside"] = bool((above | below)[0])
        out["one row inside"] = bool(inside[1])
        out["two different rows"] = rows[0] != rows[1] and not (ppo_cnn_gather(d, rows[:1])[0] == ppo_cnn_gather(d, rows[1:])[0]).all()
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


def ppo_cnn_inputs(case):
    """The synthetic rollout [T = CNN_T, N = CNN_N] (boards of seeded integers 0..5 in every cell, the border ring included; every pair
    valid), the old policy and the current network (float32, CNN_TENSORS order) and the minibatch rows t * N + trajectory. At batch >= 8
    rows[0..7] are: ratio above 1 + clipping with a positive / a negative normalised advantage, below 1 - clipping with a positive / a
    negative one, a ratio inside the range, the last row T * N - 1, row 0, and rows[1] again; the first four rows' returns are set to
    the critic's value +- 4 for that sign. At batch 2: a row outside and a row inside. "tie": old == current (every ratio is 1).
    Also "rows2" (a second minibatch, for the two-epoch test) and "ragged_lengths" (a seeded mix of 0..3 with a 0 in it)."""
    rng = np.random.default_rng(case.seed)
    (H, W), C, n = CNN_SHAPES[case.env], case.channels, CNN_T * CNN_N
    h = ppo_cnn_hyper(case)
    d = {"shape": (H, W), "states": rng.integers(0, 6, (CNN_T, CNN_N, H * W)).astype(np.int8),
         "actions": rng.integers(0, 4, (CNN_T, CNN_N)).astype(np.uint8),
         "returns": rng.uniform(-5.0, 5.0, (CNN_N, CNN_T)).astype(np.float32),
         "lengths": np.full((CNN_N,), CNN_T, dtype=np.int32)}
    old, bounds = _cnn_init(rng, C, H * W)
    noise = [rng.standard_normal(p.shape).astype(np.float32) for p in old]
    d["old"] = old
    if case.variant == "tie":
        d["cur"] = [p.copy() for p in old]
    else:
        d["cur"] = [(p + np.float32(CNN_PERTURB * k) * z).astype(np.float32) for p, k, z in zip(old, bounds, noise)]
    rows = rng.integers(0, n, case.batch)
    d["rows2"] = rng.integers(0, n, case.batch).astype(np.int64)
    lengths = rng.integers(0, CNN_T + 1, CNN_N).astype(np.int32)
    lengths[case.seed % CNN_N] = 0
    d["ragged_lengths"] = lengths
    assert 3 * int(lengths.sum()) >= n and set(lengths.tolist()) == {0, 1, 2, 3}
    if case.variant != "tie":
        full = ppo_cnn_epoch64(d["cur"], old[:10], *ppo_cnn_gather(d, np.arange(n))[:2], np.zeros(n), **_loss_kw(h))
        ratio, values = full["ratio"], full["values"]  # (neither depends on the returns)
        lo, hi = 1 - h["clipping"], 1 + h["clipping"]
        above, below = np.flatnonzero(ratio >= hi + 5 * RATIO_MARGIN), np.flatnonzero(ratio <= lo - 5 * RATIO_MARGIN)
        inside = np.flatnonzero((ratio >= lo + 5 * RATIO_MARGIN) & (ratio <= hi - 5 * RATIO_MARGIN))
        assert len(above) >= 2 and len(below) >= 2 and len(inside) >= 1, (case, len(above), len(below), len(inside))
        if case.batch == 2:
            rows[:] = [(above if case.seed % 2 else below)[0], inside[0]]
        else:
            rows[:5] = [above[0], above[1], below[0], below[1], inside[0]]
            for row, sign in zip(rows[:4], (4.0, -4.0, 4.0, -4.0)):
                d["returns"][row % CNN_N, row // CNN_N] = np.float32(values[row] + sign)
    if case.batch >= 8:
        rows[5:8] = [n - 1, 0, rows[1]]
    d["rows"] = rows.astype(np.int64)
    bad = [k for k, ok in ppo_cnn_row_conditions(case, d).items() if not ok]
    assert not bad, (case, bad)
    return d


@functools.lru_cache(maxsize=None)
def ppo_cnn_yardstick(case):
    """(inputs, float64 reference, err_t per tensor and per scalar: the same function in float32) of a conv case; once per process."""
    d = ppo_cnn_inputs(case)
    args, kw = (d["cur"], d["old"][:10]) + ppo_cnn_gather(d, d["rows"]), _loss_kw(ppo_cnn_hyper(case))
    r64, r32 = ppo_cnn_epoch64(*args, **kw), ppo_cnn_epoch64(*args, dtype=torch.float32, **kw)
    err_t = {k: rel_err(a, b) for k, a, b in zip(CNN_TENSORS, r32["grads"], r64["grads"])}
    for i, k in enumerate(("policy_loss", "value_loss", "entropy")):
        err_t[k] = cnn_stat_err(case, r64, i, r32["stats"][i])
    return d, r64, err_t


def cnn_stat_pair(case, r64, i, got):
    """(got', want') of logged scalar i (policy loss, value loss, entropy) such that rel_err(got', want') is the error to hold against
    `bound`: the value and the float64 reference. With old == current ("tie") every ratio is 1 and the policy loss is
    -mean(normalised advantage): identically 0 (1e-17 in float64), so an error relative to it means nothing; there the error is taken
    relative to the mean |term| of that sum, mean |normalised advantage| (~0.8), the scale its roundings have."""
    if case.variant == "tie" and i == 0:
        scale = float(np.abs(r64["advantage"]).mean())
        return float(got) - r64["stats"][0] + scale, scale
    return float(got), r64["stats"][i]


def cnn_stat_err(case, r64, i, got):
    return rel_err(*cnn_stat_pair(case, r64, i, got))


# ---- the epoch chain: sgk_ppo_epochs' n_epochs updates in one launch (tests/test_gpu_ppo_epoch_chain.py) -----------------------------
CHAIN_EPOCHS, CHAIN_STEP0 = 4, 4999
CHAIN_STATE_SEED = 91
CHAIN_STALE_FACTOR = 10.0         # how many limits the stale-epoch emulation must lie from the true chain, on every trunk tensor
TRUNK_TENSORS = ("w1", "b1", "w2", "b2")
RAGGED_HORIZON, SPARSE_HORIZON = 5, 16
# the cases of the float64 chain (the seeds: tests/test_learner_reference_cpu.py::test_a_stale_epoch_lies_far_outside_the_chains_limit)
CHAIN_CASES = [PpoCase("SideEffectsSokoban-v0", 100, 64, 2400), PpoCase("BoatRace-v0", 64, 64, 2401),
               PpoCase("DistributionalShift-v0", 100, 33, 2402)]


def ragged_lengths(n):
    """Lengths cycling through 0, 1, 2, 5 (RAGGED_HORIZON = 5): a trajectory of every kind among any four neighbours."""
    return np.array([0, 1, 2, 5], dtype=np.int32)[np.arange(n) % 4]


def sparse_lengths(n=N_ENVS):
    """Four trajectories of SPARSE_HORIZON steps (spread over the four waves' worth of columns), every other one empty: one (t, trajectory)
    candidate in 16 is valid, so a sample's 16 candidates all miss with probability (15/16)^16 = 0.36 and a second Philox round runs."""
    lengths = np.zeros(n, dtype=np.int32)
    lengths[[5, 22, 39, n - 1]] = SPARSE_HORIZON
    return lengths


def ppo_ragged_inputs(case, horizon, lengths):
    """ppo_inputs' rollout and networks at [horizon][len(lengths)] with the given episode lengths (the entries past a trajectory's length
    hold seeded data as well: a row drawn from there changes the result). No rows: the kernel draws them."""
    rng = np.random.default_rng(case.seed + 7000)
    lengths = np.asarray(lengths, dtype=np.int32)
    k0, h, n = ENV_CELLS[case.env], case.hidden, len(lengths)
    assert lengths.max() <= horizon and lengths.any()
    d = {"states": rng.integers(0, 6, (horizon, n, k0)).astype(np.int8),
         "actions": rng.integers(0, 4, (horizon, n)).astype(np.uint8),
         "returns": rng.uniform(-5.0, 5.0, (n, horizon)).astype(np.float32),
         "lengths": lengths}
    old = _linear(rng, h, k0) + _linear(rng, h, h) + _linear(rng, 4, h) + _linear(rng, 1, h)
    d["old"] = old
    d["cur"] = [(p + np.float32(0.05) * rng.standard_normal(p.shape).astype(np.float32)).astype(np.float32) for p in old]
    return d


def chain_rows(case, d, epochs):
    """The caller's rows of a chain on ppo_inputs' dense rollout: epoch 0 takes the case's own minibatch (both clamp branches, a
    duplicate), the later epochs seeded rows; int64 [epochs, batch]. Every pair of the dense rollout is valid, so these are both the
    flat rows t * N + trajectory and the indices into the valid pairs that BatchedPPOAgent.learn takes."""
    rng = np.random.default_rng(case.seed + 500)
    n = SLICES * N_ENVS
    # (below four rows no duplicates: two equal rows of two make the advantages' std 0)
    rows = np.stack([rng.integers(0, n, case.batch) if case.batch >= 4 else rng.choice(n, case.batch, replace=False) for _ in range(epochs)])
    rows[0] = d["rows"]
    return rows.astype(np.int64)


def chain_state(case, d, rows0):
    """(m, v), float32: inject_adam_state around a gradient of constant magnitude per tensor, the largest element of the float64
    gradient of the chain's first epoch. (Around the gradient itself, element by element, v = u g^2 is tiny wherever g is while m ~
    max|g| is not: one step then moves such elements by thousands of lr, which a one-step test bears and a chain does not -- after two
    epochs the logits saturate and the entropy is NaN in float64 as well.) So m ~ N(0, max|g|), v = u max|g|^2 with u log-uniform in
    [1e-3, 1e3]: steps of ~0.03 lr to ~100 lr in every tensor."""
    g = ppo_epoch64(d["cur"], d["old"][:6], *ppo_gather(d, rows0), **_ppo_loss_kw())["grads"]
    return inject_adam_state([np.full(x.shape, np.abs(x).max()) for x in g], CHAIN_STATE_SEED + case.seed, False)[:2]


class _TorchAdam32:
    """torch.optim.Adam itself (the single-tensor implementation) on float32 copies of the tensors, from the given moments and step
    count: the Adam of the float32 yardstick chain. lr, betas and eps are the float32 values the kernels receive, as in adam64."""

    def __init__(self, w, m, v, step0, lr):
        f = lambda x: float(np.float32(x))  # noqa: E731
        self.p = [torch.nn.Parameter(torch.as_tensor(np.array(x, dtype=np.float32))) for x in w]
        self.opt = torch.optim.Adam(self.p, lr=f(lr), betas=(f(BETA1), f(BETA2)), eps=f(EPS), foreach=False, fused=False)
        for p, m_, v_ in zip(self.p, m, v):
            self.opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": torch.as_tensor(np.array(m_, dtype=np.float32)),
                                 "exp_avg_sq": torch.as_tensor(np.array(v_, dtype=np.float32))}

    def step(self, grads):
        for p, g in zip(self.p, grads):
            p.grad = torch.as_tensor(np.asarray(g, dtype=np.float32))
        self.opt.step()
        return [p.detach().numpy().copy() for p in self.p]


def ppo_chain64(d, rows_per_epoch, state, step0, dtype=torch.float64, stale=False):
    """len(rows_per_epoch) times ppo_epoch64 followed by Adam (adam64; torch.optim.Adam on float32 tensors with dtype float32: the yardstick) from d["cur"], the Adam
    state (m, v) (None: zeros) and `step0` steps done: {"params": the eight tensors after every epoch, "stats": the three scalars of
    every epoch}. stale: epoch e >= 1 takes its gradients at the parameters epoch e - 1 started from (what a launch computes whose
    epochs re-read the previous update's stores too early) and applies them to the current ones -- the emulation the CPU suite holds
    the chain test's limit against."""
    f64 = dtype == torch.float64
    ftype = np.float64 if f64 else np.float32
    w = [np.asarray(p, dtype=ftype) for p in d["cur"]]
    m, v = ([np.zeros_like(p) for p in w] for _ in range(2)) if state is None else ([np.asarray(x, dtype=ftype) for x in s] for s in state)
    out = {"params": [], "stats": []}
    t32 = None if f64 else _TorchAdam32(w, m, v, step0, PPO_HYPER["lr"])
    before = w
    for e, rows in enumerate(rows_per_epoch):
        r = ppo_epoch64(before if stale and e else w, d["old"][:6], *ppo_gather(d, np.asarray(rows)), dtype=dtype, **_ppo_loss_kw())
        before = w
        if f64:
            new = [adam64(w[i], m[i], v[i], None, g, step0 + e + 1, PPO_HYPER["lr"]) for i, g in enumerate(r["grads"])]
            w, m, v = [n[0] for n in new], [n[1] for n in new], [n[2] for n in new]
        else:
            w = t32.step(r["grads"])
        out["params"].append(w)
        out["stats"].append(r["stats"])
    return out


def chain_err(got, want, w0):
    """max|got - want| / max|want - w0|: a tensor's error relative to its total movement over the chain."""
    got, want, w0 = (np.asarray(x, dtype=np.float64) for x in (got, want, w0))
    return float(np.abs(got - want).max() / np.abs(want - w0).max())


def chain_limit(err_t, want, w0, epochs):
    """max(8 err_t, epochs x 2^-23 max|w0| / max|want - w0|): the project's margin over the torch-float32 chain's own figure, and never
    below one rounding of the parameter per epoch."""
    want, w0 = np.asarray(want, dtype=np.float64), np.asarray(w0, dtype=np.float64)
    return max(8.0 * err_t, epochs * ULP * float(np.abs(w0).max()) / float(np.abs(want - w0).max()))


@functools.lru_cache(maxsize=None)
def chain_yardstick(case):
    """(inputs, rows [CHAIN_EPOCHS, batch], Adam state, the float64 chain, the torch-float32 chain's err_t per tensor (chain_err after
    the last epoch) and per statistic ("policy_loss 2": rel_err in epoch 2)) of a chain case; once per process."""
    d = ppo_inputs(case)
    rows = chain_rows(case, d, CHAIN_EPOCHS)
    state = chain_state(case, d, rows[0])
    c64, c32 = ppo_chain64(d, rows, state, CHAIN_STEP0), ppo_chain64(d, rows, state, CHAIN_STEP0, dtype=torch.float32)
    err_t = {k: chain_err(a, b, w0) for k, a, b, w0 in zip(PPO_TENSORS, c32["params"][-1], c64["params"][-1], d["cur"])}
    for e in range(CHAIN_EPOCHS):
        for i, k in enumerate(("policy_loss", "value_loss", "entropy")):
            err_t["%s %d" % (k, e)] = rel_err(c32["stats"][e][i], c64["stats"][e][i])
    return d, rows, state, c64, err_t
