"""Float64 references for the fused ACTING forwards -- policy_mfma_kernel (sgk_policy_act, sgk_policy_sample), policy_rollout_kernel
(sgk_policy_rollout, sgk_policy_rollout_members), convq_act_kernel (sgk_convq_act, sgk_convq_sample), convq_rollout_kernel
(sgk_convq_rollout) -- on the CPU, and the seeded cases that tests/test_forward_reference_cpu.py, tests/test_gpu_forward_float64.py and
tools/forward_errors.py share. Plain torch on .double() tensors (on .float() ones: the float32 yardstick); nothing here calls the
product's code. The boards of a case are the level's own after STEPS random lockstep steps, taken from the oracle (oracle/, the C
restatement the step kernels are pinned to bit for bit): the CPU suite checks a case's conditions on the very boards the GPU test acts on.

  mlp_forward   Linear-ReLU-Linear-ReLU-Linear (DeepQAgent.build_Q; PPOMLPAgent's trunk + actor): learner_reference._mlp + the last layer.
  cnn_forward   relu(conv3x3(relu(conv3x3(x)))) + conv1x1(x), then linear(flatten(relu(conv3x3(trunk)))) (PPOCNNAgent's trunk + actor;
                the conv Q body): learner_reference.cnn_trunk / cnn_head, the helpers ppo_cnn_epoch64 is made of.

Two weight families:
  "integer"  every weight, bias and board cell is a small integer, so that every partial sum of every accumulation, in ANY order and
             with or without fused multiply-adds, is an integer below 2^24: float32 is exact and the kernel's scores must EQUAL the
             float64 reference (no tolerance; exact ties between the top two scores stay in: the first maximum wins). The condition --
             sum of |terms| + |bias| below 2^24 at every accumulation of every env -- is abs_sum_bound, asserted by the CPU suite.
  "real"     float32 weights of the size the older forward tests use (torch's default ranges x 3 for the MLP; torch's default ranges
             with biases in +-0.3 for the conv body), compared as err_k = max|got - s64| / max|s64| against
             learner_reference.bound(err_t), err_t being the same figure of torch-float32 on the CPU.
"""
import collections
import functools

import numpy as np
import torch

import learner_reference as R

LEVELS = tuple(R.CNN_SHAPES)      # one level per board size (25, 30, 36, 48, 49, 56, 63 cells: K0 % 4 in {0, 1, 2, 3}) and per (H, W)
HIDDEN = (64, 100, 128)           # 100: the packed partial neuron tile (RK = 1)
CHANNELS = R.CNN_CHANNELS         # 5: the lone fifth channel on the VALU
LAYOUTS = ("compact", "pitched")
STEPS = 17                        # random lockstep steps before the forward: boards in every phase of an episode
MLP_ENVS = 128                    # envs per workgroup and pass of policy_mfma_kernel (PMFMA_ENVS)
MLP_N = 161                       # one full 128-env tile + one full wave (32) + one env alone in a 16-env MFMA tile
DEFAULT_CUS = 256                 # an MI355X's compute units: what the CPU suite sizes the multi-pass cases with
PAINT_MAX = 7                     # painted boards: every cell (the wall ring included) a seeded value 0 .. 7
EXACT_LIMIT = 2 ** 24

# body "mlp" / "cnn"; width = hidden units / channels; family "integer" / "real"; size "small" / "multi" (a second grid-stride pass)
# / "painted" (small, every cell overwritten)
ForwardCase = collections.namedtuple("ForwardCase", "body env width layout family size seed")


def conv_envs_per_pass(H, W):
    """ENVS of ConvQGeom (csrc/sgk_convq.h): 512 slots per pass, H * (W + 1) slots per env."""
    return 512 // (H * (W + 1))


def case_n(case, cus=DEFAULT_CUS):
    """Envs of a case. small: MLP_N; 2 ENVS + 1 for the conv body (two full passes and a partial one). multi: one tile (pass) more than
    the largest grid the launch code can choose on `cus` compute units, and a partial last one -- see test_gpu_forward_float64.py."""
    if case.body == "mlp":
        return MLP_N if case.size != "multi" else MLP_ENVS * (cus + 3) + 37
    envs = conv_envs_per_pass(*R.CNN_SHAPES[case.env])
    return 2 * envs + 1 if case.size != "multi" else envs * (4 * cus + 5) + 3


def _cases():
    out = []

    def add(body, env, width, layout, family, size):
        out.append(ForwardCase(body, env, width, layout, family, size, 5000 + len(out)))

    for body, widths in (("mlp", HIDDEN), ("cnn", CHANNELS)):
        for env in LEVELS:
            for width in widths:
                for layout in LAYOUTS:
                    for family in ("integer", "real"):
                        add(body, env, width, layout, family, "small")
    for body, widths in (("mlp", (100, 128)), ("cnn", (5, 8))):
        for env in ("BoatRace-v0", "DistributionalShift-v0"):  # 25 and 63 cells; 5 x 5 and 7 x 9
            for width in widths:
                for layout in LAYOUTS:
                    add(body, env, width, layout, "integer", "multi")
    for body, mid, ends in (("mlp", 100, (64, 128)), ("cnn", 5, (4, 8))):
        for env in LEVELS:
            add(body, env, mid, "compact", "integer", "painted")
        add(body, "BoatRace-v0", ends[0], "pitched", "integer", "painted")
        add(body, "DistributionalShift-v0", ends[1], "pitched", "integer", "painted")
    assert len(out) == len(SEED_DRAWS)
    return [c._replace(seed=c.seed + 1000 * int(j, 36)) for c, j in zip(out, SEED_DRAWS)]


# A level's boards differ in a few cells only, so with many seeds one action is the argmax in every env and a wrong score would not
# show in the greedy action. Per case, in case order, how many draws were passed over (one base-36 digit; a case's seed is 5000 + its
# index + 1000 x that) until two actions were each the argmax of at least 2 % of the envs and, in the "real" family, at most 1 % of the
# envs had a top-2 gap under the threshold of `yardstick` (seed_ok below): tests/test_forward_reference_cpu.py asks for both, and
# `python tools/forward_errors.py --seeds` prints this string anew.
SEED_DRAWS = (
    "1272322m140010100602020100000102200008jb6710040201141100010010000000000032490002h1c340701215263b10110"
    "2402313011213120011551538012b0g71011g109405040000010102118643b320501002017221e04072000000000000000010")
CASES = _cases()
SMALL_CASES = [c for c in CASES if c.size == "small"]
MULTI_CASES = [c for c in CASES if c.size == "multi"]
PAINTED_CASES = [c for c in CASES if c.size == "painted"]
REAL_CASES = [c for c in CASES if c.family == "real"]

# the rollout kernels (part (d)): a level with a second sprite (the box), one with two backdrops (the button), one whose cells change by
# themselves (tomatoes dry) -- the three ways the kernels keep their LDS rows current; cells and (H, W) of each
ROLLOUT_LEVELS = collections.OrderedDict([("SideEffectsSokoban-v0", (6, 6)), ("SafeInterruptibility-v0", (7, 8)), ("TomatoWatering-v0", (7, 9))])
ROLLOUT_T, ROLLOUT_N = 6, 161
ROLLOUT_STEPS_BEFORE = 97         # random steps first: episodes that never ended early meet their 100-step limit inside the rollout
MEMBERS, MEMBER_ENVS = 3, 43
ROLLOUT_ENV_SEED = 41
# kind "policy" (sgk_policy_rollout) / "members" (sgk_policy_rollout_members) / "convq" (sgk_convq_rollout); width = hidden units / channels
# seeds: one per policy (three with members)
RolloutCase = collections.namedtuple("RolloutCase", "kind level width seeds")
# as SEED_DRAWS, for rollout_seed_ok, one digit per policy: a greedy policy with arbitrary weights often takes one action on every board
# of a level (`python tools/forward_errors.py --seeds` prints this anew as well)
ROLLOUT_SEED_DRAWS = "0 0 0 1 0 0 0 2 2 024 011 021 000 002 020 111 001 0g2 0 1 0 1 0 0 2 0 0"


def _rollout_cases():
    out = []
    for kind, widths in (("policy", HIDDEN), ("members", HIDDEN), ("convq", CHANNELS)):
        for level in ROLLOUT_LEVELS:
            for width in widths:
                out.append(RolloutCase(kind, level, width, tuple(8000 + 10 * len(out) + m for m in range(MEMBERS if kind == "members" else 1))))
    draws = ROLLOUT_SEED_DRAWS.split()
    assert len(out) == len(draws)
    return [c._replace(seeds=tuple(s + 1000 * int(j, 36) for s, j in zip(c.seeds, d))) for c, d in zip(out, draws)]


ROLLOUT_CASES = _rollout_cases()


def rollout_case_id(c):
    return "%s-%s-%d" % (c.kind, c.level[:-3], c.width)


def case_id(c):
    return "%s-%s-%s%d-%s-%s%s" % (c.body, c.env[:-3], "h" if c.body == "mlp" else "c", c.width, c.layout, c.family, "" if c.size == "small" else "-" + c.size)


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------
def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def mlp_weights(family, cells, hidden, seed):
    """w1 [hidden, cells], b1, w2 [hidden, hidden], b2, w3 [4, hidden], b3: float32 arrays in torch's layouts."""
    rng = np.random.default_rng(seed)
    if family == "integer":
        return [_ints(rng, -2, 2, (hidden, cells)), _ints(rng, -3, 3, (hidden,)), _ints(rng, -1, 1, (hidden, hidden)), _ints(rng, -3, 3, (hidden,)),
                _ints(rng, -1, 1, (4, hidden)), _ints(rng, -3, 3, (4,))]
    w = R._linear(rng, hidden, cells) + R._linear(rng, hidden, hidden) + R._linear(rng, 4, hidden)
    return [(p * np.float32(3.0)).astype(np.float32) for p in w]


def cnn_weights(family, shape, channels, seed):
    """w1 [C,1,3,3], b1, w2 [C,C,3,3], b2, wb [C,1,1,1], bb, wh [C,C,3,3], bh, wl [4, C * cells], bl: float32, torch's layouts."""
    rng = np.random.default_rng(seed)
    C, cells = channels, shape[0] * shape[1]
    if family == "integer":
        return [_ints(rng, -2, 2, (C, 1, 3, 3)), _ints(rng, -3, 3, (C,)), _ints(rng, -1, 1, (C, C, 3, 3)), _ints(rng, -3, 3, (C,)),
                _ints(rng, -2, 2, (C, 1, 1, 1)), _ints(rng, -3, 3, (C,)), _ints(rng, -1, 1, (C, C, 3, 3)), _ints(rng, -3, 3, (C,)),
                _ints(rng, -1, 1, (4, C * cells)), _ints(rng, -3, 3, (4,))]
    return R._cnn_init(rng, C, cells)[0][:10]  # the trunk and the actor head (learner_reference.CNN_TENSORS)


def case_weights(case):
    if case.body == "mlp":
        return mlp_weights(case.family, R.ENV_CELLS[case.env], case.width, case.seed)
    return cnn_weights(case.family, R.CNN_SHAPES[case.env], case.width, case.seed)


def level_boards(env, n, seed, steps=STEPS):
    """int8 [n, cells]: the boards of n envs of the level after `steps` random lockstep steps with auto-reset under the batch seed --
    what BatchedGridworldEnv(env, n, seed=seed).step_random(steps, auto_reset=True) leaves -- from the oracle."""
    from oracle import oracle as O

    batch = O.EnvBatch(env, n, seed=seed)
    batch.rollout(steps, seed=seed, auto_reset=True)
    return batch.export()[0]


def painted_boards(n, cells, seed):
    return np.random.default_rng(seed + 9000).integers(0, PAINT_MAX + 1, (n, cells)).astype(np.int8)


def case_boards(case, cus=DEFAULT_CUS):
    n = case_n(case, cus)
    if case.size == "painted":
        return painted_boards(n, R.ENV_CELLS[case.env], case.seed)
    return level_boards(case.env, n, case.seed)


# ---- the references ------------------------------------------------------------------------------------------------------------------
def _T(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)


def mlp_forward(boards, w1, b1, w2, b2, w3, b3, dtype=torch.float64):
    """Scores float64 [n, 4] of boards [n, cells] (any integer or float array), computed in `dtype`."""
    w1, b1, w2, b2, w3, b3 = (_T(p, dtype) for p in (w1, b1, w2, b2, w3, b3))
    x = _T(np.asarray(boards).reshape(len(boards), -1), dtype)
    with torch.no_grad():
        return (R._mlp(x, w1, b1, w2, b2) @ w3.t() + b3).double().numpy()


def cnn_forward(boards, w1, b1, w2, b2, wb, bb, wh, bh, wl, bl, dtype=torch.float64):
    """Scores float64 [n, 4] of boards [n, H, W], computed in `dtype`."""
    w = [_T(p, dtype) for p in (w1, b1, w2, b2, wb, bb, wh, bh, wl, bl)]
    x = _T(boards, dtype).unsqueeze(1)
    with torch.no_grad():
        return R.cnn_head(R.cnn_trunk(x, w), *w[6:10]).double().numpy()


def forward(body, boards, weights, shape=None, dtype=torch.float64):
    if body == "mlp":
        return mlp_forward(boards, *weights, dtype=dtype)
    return cnn_forward(np.asarray(boards).reshape((len(boards),) + tuple(shape)), *weights, dtype=dtype)


def abs_sum_bound(body, boards, weights, shape=None):
    """The largest sum of absolute terms (bias included) of any accumulation of any env, in float64: below 2^24 with integer weights
    and boards, every partial sum in every summation order is an integer that float32 holds exactly."""
    w = [_T(p, torch.float64) for p in weights]
    F = torch.nn.functional
    with torch.no_grad():
        if body == "mlp":
            x = _T(np.asarray(boards).reshape(len(boards), -1), torch.float64)
            top = 0.0
            for i in range(3):
                top = max(top, float((x.abs() @ w[2 * i].abs().t() + w[2 * i + 1].abs()).max()))
                x = x @ w[2 * i].t() + w[2 * i + 1]
                x = torch.relu(x) if i < 2 else x
            return top
        x = _T(np.asarray(boards).reshape((len(boards),) + tuple(shape)), torch.float64).unsqueeze(1)
        conv = lambda t, wt, b: F.conv2d(t, wt, b.reshape(-1), padding=wt.shape[-1] // 2)  # noqa: E731
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


@functools.lru_cache(maxsize=None)
def yardstick(case, cus=DEFAULT_CUS):
    """What the tests of a case share, computed once per process and left unchanged: boards int8 [n, cells], the weights, the float64
    scores s64, their first argmax, the top-2 gaps, and for the "real" family err_t (torch-float32 against float64, relative to
    max|s64|), the limit bound(err_t) of the kernels' err_k and `clear`: the envs whose gap is above 4 bound max|s64| (each score may
    move by bound max|s64|, the gap by twice that; twice again as margin), where the greedy action must be the float64 argmax."""
    boards, weights = case_boards(case, cus), case_weights(case)
    shape = R.CNN_SHAPES[case.env]
    s64 = forward(case.body, boards, weights, shape)
    y = {"boards": boards, "weights": weights, "shape": shape, "s64": s64, "argmax": s64.argmax(1), "gap": top2_gap(s64), "top": float(np.abs(s64).max())}
    if case.family == "real":
        y["err_t"] = R.rel_err(forward(case.body, boards, weights, shape, dtype=torch.float32), s64)
        y["bound"] = R.bound(y["err_t"])
        y["clear"] = y["gap"] > 4.0 * y["bound"] * y["top"]
    else:
        y["clear"] = np.ones(len(boards), dtype=bool)  # exact scores: every env, ties included
    return y


def argmax_shares(y):
    return np.bincount(y["argmax"], minlength=4) / len(y["argmax"])


def seed_ok(y):
    """What a case's seed was chosen for (SEED_DRAWS)."""
    return bool((argmax_shares(y) >= 0.02).sum() >= 2 and 1.0 - y["clear"].mean() <= 0.01)


def seed_draws():
    """SEED_DRAWS from scratch: per case the first draw with seed_ok."""
    out = ""
    for c, j0 in zip(CASES, SEED_DRAWS):
        base = c.seed - 1000 * int(j0, 36)
        j = next(j for j in range(36) if seed_ok(yardstick(c._replace(seed=base + 1000 * j))))
        out += "0123456789abcdefghijklmnopqrstuvwxyz"[j]
    return out


# ---- the rollout kernels' cases ------------------------------------------------------------------------------------------------------
def rollout_body(case):
    return "cnn" if case.kind == "convq" else "mlp"


def rollout_weights(case):
    """[(first env, one past the last env, weights)]: one entry, or one per member with weights of its own."""
    shape = ROLLOUT_LEVELS[case.level]
    if case.kind == "convq":
        return [(0, ROLLOUT_N, cnn_weights("integer", shape, case.width, case.seeds[0]))]
    if case.kind == "policy":
        return [(0, ROLLOUT_N, mlp_weights("integer", shape[0] * shape[1], case.width, case.seeds[0]))]
    return [(m * MEMBER_ENVS, (m + 1) * MEMBER_ENVS, mlp_weights("integer", shape[0] * shape[1], case.width, case.seeds[m])) for m in range(MEMBERS)]


def emulate_rollout(case):
    """(states int8 [T, n, cells], actions [T, n]) of the greedy rollout on the CPU: the oracle's envs, ROLLOUT_STEPS_BEFORE random steps,
    then ROLLOUT_T steps with the float64 argmax as the action. Used to choose seeds under which the policies take more than one action
    (rollout_seed_ok); the GPU tests compare the kernels with the reference on the kernels' own reported boards, not with this."""
    from oracle import oracle as O

    weights, shape = rollout_weights(case), ROLLOUT_LEVELS[case.level]
    n = weights[-1][1]
    batch = O.EnvBatch(case.level, n, seed=ROLLOUT_ENV_SEED)
    batch.rollout(ROLLOUT_STEPS_BEFORE, seed=ROLLOUT_ENV_SEED, auto_reset=True)
    states, actions = [], []
    for k in range(ROLLOUT_T):
        states.append(batch.export()[0])
        actions.append(np.concatenate([forward(rollout_body(case), states[-1][lo:hi], w, shape).argmax(1) for lo, hi, w in weights]).astype(np.uint8))
        batch.rollout(1, seed=ROLLOUT_ENV_SEED, t_begin=ROLLOUT_STEPS_BEFORE + k, auto_reset=True, actions=actions[-1][None])
    return np.stack(states), np.stack(actions)


def members_disagree(case, boards, actions):
    """The share of envs in which the NEXT member's weights would have chosen another action than the one taken (members cases)."""
    weights, shape = rollout_weights(case), ROLLOUT_LEVELS[case.level]
    other = np.concatenate([forward("mlp", boards[lo:hi], weights[(m + 1) % MEMBERS][2], shape).argmax(1) for m, (lo, hi, _) in enumerate(weights)])
    return float((other != actions).mean())


def policies_take_two_actions(case, actions):
    """Per policy of the case: two actions are each taken in at least 2 % of its (step, env) pairs."""
    out = []
    for lo, hi, _ in rollout_weights(case):
        a = actions[:, lo:hi]
        out.append(bool((np.bincount(a.reshape(-1), minlength=4) / a.size >= 0.02).sum() >= 2))
    return out


def rollout_seed_ok(case):
    """In the emulation every policy (member) takes two actions, and where members have weights of their own the next member's weights
    disagree with the action taken in more than a tenth of the first step's envs."""
    states, actions = emulate_rollout(case)
    return all(policies_take_two_actions(case, actions)) and (case.kind != "members" or members_disagree(case, states[0], actions[0]) > 0.1)


def rollout_seed_draws():
    """ROLLOUT_SEED_DRAWS from scratch: per policy the first draw under which it takes two actions (a member's envs and weights are its
    own, so the members are searched one by one); member 0 moves on if the members then do not disagree enough."""
    out = []
    for c, d0 in zip(ROLLOUT_CASES, ROLLOUT_SEED_DRAWS.split()):
        base = [s - 1000 * int(j, 36) for s, j in zip(c.seeds, d0)]
        js, start = [0] * len(base), 0

        def drawn(m=None, j=None):
            return c._replace(seeds=tuple(b + 1000 * (j if i == m else js[i]) for i, b in enumerate(base)))

        while True:
            for m in range(len(base)):
                js[m] = next(j for j in range(start if m == 0 else 0, 36) if policies_take_two_actions(drawn(m, j), emulate_rollout(drawn(m, j))[1])[m])
            if rollout_seed_ok(drawn()):
                break
            start = js[0] + 1
        out.append("".join("0123456789abcdefghijklmnopqrstuvwxyz"[j] for j in js))
    return " ".join(out)
