"""tests/forward_reference.py checked on the CPU: (1) its float32 run is the product's own torch modules -- DeepQAgent's build_Q, the
PPO-MLP and PPO-CNN old policies, the conv Q body -- so the float64 reference of tests/test_gpu_forward_float64.py is the right network;
(2) every "integer" case keeps every accumulation below 2^24 (float32 is exact there, the GPU test asks for equality); (3) for every
"real" case torch-float32 lies within err_t of float64 with 8 err_t <= 1e-5 (the cap of learner_reference.bound never binds) and at most
1 % of the envs have a float64 top-2 gap below the threshold under which the GPU test leaves the greedy action open; (4) in every case at
least two actions are each the argmax of 2 % of the envs (a wrong score can change the action taken)."""
import types

import numpy as np
import pytest

import forward_reference as FR
import learner_reference as R

N = 40


def _boards(cells, seed):
    return np.random.default_rng(seed).integers(0, 6, (N, cells)).astype(np.int8)


def _copy(params, arrays):
    import torch

    with torch.no_grad():
        for p, a in zip(params, arrays):
            p.copy_(torch.as_tensor(a))


@pytest.mark.parametrize("hidden", FR.HIDDEN)
def test_mlp_forward_is_build_Q_and_the_ppo_mlp_old_policy(hidden):
    """mlp_forward in float32 against the modules tests/test_gpu_deepq.py and tests/test_gpu_ppo.py evaluate on the CPU, with the
    reference's weights copied in: both are float32 torch on the same terms, 1e-6 of the largest score."""
    import torch

    import safe_grid_agents_amd as S

    cells = 49
    w = FR.mlp_weights("real", cells, hidden, 11)
    x = _boards(cells, 12)
    want = FR.mlp_forward(x, *w, dtype=torch.float32)
    q = S.BatchedDeepQAgent.build_Q(types.SimpleNamespace(torch=torch, q_body="mlp", action_n=4), cells, 2, hidden)
    _copy(q.parameters(), w)  # registration order: w1, b1, w2, b2, w3, b3
    with torch.no_grad():
        got = q(torch.as_tensor(x.astype(np.float32))).numpy()
    assert R.rel_err(got, want) <= 1e-6
    env = types.SimpleNamespace(action_space=types.SimpleNamespace(n=4), observation_space=types.SimpleNamespace(shape=(1, 7, 7)))
    args = types.SimpleNamespace(discount=0.99, batch_size=64, rollouts=1, epochs=1, n_layers=2, n_hidden=hidden, device="cpu", log_gradients=False,
                                 **R.PPO_HYPER)
    old = S.PPOMLPAgent(env, args).old_policy
    _copy([old.network[0][0].weight, old.network[0][0].bias, old.network[1][0][0].weight, old.network[1][0][0].bias, old.actor.weight, old.actor.bias], w)
    with torch.no_grad():
        got = old(torch.as_tensor(x.astype(np.float32)).reshape(N, 1, 7, 7))[0].numpy()
    assert R.rel_err(got, want) <= 1e-6


@pytest.mark.parametrize("channels", FR.CHANNELS)
def test_cnn_forward_is_the_conv_q_body_and_the_ppo_cnn_old_policy(channels):
    """cnn_forward in float32 against the conv Q body (deepq_batched._ConvQ through build_Q) and PPOCNNAgent's old policy (its actor
    logits), as tests/test_gpu_convq.py builds them."""
    import torch

    import safe_grid_agents_amd as S

    H, W = 6, 8
    w = FR.cnn_weights("real", (H, W), channels, 21)
    x = _boards(H * W, 22)
    want = FR.cnn_forward(x.reshape(N, H, W), *w, dtype=torch.float32)
    me = types.SimpleNamespace(torch=torch, q_body="cnn", action_n=4, n_channels=channels, env=types.SimpleNamespace(H=H, W=W))
    q = S.BatchedDeepQAgent.build_Q(me, H * W, 2, 100)
    _copy([q.network[0][0].weight, q.network[0][0].bias, q.network[1][0].weight, q.network[1][0].bias, q.bottleneck.weight, q.bottleneck.bias,
           q.head_cnn[0].weight, q.head_cnn[0].bias, q.head_linear.weight, q.head_linear.bias], w)
    with torch.no_grad():
        got = q(torch.as_tensor(x.astype(np.float32))).numpy()
    assert R.rel_err(got, want) <= 1e-6
    env = types.SimpleNamespace(action_space=types.SimpleNamespace(n=4), observation_space=types.SimpleNamespace(shape=(1, H, W)))
    args = types.SimpleNamespace(discount=0.99, batch_size=64, rollouts=1, epochs=1, n_layers=2, n_channels=channels, device="cpu",
                                 log_gradients=False, **R.PPO_HYPER)
    old = S.PPOCNNAgent(env, args).old_policy
    _copy([old.network[0][0].weight, old.network[0][0].bias, old.network[1][0][0].weight, old.network[1][0][0].bias, old.bottleneck.weight,
           old.bottleneck.bias, old.actor_cnn[0].weight, old.actor_cnn[0].bias, old.actor_linear.weight, old.actor_linear.bias], w)
    with torch.no_grad():
        got = old(torch.as_tensor(x.astype(np.float32)).reshape(N, 1, H, W))[0].numpy()
    assert R.rel_err(got, want) <= 1e-6


def test_the_cases_are_the_ones_the_kernels_edges_need():
    ids = [FR.case_id(c) for c in FR.CASES]
    assert len(set(ids)) == len(ids) and len({c.seed for c in FR.CASES}) == len(FR.CASES)
    assert sorted({R.ENV_CELLS[e] % 4 for e in FR.LEVELS}) == [0, 1, 2, 3] and len({R.ENV_CELLS[e] for e in FR.LEVELS}) == 7
    small = {c[:6] for c in FR.SMALL_CASES}
    for body, widths in (("mlp", FR.HIDDEN), ("cnn", FR.CHANNELS)):
        assert all((body, e, w, l, f, "small") in small for e in FR.LEVELS for w in widths for l in FR.LAYOUTS for f in ("integer", "real"))
    assert FR.MLP_N == FR.MLP_ENVS + 32 + 1
    for c in FR.CASES:
        n, cus = FR.case_n(c), FR.DEFAULT_CUS
        if c.body == "mlp":
            tiles = -(-n // FR.MLP_ENVS)
            assert (tiles > cus and n % FR.MLP_ENVS) if c.size == "multi" else tiles == 2
        else:
            envs = FR.conv_envs_per_pass(*R.CNN_SHAPES[c.env])
            passes = -(-n // envs)
            assert (passes > 4 * cus and n % envs) if c.size == "multi" else (passes == 3 and n % envs == 1)
        assert c.size != "multi" or n < 40000


@pytest.mark.parametrize("case", [c for c in FR.CASES if c.family == "integer"], ids=FR.case_id)
def test_integer_cases_are_exact_in_float32(case):
    y = FR.yardstick(case)
    top = FR.abs_sum_bound(case.body, y["boards"], y["weights"], y["shape"])
    print("%s abs-sum bound %.4g, ties %d of %d" % (FR.case_id(case), top, int((y["gap"] == 0).sum()), len(y["gap"])))
    assert top < FR.EXACT_LIMIT
    for p in y["weights"]:
        assert (p == np.round(p)).all()
    assert (y["s64"] == np.round(y["s64"])).all() and y["boards"].min() >= 0
    # the float32 run of the reference itself lands on the same integers
    import torch

    assert np.array_equal(FR.forward(case.body, y["boards"], y["weights"], y["shape"], dtype=torch.float32), y["s64"])
    if case.size == "painted":  # every cell takes part, the wall ring and the row ends included
        assert (y["boards"].max(0) > 0).all() and y["boards"].max() == FR.PAINT_MAX


def test_some_integer_cases_hold_exact_ties_of_the_top_two_scores():
    """"The first maximum wins" inside the fused kernels is only tested where two scores tie: several cases must have such envs."""
    tied = [FR.case_id(c) for c in FR.CASES if c.family == "integer" and (FR.yardstick(c)["gap"] == 0).any()]
    print(tied)
    assert len(tied) >= 3 and any("multi" in t for t in tied)


@pytest.mark.parametrize("case", FR.REAL_CASES, ids=FR.case_id)
def test_real_cases_yardstick_and_near_ties(case):
    y = FR.yardstick(case)
    near = 1.0 - y["clear"].mean()
    print("%s err_t %.3e bound %.3e max|s64| %.3f near-ties %.4f" % (FR.case_id(case), y["err_t"], y["bound"], y["top"], near))
    assert 8.0 * y["err_t"] <= R.CAP
    assert near <= 0.01
    assert np.isfinite(y["s64"]).all()
    for p in y["weights"]:
        assert p.dtype == np.float32


@pytest.mark.parametrize("case", FR.CASES, ids=FR.case_id)
def test_two_actions_are_each_the_argmax_of_two_percent_of_the_envs(case):
    y = FR.yardstick(case)
    share = FR.argmax_shares(y)
    assert (share >= 0.02).sum() >= 2, share
    assert FR.seed_ok(y)
    assert len(y["boards"]) == FR.case_n(case)


@pytest.mark.parametrize("case", FR.ROLLOUT_CASES, ids=FR.rollout_case_id)
def test_rollout_cases_take_two_actions_per_policy_and_stay_exact(case):
    """The greedy rollouts of tests/test_gpu_forward_float64.py emulated on the CPU (the oracle's envs + the float64 argmax): every
    policy takes two actions in 2 % of its (step, env) pairs each, members with weights of their own disagree, the boards change and
    every accumulation stays below 2^24."""
    states, actions = FR.emulate_rollout(case)
    assert FR.rollout_seed_ok(case)
    assert (states[0] != states[-1]).any()
    shape = FR.ROLLOUT_LEVELS[case.level]
    for lo, hi, w in FR.rollout_weights(case):
        assert max(FR.abs_sum_bound(FR.rollout_body(case), states[k, lo:hi], w, shape) for k in range(FR.ROLLOUT_T)) < FR.EXACT_LIMIT
    seeds = [s for c in FR.ROLLOUT_CASES for s in c.seeds]
    assert len(set(seeds)) == len(seeds)
