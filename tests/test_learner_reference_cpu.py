"""tests/learner_reference.py checked on the CPU: (1) dqn_step64 + adam64 reproduce the reference's own DeepQAgent.learn run
(tests/golden/deepq_learn.npz) -- the reference is the right formula; (2) the yardstick of tests/test_gpu_learner_gradients.py: for
every case there, torch-float32 autograd on the same inputs lies within err_t of the float64 reference with 8 err_t <= 1e-5, so the cap
of the GPU tests is never the binding bound; (3) the cases named "clipped" / "unclipped" are what they say; (4) the same for the conv
body (ppo_cnn_epoch64 against PPOCNNAgent.surrogate_loss and the reference's own ppo-cnn run; the yardstick and the rows of every case
of tests/test_gpu_ppo_cnn_gradients.py)."""
import json
import os

import numpy as np
import pytest

import learner_reference as R


def test_dqn_step64_and_adam64_reproduce_the_reference_learn_steps(golden_dir):
    """The inputs of test_fused_dqn_sgd_step_reproduces_the_reference_learn_steps (14 learn() calls on a 10-entry deque, the recorded
    sample positions, a target sync after step 7) through the float64 reference and adam64 (amsgrad): the reference's 14 losses and final
    weights. The golden is float32: that test's own tolerance, rtol 2e-4 / atol 2e-6."""
    z = np.load(os.path.join(golden_dir, "deepq_learn.npz"))
    meta = json.loads(str(z["meta"]))
    keys = ("0_0_weight", "0_0_bias", "1_0_0_weight", "1_0_0_bias", "2_weight", "2_bias")
    w = [z["init_Q_" + k].astype(np.float64) for k in keys]
    t = [z["init_T_" + k].astype(np.float64) for k in keys]
    m, v, x = ([np.zeros_like(p) for p in w] for _ in range(3))
    ring, losses = [], []
    for k in range(meta["steps"]):
        ring.append(k)
        ring = ring[-meta["replay_capacity"]:]  # ReplayBuffer.add (contain.py:15-17): the deque evicts its oldest entry
        ix = np.asarray(ring)[z["sample_ix"][k]]
        out = R.dqn_step64(w, t, z["states"][ix], z["successors"][ix], z["actions"][ix], z["rewards"][ix], z["terminals"][ix],
                           meta["discount"], 1.0, broadcast=True)
        losses.append(out["loss"])
        for i, g in enumerate(out["clipped_grads"]):
            w[i], m[i], v[i], x[i] = R.adam64(w[i], m[i], v[i], x[i], g, k + 1, meta["lr"])
        if k + 1 == meta["sync_after_step"]:
            t = [p.copy() for p in w]
    np.testing.assert_allclose(losses, z["losses"], rtol=2e-4)
    for k, p in zip(keys, w):
        np.testing.assert_allclose(p, z["final_Q_" + k], rtol=2e-4, atol=2e-6, err_msg=k)


def test_adam64_is_torch_adam():
    """adam64 against torch.optim.Adam in float64 over six steps, with and without amsgrad, from a state where vmax decides."""
    import torch

    rng = np.random.default_rng(5)
    b1, b2 = float(np.float32(R.BETA1)), float(np.float32(R.BETA2))
    lr, eps = float(np.float32(1e-2)), float(np.float32(R.EPS))
    for amsgrad in (False, True):
        p = torch.nn.Parameter(torch.as_tensor(rng.standard_normal(50)))
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, amsgrad=amsgrad)
        w, m, v = p.detach().numpy().copy(), np.zeros(50), np.zeros(50)
        x = np.zeros(50) if amsgrad else None
        for step in range(1, 7):
            g = rng.standard_normal(50) * (10.0 if step == 1 else 1.0)  # a large first gradient: vmax stays above v afterwards
            p.grad = torch.as_tensor(g.copy())
            opt.step()
            w, m, v, x = R.adam64(w, m, v, x, g, step, 1e-2)
            np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-12, atol=1e-15)
        if amsgrad:
            assert (x >= v).all() and (x > v).any()


def test_ppo_epoch64_is_the_agents_surrogate_loss():
    """ppo_epoch64 (here on float32, the form the yardstick uses) against PPOMLPAgent.surrogate_loss + autograd on the CPU -- the
    golden-pinned host implementation of ppo.py -- with the same weights and minibatch: the three scalars and the eight gradients.
    Both are float32 torch on the same terms: 1e-5 of each tensor's largest element."""
    import types

    import torch

    import safe_grid_agents_amd as S

    case = next(c for c in R.PPO_CASES if c.batch == 33)
    d = R.ppo_inputs(case)
    k0 = R.ENV_CELLS[case.env]
    env = types.SimpleNamespace(action_space=types.SimpleNamespace(n=4), observation_space=types.SimpleNamespace(shape=(1, 1, k0)))
    args = types.SimpleNamespace(discount=0.99, batch_size=case.batch, rollouts=1, epochs=1, n_layers=2, n_hidden=case.hidden, device="cpu",
                                 log_gradients=False, **R.PPO_HYPER)
    agent = S.PPOMLPAgent(env, args)
    own = [agent.network[0][0].weight, agent.network[0][0].bias, agent.network[1][0][0].weight, agent.network[1][0][0].bias,
           agent.actor.weight, agent.actor.bias, agent.critic.weight, agent.critic.bias]
    old = agent.old_policy
    olds = [old.network[0][0].weight, old.network[0][0].bias, old.network[1][0][0].weight, old.network[1][0][0].bias, old.actor.weight,
            old.actor.bias]
    with torch.no_grad():
        for p, a in list(zip(own, d["cur"])) + list(zip(olds, d["old"][:6])):
            p.copy_(torch.as_tensor(a))
    s, a, r = R.ppo_gather(d, d["rows"])
    loss, pl, vl, en = agent.surrogate_loss(torch.as_tensor(s.astype(np.float32)).reshape(-1, 1, 1, k0), torch.as_tensor(a.astype(np.int64)),
                                            torch.as_tensor(r))
    grads = torch.autograd.grad(loss, own)
    ref = R.ppo_epoch64(d["cur"], d["old"][:6], s, a, r, dtype=torch.float32,
                        **{k: R.PPO_HYPER[k] for k in ("clipping", "critic_coeff", "entropy_bonus")})
    np.testing.assert_allclose(ref["stats"], [float(pl.detach()), float(vl.detach()), float(en.detach())], rtol=1e-5)
    for k, g, want in zip(R.PPO_TENSORS, ref["grads"], grads):
        assert R.rel_err(g, want.numpy()) <= 1e-5, k


@pytest.mark.parametrize("case", R.DQN_CASES, ids=R.case_id)
def test_dqn_yardstick_and_clip_condition(case):
    d, r64, err_t = R.dqn_yardstick(case)
    print("dqn %-60s norm64 %9.4f coef64 %.6f " % (R.case_id(case), r64["norm"], r64["coef"]) + " ".join("%s %.2e" % kv for kv in err_t.items()))
    assert (r64["norm"] > 20.0) if case.clipped else (r64["norm"] < 5.0), r64["norm"]
    assert (r64["coef"] < 0.5) if case.clipped else (r64["coef"] == 1.0)
    for k, e in err_t.items():
        assert 8.0 * e <= R.CAP, (k, e)
    rows = d["rows"]
    term = d["terminals"].reshape(-1)[rows]
    if case.batch == 1:
        assert term[0] == (case.rows == "terminal")
    else:
        assert len(set(rows.tolist())) < case.batch and term.any() and not term.all()
    assert 0.2 < d["terminals"].mean() < 0.4


@pytest.mark.parametrize("case", R.PPO_CASES, ids=R.case_id)
def test_ppo_yardstick_and_clamp_branches(case):
    d, r64, err_t = R.ppo_yardstick(case)
    print("ppo %-40s " % R.case_id(case) + " ".join("%s %.2e" % kv for kv in err_t.items()))
    for k, e in err_t.items():
        assert 8.0 * e <= R.CAP, (k, e)
    lo, hi = 1 - R.PPO_HYPER["clipping"], 1 + R.PPO_HYPER["clipping"]
    out = (r64["ratio"] < lo) | (r64["ratio"] > hi)
    assert out.any() and not out.all()  # both branches of the clamp's gradient
    assert case.batch < 4 or len(set(d["rows"].tolist())) < case.batch


def test_case_lists_cover_what_the_issue_names():
    cells = {R.ENV_CELLS[c.env] for c in R.DQN_CASES if c.batch == 64 and c.clipped and c.broadcast}
    assert cells == {25, 30, 36, 48, 49, 56, 63}
    assert {(c.env, c.hidden) for c in R.DQN_CASES if c.batch == 64 and c.clipped and c.broadcast} == {(e, h) for e in R.ENV_CELLS for h in (64, 100)}
    assert {R.ENV_CELLS[c.env] for c in R.PPO_CASES if c.batch == 64} == {25, 30, 36, 48, 49, 56, 63}
    assert {c.batch for c in R.PPO_CASES} == {2, 33, 64} and {c.batch for c in R.DQN_CASES} == {1, 17, 64}
    # four (env, units, batch) for the one-launch child; the batch-1 one runs on a terminal and on a non-terminal row: five cases
    assert len(R.CHILD_CASES) == 5 and sum(not c.clipped for c in R.DQN_CASES) == 2 and sum(not c.broadcast for c in R.DQN_CASES) == 2
    ms, vs, xs = R.inject_adam_state([np.array([0.0, 1.0, -2.0, 0.0]), np.array([[3.0]])], 1, True)
    assert (vs[0] > 0).all() and {float(a / b) for a, b in zip(xs[0], vs[0])} == {0.5, 2.0} and ms[1].shape == (1, 1)


def test_rtol_on_the_first_moment_needs_the_operands_scale():
    """Why tests/test_gpu_learner_gradients.py takes m' against |m| + (1 - beta1) |g - m| and not against |m'|: m' = m + (1 - beta1)(g - m)
    evaluated in float32 with every operation EXACTLY rounded (numpy) on the injected state of one case misses 1e-6 |m'| by two orders of
    magnitude in the elements where the two terms cancel, and stays far inside 1e-6 of the operands' scale."""
    import torch

    case = next(c for c in R.DQN_CASES if R.case_id(c) == "IslandNavigation-h64-b17-clipped-broadcast")
    d = R.dqn_yardstick(case)[0]
    args = (d["q"], d["t"]) + R.dqn_gather(d, d["rows"]) + (R.DQN_DISCOUNT, d["reward_scale"], case.broadcast)
    f = np.float32
    g = R.dqn_step64(*args, dtype=torch.float32)["clipped_grads"][0].astype(f)
    g_c = ((f(1) - f(R.BETA1)) * g).astype(np.float64) / R.one_minus_beta1()
    (m0,), (v0,), (x0,) = R.inject_adam_state([g_c], 77 + case.seed, True)
    m1 = (m0 + (f(1) - f(R.BETA1)) * (g - m0)).astype(f)
    m_ref = R.adam64(d["q"][0], m0, v0, x0, g_c, 5000, R.DQN_LR)[1]
    scale = np.abs(m0.astype(np.float64)) + R.one_minus_beta1() * np.abs(g_c - m0)
    assert (np.abs(m1 - m_ref) / (1e-6 * np.abs(m_ref))).max() > 100.0
    assert (np.abs(m1 - m_ref) / (1e-6 * scale)).max() < 0.5


# ---- the conv body (tests/test_gpu_ppo_cnn_gradients.py) -----------------------------------------------------------------------------
def _cnn_agent(shape, channels, batch, hyper):
    import types

    import safe_grid_agents_amd as S

    env = types.SimpleNamespace(action_space=types.SimpleNamespace(n=4), observation_space=types.SimpleNamespace(shape=(1,) + tuple(shape)))
    args = types.SimpleNamespace(discount=0.99, batch_size=batch, rollouts=1, epochs=1, n_layers=2, n_channels=channels, device="cpu",
                                 log_gradients=False, **hyper)
    return S.PPOCNNAgent(env, args)


@pytest.mark.parametrize("case", R.PLUMBING_CASES, ids=R.cnn_case_id)
def test_ppo_cnn_epoch64_is_the_agents_surrogate_loss(case):
    """ppo_cnn_epoch64 on float32 (the form the yardstick uses) against PPOCNNAgent.surrogate_loss + autograd on the CPU -- the
    golden-pinned host implementation of ppo.py -- with the same weights and minibatch, for a C = 5 case under PPO_HYPER and the C = 8
    case under the agent's defaults: the three scalars and the 14 gradients. Both are float32 torch on the same terms: 1e-5 of each
    tensor's largest element."""
    import torch

    import safe_grid_agents_amd as S

    d = R.ppo_cnn_inputs(case)
    hyper = R.ppo_cnn_hyper(case)
    agent = _cnn_agent(d["shape"], case.channels, case.batch, hyper)
    own, old = dict(agent.named_parameters()), dict(agent.old_policy.named_parameters())
    names = S.BatchedPPOAgent.CNN_PARAMS
    assert len(names) == len(R.CNN_TENSORS) == 14
    with torch.no_grad():
        for k, cur, o in zip(names, d["cur"], d["old"]):
            assert own[k].shape == cur.shape, k
            own[k].copy_(torch.as_tensor(cur))
            old[k].copy_(torch.as_tensor(o))
    s, a, r = R.ppo_cnn_gather(d, d["rows"])
    loss, pl, vl, en = agent.surrogate_loss(torch.as_tensor(s.astype(np.float32)).unsqueeze(1), torch.as_tensor(a.astype(np.int64)), torch.as_tensor(r))
    grads = torch.autograd.grad(loss, [own[k] for k in names])
    ref = R.ppo_cnn_epoch64(d["cur"], d["old"][:10], s, a, r, dtype=torch.float32, **{k: hyper[k] for k in ("clipping", "critic_coeff", "entropy_bonus")})
    np.testing.assert_allclose(ref["stats"], [float(pl.detach()), float(vl.detach()), float(en.detach())], rtol=1e-5)
    for k, g, want in zip(R.CNN_TENSORS, ref["grads"], grads):
        assert g.shape == tuple(want.shape) and R.rel_err(g, want.numpy()) <= 1e-5, k


def test_ppo_cnn_epoch64_reproduces_the_reference_ppo_cnn_runs_first_epochs(golden_dir):
    """batched_ppo_cnn_boat.npz (the reference's PPOCNNAgent, 5 channels, batch 64): the weights before each iteration's learn, its
    first epoch's rows (indices into the valid (t, env) pairs in that order), boards and returns through ppo_cnn_epoch64 in float64 give
    the reference's recorded first-epoch policy loss, value loss and entropy, at the tolerance
    test_fused_cnn_learner_reproduces_the_reference_ppo_cnn_run uses for them (rtol 2e-3 / atol 2e-5). The old policy is the current one
    there (sync() before every gather): the recorded policy loss is -mean(normalised advantage) = 0 within float32 rounding."""
    import batched_golden as BG
    import safe_grid_agents_amd as S

    fx = BG.PpoFixture("batched_ppo_cnn_boat.npz")
    m = fx.meta
    kw = {k: m[k] for k in ("clipping", "critic_coeff", "entropy_bonus")}
    for it in range(fx.iterations):
        w = fx.weights(it)
        params = [w[k] for k in S.BatchedPPOAgent.CNN_PARAMS]
        lengths, states, actions, returns = (fx.it(it, k) for k in ("lengths", "states", "actions", "returns"))  # [n], [n, horizon, ...]
        valid = np.arange(fx.horizon)[:, None] < lengths[None, :]  # [T, n]
        t_ix, n_ix = np.nonzero(valid)
        pick = fx.it(it, "rows")[0]
        t, n = t_ix[pick], n_ix[pick]
        out = R.ppo_cnn_epoch64(params, params[:10], states[n, t].reshape(-1, 5, 5), actions[n, t], returns[n, t], **kw)
        np.testing.assert_allclose(out["stats"], fx.losses(it)[0], rtol=2e-3, atol=2e-5)
        assert (out["ratio"] == 1.0).all()


@pytest.mark.parametrize("case", R.PPO_CNN_CASES, ids=R.cnn_case_id)
def test_ppo_cnn_yardstick_and_rows(case):
    """torch-float32's own error stays below the cap / 8 for every tensor and scalar of every conv case, and the minibatch holds the rows
    it is meant to hold (learner_reference.ppo_cnn_row_conditions, in float64): the four clamp branches away from the clip bounds and
    from a zero advantage, a row inside, the rollout's first and last row, a duplicate."""
    d, r64, err_t = R.ppo_cnn_yardstick(case)
    print("ppo-cnn %-40s " % R.cnn_case_id(case) + " ".join("%s %.2e" % kv for kv in err_t.items()))
    assert set(err_t) == set(R.CNN_TENSORS) | {"policy_loss", "value_loss", "entropy"}
    for k, e in err_t.items():
        assert 8.0 * e <= R.CAP, (k, e)
    conditions = R.ppo_cnn_row_conditions(case, d)
    assert all(conditions.values()), conditions
    want = {"tie": 6 if case.batch >= 8 else 3, "clip": 10 if case.batch >= 8 else 5, "defaults": 10}[case.variant]
    assert len(conditions) == want, conditions  # (none of them silently left out)
    h = R.ppo_cnn_hyper(case)
    out = (r64["ratio"] < 1 - h["clipping"]) | (r64["ratio"] > 1 + h["clipping"])
    assert (out.any() and not out.all()) or case.variant == "tie"
    assert d["states"].shape == (R.CNN_T, R.CNN_N, d["shape"][0] * d["shape"][1]) and d["returns"].shape == (R.CNN_N, R.CNN_T)
    ring = d["states"].reshape((-1,) + d["shape"])
    border = np.concatenate([ring[:, 0].ravel(), ring[:, -1].ravel(), ring[:, :, 0].ravel(), ring[:, :, -1].ravel()])
    assert set(border.tolist()) == set(range(6)) and (d["lengths"] == R.CNN_T).all()  # no constant wall ring
    for g in r64["grads"]:
        assert np.abs(g).max() > 0


def test_conv_case_list_covers_what_the_issue_names():
    from oracle import oracle as O

    for env, shape in R.CNN_SHAPES.items():
        assert tuple(O.shape(env)) == shape, env
    cases = R.PPO_CNN_CASES
    pairs = {(c.env, c.channels) for c in cases if c.batch == 64 and c.variant == "clip"}
    assert pairs == {(e, ch) for e in R.CNN_SHAPES for ch in (4, 5, 8)} and len(pairs) == 21
    assert len(set(R.CNN_SHAPES.values())) == 7
    assert {c.batch for c in cases} == {2, 37, 64}
    for batch in (2, 37):
        small = [c for c in cases if c.batch == batch]
        assert len({c.env for c in small}) == 2 and {c.channels for c in small} == {5, 8}
    assert [c.batch for c in cases if c.variant == "defaults"] == [37] and sum(c.variant == "tie" for c in cases) == 1
    assert R.ppo_cnn_hyper(next(c for c in cases if c.variant == "defaults")) == dict(lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01)
    assert all(R.ppo_cnn_hyper(c) == R.PPO_HYPER for c in cases if c.variant != "defaults")
    assert len({c.seed for c in cases}) == len(cases) and not {c.seed for c in cases} & {c.seed for c in R.PPO_CASES + R.DQN_CASES}
    assert {c.channels for c in R.PLUMBING_CASES} == {5, 8} and (R.CNN_T, R.CNN_N) == (3, 37)


# ---- the epoch chain (tests/test_gpu_ppo_epoch_chain.py) -----------------------------------------------------------------------------
def test_ppo_chain64_of_one_epoch_is_ppo_epoch64_then_adam64():
    """ppo_chain64 with one epoch against the step the one-epoch tests take (ppo_epoch64's gradients through adam64 at step0 + 1, from the
    same injected state), exactly; and with two epochs, the second epoch is that step again from the first one's results."""
    case = R.CHAIN_CASES[0]
    d, rows, state, c64, _ = R.chain_yardstick(case)
    kw = {k: R.PPO_HYPER[k] for k in ("clipping", "critic_coeff", "entropy_bonus")}
    one = R.ppo_chain64(d, rows[:1], state, R.CHAIN_STEP0)
    ref = R.ppo_epoch64(d["cur"], d["old"][:6], *R.ppo_gather(d, rows[0]), **kw)
    assert one["stats"] == [ref["stats"]] and len(one["params"]) == 1
    stepped = [R.adam64(d["cur"][i], state[0][i], state[1][i], None, g, R.CHAIN_STEP0 + 1, R.PPO_HYPER["lr"]) for i, g in enumerate(ref["grads"])]
    for k, got, want in zip(R.PPO_TENSORS, one["params"][0], stepped):
        assert got.dtype == np.float64 and (got == want[0]).all() and np.abs(got - d["cur"][R.PPO_TENSORS.index(k)]).max() > 0, k
    for got, want in zip(c64["params"][0], one["params"][0]):
        assert (got == want).all()
    ref2 = R.ppo_epoch64(one["params"][0], d["old"][:6], *R.ppo_gather(d, rows[1]), **kw)
    assert c64["stats"][1] == ref2["stats"]
    for i, g in enumerate(ref2["grads"]):
        want = R.adam64(one["params"][0][i], stepped[i][1], stepped[i][2], None, g, R.CHAIN_STEP0 + 2, R.PPO_HYPER["lr"])[0]
        assert (c64["params"][1][i] == want).all(), i
    zero = R.ppo_chain64(d, rows[:1], None, 0)  # no state: zero moments, the first Adam step moves an element by lr |g| / (|g| + eps)
    moved = np.abs(zero["params"][0][2] - d["cur"][2])
    lr = float(np.float32(R.PPO_HYPER["lr"]))
    assert (moved <= lr * (1 + 1e-12)).all() and np.median(moved[ref["grads"][2] != 0]) > 0.999 * lr


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=R.case_id)
def test_a_stale_epoch_lies_far_outside_the_chains_limit(case):
    """What keeps the float64 chain test from being vacuous: the same chain with every epoch e >= 1 taking its gradients at the
    parameters epoch e - 1 started from (ppo_chain64(stale=True), in float64) lies at least CHAIN_STALE_FACTOR = 10 times the GPU test's
    limit away from the true chain, in that test's metric, on every trunk tensor (here on the heads as well). Also: torch-float32's own
    error on every epoch's statistics stays below the cap / 8, as for the one-epoch cases, and the chain stays finite."""
    d, rows, state, c64, err_t = R.chain_yardstick(case)
    stale = R.ppo_chain64(d, rows, state, R.CHAIN_STEP0, stale=True)
    assert len(c64["params"]) == R.CHAIN_EPOCHS and rows.shape == (R.CHAIN_EPOCHS, case.batch)
    for i, k in enumerate(R.PPO_TENSORS):
        want, w0 = c64["params"][-1][i], d["cur"][i]
        assert np.isfinite(want).all()
        limit = R.chain_limit(err_t[k], want, w0, R.CHAIN_EPOCHS)
        far = R.chain_err(stale["params"][-1][i], want, w0)
        print("chain %-34s %-3s err_t %.3e limit %.3e (floor %.3e) stale %.3e = %.0f limits" % (
            R.case_id(case), k, err_t[k], limit, R.chain_limit(0.0, want, w0, R.CHAIN_EPOCHS), far, far / limit))
        assert far >= R.CHAIN_STALE_FACTOR * limit, (k, far, limit)
    assert set(R.TRUNK_TENSORS) <= set(R.PPO_TENSORS)
    for k, e in err_t.items():
        if " " in k:  # "policy_loss 2": a statistic of an epoch
            assert np.isfinite(e) and 8.0 * e <= R.CAP, (k, e)
    assert (stale["params"][0][0] == c64["params"][0][0]).all()  # epoch 0 has nothing stale to read


def test_ppo_ragged_inputs_give_the_stated_length_patterns():
    case = R.CHAIN_CASES[1]
    lengths = R.ragged_lengths(R.N_ENVS)
    assert set(lengths.tolist()) == {0, 1, 2, 5} and all((lengths == v).sum() == R.N_ENVS // 4 for v in (0, 1, 2, 5))
    assert set(R.ragged_lengths(16).tolist()) == {0, 1, 2, 5} and (R.ragged_lengths(48)[16:32] == R.ragged_lengths(16)).all()  # per member
    d = R.ppo_ragged_inputs(case, R.RAGGED_HORIZON, lengths)
    k0 = R.ENV_CELLS[case.env]
    assert d["states"].shape == (5, 64, k0) and d["states"].dtype == np.int8 and d["actions"].shape == (5, 64) and d["actions"].dtype == np.uint8
    assert d["returns"].shape == (64, 5) and d["returns"].dtype == np.float32 and d["lengths"].dtype == np.int32 and (d["lengths"] == lengths).all()
    assert [p.shape for p in d["cur"]] == [(case.hidden, k0), (case.hidden,), (case.hidden, case.hidden), (case.hidden,), (4, case.hidden), (4,), (1, case.hidden), (1,)]
    assert all(p.dtype == np.float32 and not np.array_equal(p, o) for p, o in zip(d["cur"], d["old"]))
    sparse = R.sparse_lengths()
    s = R.ppo_ragged_inputs(case, R.SPARSE_HORIZON, sparse)
    assert sorted(sparse.tolist()) == [0] * 60 + [16] * 4 and s["actions"].shape == (16, 64)
    valid = np.arange(R.SPARSE_HORIZON)[:, None] < sparse[None, :]
    assert valid.sum() * 16 == valid.size  # exactly one (t, trajectory) candidate in 16 is valid
    assert len({i // 16 for i in np.flatnonzero(sparse)}) == 4  # a full trajectory among every 16 columns
    with pytest.raises(AssertionError):
        R.ppo_ragged_inputs(case, 5, np.zeros(64, dtype=np.int32))  # (an all-zero rollout is no input of these tests)
