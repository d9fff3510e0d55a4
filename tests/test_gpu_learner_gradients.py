"""The two fused MLP learners (sgk_dqn_sgd_step: dqn_sgd_kernel + dqn_adam_kernel / dqn_adam_reset_kernel; sgk_ppo_epochs:
ppo_epochs_kernel) against the float64 references of tests/learner_reference.py, quantity by quantity instead of through the weights
after a few Adam steps (Adam's first steps move every element by ~lr g/|g|: a gradient tensor off by a constant factor -- a wrong 1/B, a
wrong clip coefficient, a bias gradient counted twice -- gives the same weights).

(a) gradients: one step from zero Adam state leaves m = (1 - beta1) coef g, so m / (1 - beta1) is the kernel's clipped gradient; per
    tensor err_k = max|g_k - coef64 g64| / max|g64| <= max(8 err_t, 16 x 2^-23) and <= 1e-5, err_t being torch-float32 autograd's error
    on the same inputs (tests/test_learner_reference_cpu.py keeps 8 err_t below the cap); the loss / the three PPO statistics by the same
    rule; v = (1 - beta2) g_k^2 element by element (rtol 1e-6; + 2^-126 absolute: squares of gradients below 1e-19 leave float32's normal
    range), nothing NaN / Inf: a padded row or column leaking into a live parameter shows here.
(b) Adam from an injected state at step 4999 (learner_reference.inject_adam_state: vmax = v x {0.5, 2}, so amsgrad's maximum is a real
    choice in both directions in every tensor), fed the kernel's own clipped gradient: m', v', vmax' (1e-6 relative; m' relative to
    its operands, see m_scale) and the update (4e-6 |dw| + 2^-23 |w|) against adam64, the step counter, the transposed copies, and the
    same step through sgk_dqn_sgd_step_reset_store bit for bit.
(c) the same for the non-default in-kernel Adam (SGK_DQN_ONE_LAUNCH=1, read when the library is loaded: a fresh child process,
    tests/learner_child.py) against float64 and against this process's two-launch results.

Shapes: 64 envs, a replay ring / rollout of 2 slices, every board size K0 in {25, 30, 36, 48, 49, 56, 63} (W1T = K0 % 4 == 0 selects
another ownership layout of W1) x {64, 100} hidden units, batches 1 / 2 / 17 / 33 / 64, gradients clipped (norm > 20) and not (< 5), both
DQN loss modes.

Measured on an MI355X (profiles/learner_gradients/errors.log, printed by tools/learner_gradient_errors.py): over the 324 gradient tensors
the median err_k / err_t is 1.13; the worst err_k / err_t is 67.45 (PPO FriendFoe, 100 units, batch 64, the critic bias: err_k 4.1e-7 where
torch-float32 happens to be within 6.0e-9 -- the 16-ulp floor of the limit is for this); the figure closest to its limit is the policy loss
of PPO SafeInterruptibility, 64 units, batch 2: err_k 1.70e-6 = 6.15 err_t against 8 err_t. Step B: m' would miss 1e-6 |m'| in 47 of 180
DQN tensors, by up to 252 times (the "m'/|m'|" lines), and stays within 1e-6 m_scale everywhere. The one-launch form was bit-identical
to the two-launch form in all five cases. profiles/learner_gradients/mutations.log: three mutations of the kernels against these tests.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import learner_child as LC
import learner_reference as R

pytestmark = pytest.mark.gpu

F64 = np.float64
TINY = 2.0 ** -126  # float32's smallest normal number
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dqn_result(case):
    return _once(("dqn", case), lambda: LC.run_dqn_case(case, reset_store=case == R.RESET_STORE_CASE))


def run_ppo_case(case):
    """The PPO learner through step A (zero Adam state) and step B (injected state, step 4999) on the case's seeded rollout."""
    import torch

    import safe_grid_agents_amd as S

    d = R.ppo_yardstick(case)[0]
    env = S.BatchedGridworldEnv(case.env, R.N_ENVS, seed=3)
    env.bind_torch_stream()
    assert env.n_cells == R.ENV_CELLS[case.env]
    args = types.SimpleNamespace(discount=0.99, batch_size=case.batch, rollouts=1, epochs=1, n_layers=2, n_hidden=case.hidden, n_channels=5,
                                 device=0, log_gradients=False, cheat=False, **R.PPO_HYPER)
    agent = S.BatchedPPOAgent(env, args)
    assert agent.fused_learn and agent.body == "mlp"
    dev = agent.device
    own, old = agent._own_tensors(), agent.net.old_policy
    l1, l2 = old.network[0][0], old.network[1][0][0]
    cpu = lambda ts: [t.detach().cpu().numpy().copy() for t in ts]  # noqa: E731

    def put(dst, arrays):
        with torch.no_grad():
            for t, a in zip(dst, arrays):
                t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(dev))

    put([l1.weight.data, l1.bias.data, l2.weight.data, l2.bias.data, old.actor.weight.data, old.actor.bias.data], d["old"][:6])
    ro = types.SimpleNamespace(**{k: torch.as_tensor(d[k]).to(dev) for k in ("states", "actions", "returns", "lengths")})
    out = {}
    put(own, d["cur"])
    agent.learn(ro, None, rows=[d["rows"]])  # (every (t, env) pair is valid: the index into the valid pairs is the flat row t * N + env)
    pl = agent._pl
    out["stats"] = [agent._stats.cpu().numpy()[0].copy()]
    out["m_a"], out["v_a"], out["w_a"], out["step_a"] = cpu(pl["m"]), cpu(pl["v"]), cpu(own), [pl["step"].cpu().numpy().copy()]
    g_c = [m.astype(F64) / R.one_minus_beta1() for m in out["m_a"]]
    ms, vs, _ = R.inject_adam_state(g_c, LC.STATE_SEED + case.seed, False)
    put(own, d["cur"])  # (the learner refreshes its transposed copies from the parameters itself)
    put(pl["m"], ms)
    put(pl["v"], vs)
    pl["step"].fill_(LC.STEP_BEFORE_B)
    agent.learn(ro, None, rows=[d["rows"]])
    out["m_b"], out["v_b"], out["w_b"], out["step_b"] = cpu(pl["m"]), cpu(pl["v"]), cpu(own), [pl["step"].cpu().numpy().copy()]
    out["w1t"], out["w2t"] = cpu([pl["w1t"]]), cpu([pl["w2t"]])
    torch.cuda.synchronize()
    env.close()
    return out


def ppo_result(case):
    return _once(("ppo", case), lambda: run_ppo_case(case))


# ---- figures: (what, measured, limit), measured <= limit ------------------------------------------------------------------------------
def _clipped_gradient(out):
    return [m.astype(F64) / R.one_minus_beta1() for m in out["m_a"]]


def _figures_a(names, out, want, err_t, scalars):
    """Step A. want: the float64 (clipped) gradients; scalars: [(name, kernel's value, float64 value)]."""
    figs = []
    g = _clipped_gradient(out)
    for k, gk, g64, v in zip(names, g, want, out["v_a"]):
        figs.append(("grad " + k, R.rel_err(gk, g64), R.bound(err_t[k]), err_t[k]))
        want_v = R.one_minus_beta2() * gk * gk
        figs.append(("v " + k, float((np.abs(v - want_v) / (1e-6 * want_v + TINY)).max()), 1.0, None))
    for k, got, ref in scalars:
        figs.append((k, R.rel_err(got, ref), R.bound(err_t[k]), err_t[k]))
    return figs


def m_scale(m0, g_c):
    """What the roundings of m' = m + (1 - beta1) (g - m) are relative to: |m| + (1 - beta1) |g - m|. It equals |m'| where the two terms
    have one sign; where they cancel (m ~ -g / 9: a few elements of every seeded tensor) even an exactly rounded float32 evaluation is
    off by far more than 1e-6 |m'| (tests/test_learner_reference_cpu.py shows it), so "rtol 1e-6 on m'" is taken against this scale."""
    return np.abs(m0.astype(F64)) + R.one_minus_beta1() * np.abs(g_c - m0.astype(F64))


def _figures_b(names, w0s, out, state, lr):
    """Step B against adam64 fed the kernel's own clipped gradient. v', vmax': |got - ref| <= 1e-6 |ref| (+ 2^-126); m': <= 1e-6 m_scale;
    the update: |dw - dw_ref| <= 4e-6 |dw_ref| + 2^-23 |w|. Each figure is the worst element's error over its allowance (limit 1)."""
    figs = []
    ms, vs, xs = state
    for i, k in enumerate(names):
        w0, g_c = w0s[i].astype(F64), _clipped_gradient(out)[i]
        w_ref, m_ref, v_ref, x_ref = R.adam64(w0, ms[i], vs[i], None if xs is None else xs[i], g_c, LC.STEP_BEFORE_B + 1, lr)
        figs.append(("m' " + k, float((np.abs(out["m_b"][i] - m_ref) / (1e-6 * m_scale(ms[i], g_c) + TINY)).max()), 1.0, None))
        for what, got, ref in [("v'", out["v_b"][i], v_ref)] + ([("vmax'", out["x_b"][i], x_ref)] if xs is not None else []):
            figs.append(("%s %s" % (what, k), float((np.abs(got - ref) / (1e-6 * np.abs(ref) + TINY)).max()), 1.0, None))
        dw, dw_ref = out["w_b"][i].astype(F64) - w0, w_ref - w0
        figs.append(("update " + k, float((np.abs(dw - dw_ref) / (4e-6 * np.abs(dw_ref) + R.ULP * np.abs(w0) + TINY)).max()), 1.0, None))
    return figs


def _check(figs):
    bad = [f[:3] for f in figs if not f[1] <= f[2]]
    assert not bad, bad


def _finite(out, keys):
    for key in keys:
        for a in out[key]:
            assert np.isfinite(a).all(), key


def dqn_figures_a(case, out):
    d, r64, err_t = R.dqn_yardstick(case)
    return _figures_a(R.DQN_TENSORS, out, r64["clipped_grads"], err_t, [("loss", float(out["loss"][0][0]), r64["loss"])])


def dqn_state(case, out):
    return R.inject_adam_state(_clipped_gradient(out), LC.STATE_SEED + case.seed, True)


def dqn_figures_b(case, out):
    return _figures_b(R.DQN_TENSORS, R.dqn_yardstick(case)[0]["q"], out, dqn_state(case, out), R.DQN_LR)


def dqn_checks_a(case, out):
    _finite(out, ("m_a", "v_a", "x_a", "w_a"))
    assert int(out["step_a"][0][0]) == 1
    for v, x in zip(out["v_a"], out["x_a"]):
        assert (v == x).all()  # max(0, v)
    _check(dqn_figures_a(case, out))


def dqn_checks_b(case, out):
    _finite(out, ("m_b", "v_b", "x_b", "w_b"))
    assert int(out["step_b"][0][0]) == LC.STEP_BEFORE_B + 1
    ms, vs, xs = dqn_state(case, out)
    for k, x0, v1 in zip(R.DQN_TENSORS, xs, out["v_b"]):
        grew = v1 > x0  # amsgrad's maximum takes the new v here and keeps vmax elsewhere: both happen in every tensor
        assert grew.any() and not grew.all(), k
    _check(dqn_figures_b(case, out))
    w1, w2, w3 = out["w_b"][0], out["w_b"][2], out["w_b"][4]
    assert (out["w1t"][0] == w1.T).all() and (out["w2t"][0] == w2.T).all() and (out["w3t"][0] == w3.T).all()


def ppo_figures_a(case, out):
    d, r64, err_t = R.ppo_yardstick(case)
    stats = out["stats"][0]
    return _figures_a(R.PPO_TENSORS, out, r64["grads"], err_t,
                      [(k, float(stats[i]), r64["stats"][i]) for i, k in enumerate(("policy_loss", "value_loss", "entropy"))])


def ppo_figures_b(case, out):
    state = R.inject_adam_state(_clipped_gradient(out), LC.STATE_SEED + case.seed, False)
    return _figures_b(R.PPO_TENSORS, R.ppo_yardstick(case)[0]["cur"], out, state, R.PPO_HYPER["lr"])


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DQN_CASES, ids=R.case_id)
def test_dqn_learner_gradients_and_loss_against_float64(case):
    dqn_checks_a(case, dqn_result(case))


@pytest.mark.parametrize("case", R.DQN_CASES, ids=R.case_id)
def test_dqn_learner_adam_amsgrad_from_injected_state(case):
    dqn_checks_b(case, dqn_result(case))


def test_dqn_adam_in_the_reset_store_launch_is_bit_equal_to_the_two_calls():
    """sgk_dqn_sgd_step_reset_store (dqn_adam_reset_kernel) on step B of (Sokoban, 100 units, batch 64): m', v', vmax', w' and the step."""
    out = dqn_result(R.RESET_STORE_CASE)
    for a, b in (("m_r", "m_b"), ("v_r", "v_b"), ("x_r", "x_b"), ("w_r", "w_b"), ("step_r", "step_b")):
        for x, y in zip(out[a], out[b]):
            assert (x == y).all(), a


@pytest.mark.parametrize("case", R.PPO_CASES, ids=R.case_id)
def test_ppo_learner_gradients_and_statistics_against_float64(case):
    out = ppo_result(case)
    ratio = R.ppo_yardstick(case)[1]["ratio"]
    assert ((ratio < 1 - R.PPO_HYPER["clipping"]) | (ratio > 1 + R.PPO_HYPER["clipping"])).any()  # the clamp branch of the gradient
    _finite(out, ("m_a", "v_a", "w_a", "stats"))
    assert int(out["step_a"][0][0]) == 1
    _check(ppo_figures_a(case, out))


@pytest.mark.parametrize("case", R.PPO_CASES, ids=R.case_id)
def test_ppo_learner_adam_from_injected_state(case):
    out = ppo_result(case)
    _finite(out, ("m_b", "v_b", "w_b"))
    assert int(out["step_b"][0][0]) == LC.STEP_BEFORE_B + 1
    _check(ppo_figures_b(case, out))
    assert (out["w1t"][0] == out["w_b"][0].T).all() and (out["w2t"][0] == out["w_b"][2].T).all()


def one_launch_results(path):
    """tests/learner_child.py in a fresh process with SGK_DQN_ONE_LAUNCH=1: its results for learner_reference.CHILD_CASES."""
    env = dict(os.environ, SGK_DQN_ONE_LAUNCH="1")
    p = subprocess.run([sys.executable, os.path.join(LC.HERE, "learner_child.py"), str(path)], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return LC.unpack(np.load(str(path)))


def one_launch_figures_vs_two_launches(case, child, parent):
    """The in-kernel Adam against the two-launch form on the same inputs, within (b)'s allowances."""
    figs = []
    ms = dqn_state(case, parent)[0]
    for i, k in enumerate(R.DQN_TENSORS):
        g_c = _clipped_gradient(parent)[i]
        for what, scale in (("m_a", np.abs(parent["m_a"][i])), ("m_b", m_scale(ms[i], g_c)), ("v_b", np.abs(parent["v_b"][i])), ("x_b", np.abs(parent["x_b"][i]))):
            a, b = child[what][i].astype(F64), parent[what][i].astype(F64)
            figs.append(("%s %s" % (what, k), float((np.abs(a - b) / (1e-6 * scale + TINY)).max()), 1.0, None))
        w0 = R.dqn_yardstick(case)[0]["q"][i].astype(F64)
        da, db = child["w_b"][i].astype(F64) - w0, parent["w_b"][i].astype(F64) - w0
        figs.append(("update " + k, float((np.abs(da - db) / (4e-6 * np.abs(db) + R.ULP * np.abs(w0) + TINY)).max()), 1.0, None))
    a, b = float(child["loss"][0][0]), float(parent["loss"][0][0])
    figs.append(("loss", abs(a - b) / abs(b), 1e-6, None))
    return figs


def bit_identical(child, parent):
    return all((x == y).all() for key in ("loss", "m_a", "v_a", "w_a", "m_b", "v_b", "x_b", "w_b") for x, y in zip(child[key], parent[key]))


def test_dqn_one_launch_adam_meets_the_same_bounds_and_agrees_with_two_launches(tmp_path):
    """dqn_sgd_kernel's own Adam (its quad_ref ownership code; SGK_DQN_ONE_LAUNCH=1, non-default since the two-launch form): the child's
    gradients, loss, m', v', vmax', updates, step counters and transposed copies meet (a)'s and (b)'s float64 bounds, and agree with this
    process's two-launch results within (b)'s allowances. (Bit-identity of the two forms is printed by tools/learner_gradient_errors.py
    and not asserted: the compiler may contract the two inlined copies of adam_scalar differently.)"""
    results = one_launch_results(tmp_path / "one_launch.npz")
    assert len(results) == len(R.CHILD_CASES)
    for case, child in zip(R.CHILD_CASES, results):
        dqn_checks_a(case, child)
        dqn_checks_b(case, child)
        _check(one_launch_figures_vs_two_launches(case, child, dqn_result(case)))
