"""The fused PPO-CNN learner (sgk_ppo_cnn_epochs: ppo_cnn_forward_kernel, ppo_cnn_backward_kernel, ppo_cnn_adam_kernel) against the
float64 reference of tests/learner_reference.py (ppo_cnn_epoch64), quantity by quantity, with the helpers and bounds of
tests/test_gpu_learner_gradients.py.

(a) one epoch from zero Adam state: m / (1 - beta1) is the kernel's gradient; per tensor err_k = max|g_k - g64| / max|g64| <=
    max(8 err_t, 16 x 2^-23) and <= 1e-5, err_t being torch-float32 autograd's error on the same inputs, every element counted; the
    three statistics by the same rule; v = (1 - beta2) g_k^2 element by element; nothing NaN / Inf; step == 1; the old policy untouched.
(b) Adam from an injected state at step 4999 fed the kernel's own gradient: m', v' and the update against adam64, step == 5000.
(c) two epochs in one call equal two calls of one epoch bit for bit, rows_out included.
(d) the in-kernel draws on a ragged rollout: valid rows, the same rows from the same state, the statistics of exactly those rows.

Inputs (learner_reference.ppo_cnn_inputs): a synthetic rollout of 3 steps x 37 trajectories whose boards hold seeded integers 0..5 in
every cell, the border ring included (a tap over a border cell of the input plane then counts in conv1 and the bottleneck); the old
policy at torch's default initialisation, the current network perturbed away from it so that 31 to 57 of 64 ratios (27 and 28 of 37)
leave 1 +- clipping; rows 0..7 of a minibatch are the four (ratio above / below the range) x (advantage positive / negative) branches
of the clamp's gradient, a ratio inside, the rollout's last row, row 0 and a duplicate. All 21 (board shape, channels) instantiations
at batch 64, batches 2 and 37 at C = 5 and C = 8, one case under the agent's default hyperparameters, one with old == current (the
tie halves).

Measured on an MI355X (profiles/ppo_cnn_gradients/errors.log, printed by tools/learner_gradient_errors.py --cnn): over the 364 gradient
tensors the median err_k / err_t is 1.11; the worst is 216 at DistributionalShift-c5-b64 'grad lvb' (err_k
2.2e-7 against err_t 1.0e-9: torch happened to be nearly exact there; 0.11 of the limit). The gradient closest to its limit is
IslandNavigation-c8-b64 'grad b1' at 0.42 of it (9.3e-7 against 2.2e-6), the statistic closest SafeInterruptibility-c4-b64's policy
loss at 0.37 (7.0e-7 against 1.9e-6); the worst err_k / err_t of a statistic is 420 (FriendFoe-c5-b37's policy loss, 4.6e-7 against an
err_t of 1.1e-9). Of every figure the closest to its limit is step B's update of 'la' at SafeInterruptibility-c4-b64, 0.745 of its
allowance; v, m' and v' stay below 0.2 of theirs. The tie case's policy loss is measured on another scale (cnn_stat_pair: the
reference value is 0, so the error is absolute, over mean |normalised advantage|): 2.6e-8.

profiles/ppo_cnn_gradients/mutations.log: three numerical mutations of csrc/sgk_ppo_cnn.hip, each in a library of its own, against
these 56 tests and the 26 of tests/test_gpu_ppo_cnn_learn.py. inrange forced to 1: 23 of these fail (every gradient case with a batch of
37 or 64 but the tie case), 5 of the earlier ones. The old policy staged from the current parameters: 27 fail (every gradient case but
the tie case, both ragged cases), 10 of the earlier ones. pc_wgrad's (kx - 1) shift dropped for CIN == 1: 26 fail (every gradient case,
on 'grad w1'), 19 of the earlier ones.
"""
import types

import numpy as np
import pytest

import learner_child as LC
import learner_reference as R
import test_gpu_learner_gradients as G

pytestmark = pytest.mark.gpu

F64 = np.float64
STATS = ("policy_loss", "value_loss", "entropy")
RAGGED_STEP = 11  # the Adam step the ragged rollout's draws are keyed by


def _cpu(ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


def _put(dst, arrays):
    import torch

    with torch.no_grad():
        for t, a in zip(dst, arrays):
            t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(t.device).reshape(t.shape))


def _own(agent):
    named = dict(agent.net.named_parameters())
    return [named[k].data for k in agent.CNN_PARAMS]


def _old(agent):
    named = dict(agent.net.old_policy.named_parameters())
    return [named[k].data for k in agent.CNN_PARAMS]


def make_agent(case, env, epochs):
    """A BatchedPPOAgent on the conv learner whose own and old-policy parameters are the case's seeded tensors."""
    import safe_grid_agents_amd as S

    assert tuple(int(v) for v in env.observation_space.shape[-2:]) == R.CNN_SHAPES[case.env]
    args = types.SimpleNamespace(discount=0.99, batch_size=case.batch, rollouts=1, epochs=epochs, n_layers=2, n_hidden=None,
                                 n_channels=case.channels, device=0, log_gradients=False, cheat=False, **R.ppo_cnn_hyper(case))
    agent = S.BatchedPPOAgent(env, args, body="cnn", fused_conv_learn=True)
    assert agent.fused_learn and agent.fused_conv and agent.body == "cnn"
    d = R.ppo_cnn_yardstick(case)[0]
    _put(_old(agent), d["old"])
    _put(_own(agent), d["cur"])
    return agent


def rollout(agent, d, lengths=None):
    import torch

    ro = {k: torch.as_tensor(d[k]).to(agent.device) for k in ("states", "actions", "returns")}
    ro["lengths"] = torch.as_tensor(d["lengths"] if lengths is None else lengths).to(agent.device)
    return types.SimpleNamespace(**ro)


def set_state(agent, ro, params, ms, vs, step):
    if agent._pl is None:
        agent._cnn_learner(ro)  # (allocates Adam's state and the workspace; launches nothing)
    _put(_own(agent), params)
    _put(agent._pl["m"], ms)
    _put(agent._pl["v"], vs)
    agent._pl["step"].fill_(step)


def _open_env(case):
    import safe_grid_agents_amd as S

    env = S.BatchedGridworldEnv(case.env, R.N_ENVS, seed=3)
    env.bind_torch_stream()
    return env


def run_cnn_case(case):
    """The conv learner through step A (zero Adam state) and step B (injected state, step 4999) on the case's seeded rollout."""
    import torch

    d = R.ppo_cnn_yardstick(case)[0]
    env = _open_env(case)
    try:
        agent = make_agent(case, env, 1)
        ro = rollout(agent, d)
        out = {"old_before": _cpu(_old(agent))}
        agent.learn(ro, None, rows=[d["rows"]])  # (every (t, trajectory) pair is valid: the index into the valid pairs is the flat row)
        pl = agent._pl
        out["stats"] = [agent._stats.cpu().numpy()[0].copy()]
        out["m_a"], out["v_a"], out["w_a"], out["step_a"] = _cpu(pl["m"]), _cpu(pl["v"]), _cpu(_own(agent)), [pl["step"].cpu().numpy().copy()]
        out["old_after"] = _cpu(_old(agent))
        g_c = [m.astype(F64) / R.one_minus_beta1() for m in out["m_a"]]
        ms, vs, _ = R.inject_adam_state(g_c, LC.STATE_SEED + case.seed, False)
        set_state(agent, ro, d["cur"], ms, vs, LC.STEP_BEFORE_B)
        agent.learn(ro, None, rows=[d["rows"]])
        out["m_b"], out["v_b"], out["w_b"], out["step_b"] = _cpu(pl["m"]), _cpu(pl["v"]), _cpu(_own(agent)), [pl["step"].cpu().numpy().copy()]
        torch.cuda.synchronize()
    finally:
        env.close()
    return out


def cnn_result(case):
    return G._once(("ppo-cnn", case), lambda: run_cnn_case(case))


def _snapshot(agent):
    pl = agent._pl
    return {"w": _cpu(_own(agent)), "m": _cpu(pl["m"]), "v": _cpu(pl["v"]), "step": [pl["step"].cpu().numpy().copy()]}


def run_plumbing_case(case):
    """(c) and (d) of the module docstring on one case: what the two-epoch call and the two one-epoch calls left, and the ragged
    rollout's two draws with their statistics."""
    import torch

    d, r64, _ = R.ppo_cnn_yardstick(case)
    env = _open_env(case)
    try:
        two, one = make_agent(case, env, 2), make_agent(case, env, 1)
        ro = rollout(one, d)
        ms, vs, _ = R.inject_adam_state(r64["grads"], LC.STATE_SEED + case.seed, False)
        start = (d["cur"], ms, vs, LC.STEP_BEFORE_B)
        out = {}
        rows_out = torch.full((2, case.batch), -1, dtype=torch.int64, device=two.device)
        set_state(two, ro, *start)
        two._learn_fused_cnn(ro, rows=[d["rows"], d["rows2"]], rows_out=rows_out)
        out["two"] = dict(_snapshot(two), stats=two._stats.cpu().numpy().copy(), rows_out=rows_out.cpu().numpy().copy())
        set_state(one, ro, *start)
        stats, used = [], []
        for rows in (d["rows"], d["rows2"]):
            got = torch.full((1, case.batch), -1, dtype=torch.int64, device=one.device)
            one._learn_fused_cnn(ro, rows=[rows], rows_out=got)
            stats.append(one._stats.cpu().numpy()[0].copy())
            used.append(got.cpu().numpy()[0].copy())
        out["one"] = dict(_snapshot(one), stats=np.stack(stats), rows_out=np.stack(used))
        # (d): the kernel's own draws on a ragged rollout, twice from the same state and step
        ragged = rollout(one, d, d["ragged_lengths"])
        zeros = [np.zeros_like(p) for p in d["cur"]]
        out["ragged"] = []
        for _ in range(2):
            got = torch.full((1, case.batch), -1, dtype=torch.int64, device=one.device)
            set_state(one, ragged, d["cur"], zeros, zeros, RAGGED_STEP)
            one._learn_fused_cnn(ragged, rows_out=got)
            out["ragged"].append({"rows": got.cpu().numpy()[0].copy(), "stats": one._stats.cpu().numpy()[0].copy(),
                                  "step": int(one._pl["step"].item())})
        torch.cuda.synchronize()
    finally:
        env.close()
    return out


def plumbing_result(case):
    return G._once(("ppo-cnn plumbing", case), lambda: run_plumbing_case(case))


# ---- figures: (what, measured, limit, err_t), measured <= limit ----------------------------------------------------------------------
def cnn_figures_a(case, out):
    d, r64, err_t = R.ppo_cnn_yardstick(case)
    stats = out["stats"][0]
    return G._figures_a(R.CNN_TENSORS, out, r64["grads"], err_t, [(k,) + R.cnn_stat_pair(case, r64, i, stats[i]) for i, k in enumerate(STATS)])


def cnn_figures_b(case, out):
    state = R.inject_adam_state(G._clipped_gradient(out), LC.STATE_SEED + case.seed, False)
    return G._figures_b(R.CNN_TENSORS, R.ppo_cnn_yardstick(case)[0]["cur"], out, state, R.ppo_cnn_hyper(case)["lr"])


def ragged_figures(case, res):
    """The statistics of the ragged rollout's epoch against ppo_cnn_epoch64 on exactly the rows the kernel drew (err_t: the same
    function in float32 on those rows)."""
    import torch

    d = R.ppo_cnn_yardstick(case)[0]
    h = R.ppo_cnn_hyper(case)
    kw = {k: h[k] for k in ("clipping", "critic_coeff", "entropy_bonus")}
    args = (d["cur"], d["old"][:10]) + R.ppo_cnn_gather(d, res["rows"])
    r64, r32 = R.ppo_cnn_epoch64(*args, **kw), R.ppo_cnn_epoch64(*args, dtype=torch.float32, **kw)
    figs = []
    for i, k in enumerate(STATS):
        err_t = R.cnn_stat_err(case, r64, i, r32["stats"][i])
        figs.append((k, R.cnn_stat_err(case, r64, i, float(res["stats"][i])), R.bound(err_t), err_t))
    return figs


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PPO_CNN_CASES, ids=R.cnn_case_id)
def test_cnn_learner_gradients_and_statistics_against_float64(case):
    out = cnn_result(case)
    G._finite(out, ("m_a", "v_a", "w_a", "stats"))
    assert int(out["step_a"][0][0]) == 1
    for k, a, b in zip(R.CNN_TENSORS, out["old_before"], out["old_after"]):
        assert a.tobytes() == b.tobytes(), k  # the old policy, bit for bit
    for k, a, b in zip(R.CNN_TENSORS, out["old_before"], R.ppo_cnn_yardstick(case)[0]["old"]):
        assert (a.reshape(b.shape) == b).all(), k
    G._check(cnn_figures_a(case, out))


@pytest.mark.parametrize("case", R.PPO_CNN_CASES, ids=R.cnn_case_id)
def test_cnn_learner_adam_from_injected_state(case):
    out = cnn_result(case)
    G._finite(out, ("m_b", "v_b", "w_b"))
    assert int(out["step_b"][0][0]) == LC.STEP_BEFORE_B + 1
    G._check(cnn_figures_b(case, out))


@pytest.mark.parametrize("case", R.PLUMBING_CASES, ids=R.cnn_case_id)
def test_two_epochs_in_one_call_equal_two_calls_of_one_epoch_bit_for_bit(case):
    """n_epochs = 2 on rows [r0, r1] against n_epochs = 1 on r0, then on r1, from the same parameters, Adam state and step 4999: all 14
    parameters, m, v, the step counter and both rows of the statistics are identical, and rows_out holds [r0, r1]."""
    d = R.ppo_cnn_yardstick(case)[0]
    res = plumbing_result(case)
    two, one = res["two"], res["one"]
    for key in ("w", "m", "v", "step"):
        for k, a, b in zip(R.CNN_TENSORS, two[key], one[key]):
            assert np.isfinite(a).all() and a.tobytes() == b.tobytes(), (key, k)
    assert int(two["step"][0][0]) == LC.STEP_BEFORE_B + 2
    assert np.isfinite(two["stats"]).all() and two["stats"].tobytes() == one["stats"].tobytes()
    assert not (two["stats"][0] == two["stats"][1]).all()  # (two different epochs)
    want = np.stack([d["rows"], d["rows2"]])
    assert (two["rows_out"] == want).all() and (one["rows_out"] == want).all()
    assert any((a != b).any() for a, b in zip(two["w"], d["cur"]))


@pytest.mark.parametrize("case", R.PLUMBING_CASES, ids=R.cnn_case_id)
def test_in_kernel_draws_on_a_ragged_rollout(case):
    """T = 3, N = 37, lengths a seeded mix of 0..3 (a third or more of the pairs valid, a trajectory of length 0 among them), rows=None:
    every drawn row is a valid pair, the same state and step draw the same rows, and the statistics are those of exactly these rows."""
    d = R.ppo_cnn_yardstick(case)[0]
    first, second = plumbing_result(case)["ragged"]
    lengths = d["ragged_lengths"]
    assert (lengths == 0).any() and 3 * int(lengths.sum()) >= R.CNN_T * R.CNN_N
    rows = first["rows"]
    assert rows.shape == (case.batch,) and (rows >= 0).all() and (rows < R.CNN_T * R.CNN_N).all()
    t, n = rows // R.CNN_N, rows % R.CNN_N
    assert (t < lengths[n]).all()
    assert len(np.unique(rows)) > case.batch // 4  # (draws, not a constant)
    assert (second["rows"] == rows).all() and second["stats"].tobytes() == first["stats"].tobytes()
    assert first["step"] == second["step"] == RAGGED_STEP + 1
    assert np.isfinite(first["stats"]).all()
    G._check(ragged_figures(case, first))
