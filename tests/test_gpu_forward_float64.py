"""The fused ACTING forwards against float64 (tests/forward_reference.py): policy_mfma_kernel (sgk_policy_act, sgk_policy_sample),
convq_act_kernel (sgk_convq_act, sgk_convq_sample) and the rollout kernels (sgk_policy_rollout, sgk_policy_rollout_members,
sgk_convq_rollout). The older forward tests compare with torch-float32 at rtol / atol 1e-4; here

  (a) the scores of both per-step kernels of a body, on the level's boards after 17 random steps, for all seven board sizes x three widths x
      both layouts: with "integer" weights they EQUAL the float64 scores (float32 is exact there: every partial sum is an integer below
      2^24, tests/test_forward_reference_cpu.py), with "real" weights err_k = max|got - s64| / max|s64| <= learner_reference.bound(err_t),
      err_t being torch-float32's figure on the CPU; the greedy action is the float64 argmax on every env whose top-2 gap is above
      4 bound max|s64|, and on EVERY env of an integer case, exact ties included (the first maximum wins);
  (b) the same on painted boards -- every cell a seeded value 0 .. 7, written through env.boards(): on a level's own boards the wall ring
      is 0, so a first-layer column or a window tap at a row end is otherwise multiplied by zero in every test;
  (c) the same, exact, at sizes that take a second grid-stride pass (test_a_second_grid_stride_pass_... derives them);
  (d) the rollout kernels: for every step k and env, actions[k] is the float64 argmax of the forward on states[k], the board the kernel
      reports to have acted on -- for one policy, for three members with different weights, and for the conv body.

Every launch writes into over-allocated outputs whose tails hold a sentinel: nothing past env n - 1 is written.
Measured on an MI355X (profiles/forward_float64/errors.log, tools/forward_errors.py): all 118 integer cases equal float64 on every env;
over the 168 figures of the real cases the median err_k / err_t is 1.00 (MLP 1.13, conv body 0.90) and the worst 1.84 (sgk_policy_act,
Sokoban, 64 units, pitched: 1.8e-7 against torch's 1.0e-7); the figure closest to its limit is at 0.22 of it (FriendFoe, 100 units,
pitched) -- the kernels' k-ordered fp32 chains are as good as torch-float32's sums, and the rule's factor of 8 is not used up anywhere.
Seven value-only mutations of the kernels, the tests each fails and what the older forward tests say to them:
profiles/forward_float64/mutations.log."""
import functools

import numpy as np
import pytest

import forward_reference as FR
import learner_reference as R
import safe_grid_agents_amd as S

pytestmark = pytest.mark.gpu

SENTINEL, ACTION_SENTINEL, PAD = -12345.0, 99, 259


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def mlp_dict(w):
    """The dict env.policy_act takes, from torch-layout arrays: w1t = W1^T [cells, H], w3t = W3^T [H, 4]."""
    return {"w1t": _dev(w[0].T), "b1": _dev(w[1]), "w2": _dev(w[2]), "b2": _dev(w[3]), "w3t": _dev(w[4].T), "b3": _dev(w[5])}


def member_dict(ws):
    """Stacked on a leading member axis (env.policy_rollout_members)."""
    one = [mlp_dict(w) for w in ws]
    import torch

    return {k: torch.stack([d[k] for d in one]).contiguous() for k in one[0]}


def cnn_dict(w):
    return {k: _dev(p) for k, p in zip(("w1", "b1", "w2", "b2", "wb", "bb", "wh", "bh", "wl", "bl"), w)}


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count  # what the library's n_cus is (csrc/sgk_api.hip)


def case_cus(case):
    return _cus() if case.size == "multi" else FR.DEFAULT_CUS


@functools.lru_cache(maxsize=None)
def kernel_result(case):
    """Both per-step kernels of the case's body on the case's boards: {"boards" (what the env held), "act" / "sample" (the scores /
    logits [n, 4]), "greedy", "sampled" (the actions [n]), "tails_untouched"}; once per process (tools/forward_errors.py reads it too)."""
    import torch

    y = FR.yardstick(case, case_cus(case))
    n = len(y["boards"])
    env = S.BatchedGridworldEnv(case.env, n, seed=case.seed, layout=case.layout)
    try:
        env.step_random(FR.STEPS, auto_reset=True)
        if case.size == "painted":
            env.boards().copy_(_dev(y["boards"]).reshape(n, 1, env.H, env.W))
        out = {"boards": env.boards_host().reshape(n, -1)}
        scores = [torch.full((n + PAD, 4), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in range(2)]
        actions = [torch.full((n + PAD,), ACTION_SENTINEL, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        if case.body == "mlp":
            w = mlp_dict(y["weights"])
            env.policy_act(w, 0.0, 3, out=actions[0][:n], scores_out=scores[0][:n])
            env.policy_sample(w, 3, out=actions[1][:n], logits_out=scores[1][:n])
        else:
            w = cnn_dict(y["weights"])
            env.convq_act(w, 0.0, 3, case.width, out=actions[0][:n], scores_out=scores[0][:n])
            env.convq_sample(w, 3, case.width, out=actions[1][:n], logits_out=scores[1][:n])
        torch.cuda.synchronize()
        s, a = [t.cpu().numpy() for t in scores], [t.cpu().numpy() for t in actions]
    finally:
        env.close()
    out.update(act=s[0][:n], sample=s[1][:n], greedy=a[0][:n], sampled=a[1][:n],
               tails_untouched=all((t[n:] == SENTINEL).all() for t in s) and all((t[n:] == ACTION_SENTINEL).all() for t in a))
    return out


def figures(case):
    """(kernel, err_k, err_t, limit) of both kernels of a "real" case."""
    y, out = FR.yardstick(case, case_cus(case)), kernel_result(case)
    return [(k, R.rel_err(out[k], y["s64"]), y["err_t"], y["bound"]) for k in ("act", "sample")]


def _check(case):
    y, out = FR.yardstick(case, case_cus(case)), kernel_result(case)
    assert np.array_equal(out["boards"], y["boards"]), "the env's boards are not the case's"
    assert out["tails_untouched"], "scores or actions of envs >= n were written"
    for k in ("act", "sample"):
        assert np.isfinite(out[k]).all(), k
    if case.family == "integer":
        for k in ("act", "sample"):
            wrong = np.flatnonzero((out[k] != y["s64"]).any(axis=1))
            assert np.array_equal(out[k], y["s64"]), (k, len(wrong), wrong[:8], out[k][wrong[:2]], y["s64"][wrong[:2]])
    else:
        for k, err_k, err_t, limit in figures(case):
            print("%s %s err_k %.3e err_t %.3e err_k/err_t %.2f limit %.3e" % (FR.case_id(case), k, err_k, err_t, err_k / err_t, limit))
            assert err_k <= limit, (k, err_k, err_t, limit)
    clear = y["clear"]
    assert (out["greedy"][clear] == y["argmax"][clear]).all(), np.flatnonzero(out["greedy"] != y["argmax"])[:8]
    assert out["sampled"].max() <= 3


@pytest.mark.parametrize("case", FR.SMALL_CASES, ids=FR.case_id)
def test_per_step_scores_against_float64(case):
    """(a): 161 envs for the MLP (one full 128-env tile, one full wave, one env alone in a 16-env MFMA tile), 2 ENVS + 1 for the conv body
    (two full passes of one workgroup each and a partial one)."""
    _check(case)


@pytest.mark.parametrize("case", FR.PAINTED_CASES, ids=FR.case_id)
def test_per_step_scores_on_painted_boards_are_exact(case):
    """(b): every cell of every board non-zero somewhere in the batch (asserted on the CPU), integer weights, equality."""
    _check(case)


@pytest.mark.parametrize("case", FR.MULTI_CASES, ids=FR.case_id)
def test_a_second_grid_stride_pass_is_exact_and_stops_at_n(case):
    """(c). launch_policy_act (csrc/sgk_policy.hip) starts grid_for(ceil(n / 128), n_cus) = min(tiles, n_cus) workgroups, each taking the
    tiles blockIdx.x, blockIdx.x + grid, ...: with n = 128 (cus + 3) + 37 there are cus + 4 tiles, so workgroups 0 .. 3 run a second pass
    -- the board tile fetched into the other LDS buffer during the first (compact) or gathered at the pitch (pitched), W2 / W3 not
    committed again -- and the last tile holds 37 envs: one full wave and five envs of the next.
    launch_convq_act (csrc/sgk_convq.hip) starts min(passes, n_cus x per_cu) workgroups with per_cu <= 4 (CQ_WAVES_FOR: 3 with five
    channels); a pass is ENVS = 512 // (H (W + 1)) envs (ConvQGeom): with n = ENVS (4 cus + 5) + 3 there are 4 cus + 6 passes, above the
    grid for every channel count, so at least six workgroups run a second pass (three waves write its boards into plane 0 while wave 0
    still sums the first pass's per-slot products) and the last pass holds 3 envs.
    Integer weights: every env of every pass is compared exactly; the sentinel tails show that envs >= n were left alone."""
    cus, n = _cus(), FR.case_n(case, _cus())
    if case.body == "mlp":
        assert -(-n // FR.MLP_ENVS) == cus + 4 and n % FR.MLP_ENVS == 37
    else:
        envs = FR.conv_envs_per_pass(*R.CNN_SHAPES[case.env])
        assert -(-n // envs) == 4 * cus + 6 and n % envs == 3
    assert len(kernel_result(case)["greedy"]) == n
    _check(case)


# ---- (d) the rollout kernels ---------------------------------------------------------------------------------------------------------
def _rollout_buffers(n, cells):
    import torch

    T = FR.ROLLOUT_T
    return (torch.full((T, n, cells), 77, dtype=torch.int8, device="cuda:0"), torch.full((T, n), 9, dtype=torch.uint8, device="cuda:0"),
            torch.full((T, n, 4), 5, dtype=torch.int8, device="cuda:0"))


def _check_rollout(case, launch):
    """Every step's action against the float64 forward on that step's reported board, per policy of the case. The boards must keep the
    integer weights exact and differ between steps, some episode must have ended inside the rollout, and every policy must have taken
    more than one action (what the seeds were chosen for on the CPU: forward_reference.rollout_seed_ok)."""
    import torch

    shape, weights = FR.ROLLOUT_LEVELS[case.level], FR.rollout_weights(case)
    cells, n, body = shape[0] * shape[1], weights[-1][1], FR.rollout_body(case)
    env = S.BatchedGridworldEnv(case.level, n, seed=FR.ROLLOUT_ENV_SEED)
    try:
        env.step_random(FR.ROLLOUT_STEPS_BEFORE, auto_reset=True)
        states, actions, recs = _rollout_buffers(n, cells)
        launch(env, weights, dict(mode="greedy", epsilon=0.0, draw_index0=5, auto_reset=True, states=states, actions=actions, recs=recs))
        torch.cuda.synchronize()
        states, actions, recs = states.cpu().numpy(), actions.cpu().numpy(), recs.cpu().numpy()
    finally:
        env.close()
    for k in range(FR.ROLLOUT_T):
        for lo, hi, w in weights:
            boards = states[k, lo:hi]
            assert boards.min() >= 0 and FR.abs_sum_bound(body, boards, w, shape) < FR.EXACT_LIMIT
            want = FR.forward(body, boards, w, shape).argmax(1)
            got = actions[k, lo:hi]
            assert np.array_equal(got, want), (k, lo, np.flatnonzero(got != want)[:8])
    assert (states[0] != states[-1]).any() and (recs[:, :, 2] != 0).any()
    for lo, hi, _ in weights:
        assert len(np.unique(actions[:, lo:hi])) >= 2, (lo, np.unique(actions[:, lo:hi]))
    return states, actions


def _rollout_cases(kind):
    return [c for c in FR.ROLLOUT_CASES if c.kind == kind]


@pytest.mark.parametrize("case", _rollout_cases("policy"), ids=FR.rollout_case_id)
def test_policy_rollout_takes_the_float64_argmax_on_the_board_it_reports(case):
    """sgk_policy_rollout stages its weights with code of its own ("staged once per launch, so plainly") and redraws its LDS rows from
    the state words: greedy, epsilon 0, 6 steps with auto-reset from boards 97 random steps into their episodes (the 100-step limit
    falls inside the rollout), integer weights, 161 envs; three levels (a second sprite, two backdrops, cells that change by
    themselves) x three hidden widths."""
    _check_rollout(case, lambda env, weights, kw: env.policy_rollout(mlp_dict(weights[0][2]), FR.ROLLOUT_T, **kw))


@pytest.mark.parametrize("case", _rollout_cases("members"), ids=FR.rollout_case_id)
def test_policy_rollout_members_act_with_their_own_weights(case):
    """sgk_policy_rollout_members: three members of 43 envs, each with DIFFERENT integer weights: a wrong member slice of any of the six
    stacked tensors shows as another policy's action (the next member's weights disagree with the action taken in more than a tenth of
    the first step's envs)."""
    states, actions = _check_rollout(case, lambda env, weights, kw: env.policy_rollout_members(member_dict([w for _, _, w in weights]), FR.MEMBERS,
                                                                                              FR.ROLLOUT_T, **kw))
    assert FR.members_disagree(case, states[0], actions[0]) > 0.1


@pytest.mark.parametrize("case", _rollout_cases("convq"), ids=FR.rollout_case_id)
def test_convq_rollout_takes_the_float64_argmax_on_the_board_it_reports(case):
    """sgk_convq_rollout (weights through cq_setup, boards as int8 rows in LDS turned into plane 0 every step), greedy, as above; 161 envs
    are 7 to 23 passes, the last one partial."""
    _check_rollout(case, lambda env, weights, kw: env.convq_rollout(cnn_dict(weights[0][2]), FR.ROLLOUT_T, case.width, **kw))
