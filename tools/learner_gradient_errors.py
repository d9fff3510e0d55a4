"""Prints what tests/test_gpu_learner_gradients.py measures, per case and quantity: the float64 reference's gradient norm and clip
coefficient, err_k (kernel against float64), err_t (torch-float32 against float64) and the limit for step A; the worst element's error
over its allowance for step B; the one-launch child against float64 and against the two-launch form. -> profiles/learner_gradients/errors.log"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "safe-grid-agents_amd")]
import learner_reference as R  # noqa: E402
import test_gpu_learner_gradients as T  # noqa: E402


worst = [0.0, ""]  # the largest err_k / err_t and where


def show(tag, figs):
    for what, got, limit, err_t in figs:
        if err_t is not None and got / err_t > worst[0]:
            worst[:] = [got / err_t, "%s %s (err_k %.3e, err_t %.3e)" % (tag, what, got, err_t)]
        print("%-58s %-18s %.3e  limit %.3e%s%s" % (tag, what, got, limit, "" if err_t is None else "  err_t %.3e  err_k/err_t %.2f" % (err_t, got / max(err_t, 1e-300)),
                                                    "" if got <= limit else "  ABOVE"), flush=True)


# the CPU side first (all that `--cpu` prints): the float64 norms and torch-float32's own error err_t per case and quantity
for c in R.DQN_CASES:
    _, r64, err_t = R.dqn_yardstick(c)
    print("yardstick dqn %-54s float64 norm %.4f coef %.6f  err_t " % (R.case_id(c), r64["norm"], r64["coef"]) + " ".join("%s %.2e" % kv for kv in err_t.items()))
for c in R.PPO_CASES:
    print("yardstick ppo %-54s err_t " % R.case_id(c) + " ".join("%s %.2e" % kv for kv in R.ppo_yardstick(c)[2].items()))
if "--cpu" in sys.argv:
    sys.exit(0)


def m_stated(tag, names, out, state, w0s, lr):
    """m' against 1e-6 |m'| (the bound as first stated, which cancellation in m + (1 - beta1)(g - m) makes unreachable): for the record"""
    for i, k in enumerate(names):
        ref = R.adam64(w0s[i], state[0][i], state[1][i], None, T._clipped_gradient(out)[i], T.LC.STEP_BEFORE_B + 1, lr)[1]
        worst = float((np.abs(out["m_b"][i] - ref) / (1e-6 * np.abs(ref) + T.TINY)).max())
        print("%-58s %-18s %.3e  (error over 1e-6 |m'|; not asserted)" % (tag, "m'/|m'| " + k, worst), flush=True)


for c in R.DQN_CASES:
    r64, out = R.dqn_yardstick(c)[1], T.dqn_result(c)
    print("dqn %-54s float64 norm %.4f coef %.6f" % (R.case_id(c), r64["norm"], r64["coef"]))
    show("dqn a " + R.case_id(c), T.dqn_figures_a(c, out))
    show("dqn b " + R.case_id(c), T.dqn_figures_b(c, out))
    m_stated("dqn b " + R.case_id(c), R.DQN_TENSORS, out, T.dqn_state(c, out), R.dqn_yardstick(c)[0]["q"], R.DQN_LR)
for c in R.PPO_CASES:
    out = T.ppo_result(c)
    show("ppo a " + R.case_id(c), T.ppo_figures_a(c, out))
    show("ppo b " + R.case_id(c), T.ppo_figures_b(c, out))
with tempfile.TemporaryDirectory() as tmp:
    for c, child in zip(R.CHILD_CASES, T.one_launch_results(os.path.join(tmp, "one_launch.npz"))):
        show("one-launch a " + R.case_id(c), T.dqn_figures_a(c, child))
        show("one-launch b " + R.case_id(c), T.dqn_figures_b(c, child))
        show("one-launch vs two " + R.case_id(c), T.one_launch_figures_vs_two_launches(c, child, T.dqn_result(c)))
        print("one-launch vs two %s bit-identical: %s" % (R.case_id(c), T.bit_identical(child, T.dqn_result(c))))
print("worst err_k / err_t: %.2f at %s" % tuple(worst))
