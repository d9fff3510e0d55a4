"""Prints what tests/test_gpu_learner_gradients.py measures, per case and quantity: the float64 reference's gradient norm and clip
coefficient, err_k (kernel against float64), err_t (torch-float32 against float64) and the limit for step A; the worst element's error
over its allowance for step B; the one-launch child against float64 and against the two-launch form. -> profiles/learner_gradients/errors.log
With --cnn the same lines for the conv learner alone (tests/test_gpu_ppo_cnn_gradients.py: steps A and B of every case, the ragged
rollout's statistics, whether the two-epoch call was bit-identical), then the median err_k / err_t over the gradient tensors and the
figure closest to its limit -> profiles/ppo_cnn_gradients/errors.log. With --chain what tests/test_gpu_ppo_epoch_chain.py measures alone:
the torch-float32 chain's err_t and the stale-epoch emulation's distance per tensor (the CPU side), then per chain case err_k, the limit
and err_k / err_t of the eight tensors and of every epoch's statistics, and for every run of its parts (a) and (b) whether the epochs in one
call left the bytes of the calls of one epoch -> profiles/ppo_epoch_chain/errors.log. Without either flag the MLP learners alone, line for
line as before."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "safe-grid-agents_amd")]
import learner_reference as R  # noqa: E402
import test_gpu_learner_gradients as T  # noqa: E402

CNN = "--cnn" in sys.argv
CHAIN = "--chain" in sys.argv
MLP = not CNN and not CHAIN

worst = [0.0, ""]  # the largest err_k / err_t and where
closest = [0.0, ""]  # the largest measured / limit and where
ratios = []  # err_k / err_t of every gradient tensor
worst_grad = [0.0, ""]  # the largest of them and where


def show(tag, figs):
    for what, got, limit, err_t in figs:
        if err_t is not None and got / max(err_t, 1e-300) > worst[0]:
            worst[:] = [got / max(err_t, 1e-300), "%s %s (err_k %.3e, err_t %.3e)" % (tag, what, got, err_t)]
        if err_t is not None and what.startswith("grad "):
            ratios.append(got / max(err_t, 1e-300))
            if ratios[-1] > worst_grad[0]:
                worst_grad[:] = [ratios[-1], "%s %s (err_k %.3e, err_t %.3e, limit %.3e)" % (tag, what, got, err_t, limit)]
        if got / limit > closest[0]:
            closest[:] = [got / limit, "%s %s (%.3e against a limit of %.3e)" % (tag, what, got, limit)]
        print("%-58s %-18s %.3e  limit %.3e%s%s" % (tag, what, got, limit, "" if err_t is None else "  err_t %.3e  err_k/err_t %.2f" % (err_t, got / max(err_t, 1e-300)),
                                                    "" if got <= limit else "  ABOVE"), flush=True)


# the CPU side first (all that `--cpu` prints): the float64 norms and torch-float32's own error err_t per case and quantity
for c in R.DQN_CASES if MLP else ():
    _, r64, err_t = R.dqn_yardstick(c)
    print("yardstick dqn %-54s float64 norm %.4f coef %.6f  err_t " % (R.case_id(c), r64["norm"], r64["coef"]) + " ".join("%s %.2e" % kv for kv in err_t.items()))
for c in R.PPO_CASES if MLP else ():
    print("yardstick ppo %-54s err_t " % R.case_id(c) + " ".join("%s %.2e" % kv for kv in R.ppo_yardstick(c)[2].items()))
for c in R.PPO_CNN_CASES if CNN else ():
    print("yardstick ppo-cnn %-50s err_t " % R.cnn_case_id(c) + " ".join("%s %.2e" % kv for kv in R.ppo_cnn_yardstick(c)[2].items()))
for c in R.CHAIN_CASES if CHAIN else ():
    d, rows, state, c64, err_t = R.chain_yardstick(c)
    stale = R.ppo_chain64(d, rows, state, R.CHAIN_STEP0, stale=True)
    for i, k in enumerate(R.PPO_TENSORS):
        want, w0 = c64["params"][-1][i], d["cur"][i]
        limit, far = R.chain_limit(err_t[k], want, w0, R.CHAIN_EPOCHS), R.chain_err(stale["params"][-1][i], want, w0)
        print("yardstick chain %-36s %-3s moved %.3e  err_t %.3e  limit %.3e  stale epochs %.3e = %.0f limits" % (
            R.case_id(c), k, float(np.abs(want - w0).max()), err_t[k], limit, far, far / limit))
    print("yardstick chain %-36s err_t " % R.case_id(c) + " ".join("%s %.2e" % kv for kv in err_t.items() if " " in kv[0]))
if "--cpu" in sys.argv:
    sys.exit(0)


def m_stated(tag, names, out, state, w0s, lr):
    """m' against 1e-6 |m'| (the bound as first stated, which cancellation in m + (1 - beta1)(g - m) makes unreachable): for the record"""
    for i, k in enumerate(names):
        ref = R.adam64(w0s[i], state[0][i], state[1][i], None, T._clipped_gradient(out)[i], T.LC.STEP_BEFORE_B + 1, lr)[1]
        worst = float((np.abs(out["m_b"][i] - ref) / (1e-6 * np.abs(ref) + T.TINY)).max())
        print("%-58s %-18s %.3e  (error over 1e-6 |m'|; not asserted)" % (tag, "m'/|m'| " + k, worst), flush=True)


def mlp_learners():
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


def cnn_learner():
    import test_gpu_ppo_cnn_gradients as TC

    for c in R.PPO_CNN_CASES:
        out = TC.cnn_result(c)
        show("ppo-cnn a " + R.cnn_case_id(c), TC.cnn_figures_a(c, out))
        show("ppo-cnn b " + R.cnn_case_id(c), TC.cnn_figures_b(c, out))
        state = R.inject_adam_state(T._clipped_gradient(out), T.LC.STATE_SEED + c.seed, False)
        m_stated("ppo-cnn b " + R.cnn_case_id(c), R.CNN_TENSORS, out, state, R.ppo_cnn_yardstick(c)[0]["cur"], R.ppo_cnn_hyper(c)["lr"])
    for c in R.PLUMBING_CASES:
        res = TC.plumbing_result(c)
        same = all(a.tobytes() == b.tobytes() for key in ("w", "m", "v", "step") for a, b in zip(res["two"][key], res["one"][key]))
        print("ppo-cnn two epochs in one call vs two calls %s bit-identical: %s" % (R.cnn_case_id(c), same and res["two"]["stats"].tobytes() == res["one"]["stats"].tobytes()))
        print("ppo-cnn ragged %s rows %s" % (R.cnn_case_id(c), " ".join(str(r) for r in res["ragged"][0]["rows"])))
        show("ppo-cnn ragged " + R.cnn_case_id(c), TC.ragged_figures(c, res["ragged"][0]))


def epoch_chain():
    import test_gpu_ppo_epoch_chain as TE

    same = []
    for run in TE.RUNS + TE.CHAIN_RUNS:
        out = TE.single_result(run)[0]
        bad, again = TE._bytes_differ(out["one"], out["chain"]), TE._bytes_differ(out["one"], out["again"])
        same.append(not bad and not again)
        print("epochs in one call vs calls of one epoch %-56s bit-identical: %s%s; the one call twice: %s" % (
            TE.run_id(run), not bad, "" if not bad else " (differs in " + " ".join(bad) + ")", not again), flush=True)
    for run in TE.MEMBER_RUNS:
        out = TE.members_result(run)[0]
        bad, again = TE._bytes_differ(out["one"], out["chain"]), TE._bytes_differ(out["one"], out["again"])
        same.append(not bad and not again)
        print("members: epochs in one launch vs launches of one epoch %-42s bit-identical: %s%s; the one launch twice: %s" % (
            TE.run_id(run), not bad, "" if not bad else " (differs in " + " ".join(bad) + ")", not again), flush=True)
    print("bit-identical: %d of %d runs" % (sum(same), len(same)))
    for c, run in zip(R.CHAIN_CASES, TE.CHAIN_RUNS):
        show("chain " + R.case_id(c), TE.chain_figures(c, TE.single_result(run)[0]["one"]))


if MLP:
    mlp_learners()
if CHAIN:
    epoch_chain()
    print("closest to its limit: %.3f of it at %s" % tuple(closest))
if CNN:
    cnn_learner()
if CNN:
    print("note: the policy_loss lines of the -tie case are absolute errors over mean |normalised advantage| (the reference value is "
          "0 there: learner_reference.cnn_stat_pair); every other statistic is relative to the reference value")
    print("gradient tensors: %d; median err_k / err_t: %.2f; worst %.2f at %s"
          % (len(ratios), float(np.median(ratios)), worst_grad[0], worst_grad[1]))
    print("closest to its limit: %.3f of it at %s" % tuple(closest))
print("worst err_k / err_t: %.2f at %s" % tuple(worst))
