"""Prints what tests/test_gpu_forward_float64.py measures: per "real" case and per-step kernel (act = sgk_policy_act / sgk_convq_act,
sample = sgk_policy_sample / sgk_convq_sample) err_k (kernel against float64, relative to the largest score), err_t (torch-float32
against float64 on the CPU), their ratio and the limit learner_reference.bound(err_t); then the median and the worst ratio, the case
closest to its limit, and how many "integer" cases (small, painted, multi-pass) equal the float64 scores. -> profiles/forward_float64/errors.log
With --cpu the CPU side alone (err_t, the limit, max|s64|, the share of near-ties per real case; the abs-sum bound and the exact ties per
integer case); with --seeds forward_reference.SEED_DRAWS and ROLLOUT_SEED_DRAWS computed anew."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "safe-grid-agents_amd")]
import forward_reference as FR  # noqa: E402

if "--seeds" in sys.argv:
    print("SEED_DRAWS", FR.seed_draws())
    print("ROLLOUT_SEED_DRAWS", FR.rollout_seed_draws())
    sys.exit(0)

for c in FR.CASES:
    y = FR.yardstick(c)
    if c.family == "real":
        print("yardstick %-52s err_t %.3e  limit %.3e  max|s64| %8.3f  near-ties %.4f" % (FR.case_id(c), y["err_t"], y["bound"], y["top"], 1.0 - y["clear"].mean()))
    else:
        print("yardstick %-52s envs %5d (at %d CUs)  abs-sum bound %8.0f of %d  exact ties %d" % (
            FR.case_id(c), len(y["boards"]), FR.DEFAULT_CUS, FR.abs_sum_bound(c.body, y["boards"], y["weights"], y["shape"]), FR.EXACT_LIMIT, int((y["gap"] == 0).sum())))
if "--cpu" in sys.argv:
    sys.exit(0)

import test_gpu_forward_float64 as T  # noqa: E402

ratios, worst, closest = [], [0.0, ""], [0.0, ""]
for c in FR.REAL_CASES:
    for kernel, err_k, err_t, limit in T.figures(c):
        ratio = err_k / max(err_t, 1e-300)
        ratios.append(ratio)
        where = "%s %s (err_k %.3e, err_t %.3e, limit %.3e)" % (FR.case_id(c), kernel, err_k, err_t, limit)
        if ratio > worst[0]:
            worst[:] = [ratio, where]
        if err_k / limit > closest[0]:
            closest[:] = [err_k / limit, where]
        print("%-52s %-6s err_k %.3e  err_t %.3e  err_k/err_t %5.2f  limit %.3e%s" % (FR.case_id(c), kernel, err_k, err_t, ratio, limit,
                                                                                     "" if err_k <= limit else "  ABOVE"), flush=True)
exact = {}
for c in FR.CASES:
    if c.family == "integer":
        y, out = FR.yardstick(c, T.case_cus(c)), T.kernel_result(c)
        same = all(np.array_equal(out[k], y["s64"]) for k in ("act", "sample")) and np.array_equal(out["greedy"], y["argmax"])
        if not same:
            print("%-52s NOT EQUAL to float64" % FR.case_id(c))
        exact.setdefault(c.size, []).append(same)
for size, same in exact.items():
    print("integer cases (%s): %d of %d equal the float64 scores and argmax on every env" % (size, sum(same), len(same)))
print("real cases: %d figures; median err_k / err_t: %.2f; worst %.2f at %s" % (len(ratios), float(np.median(ratios)), worst[0], worst[1]))
print("closest to its limit: %.3f of it at %s" % tuple(closest))
