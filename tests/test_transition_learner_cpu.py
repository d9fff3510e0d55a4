"""What tests/test_gpu_transition_learn.py stands on, checked without a GPU: the float64 reference of the two-board conv learner
(tests/transition_learner_reference.py) against the one-board reference, the seeded cases' row conditions and their float32 yardstick,
the header's and the binding's two new entry points, the workspace formula and the command line flag."""
import re

import numpy as np
import pytest

import learner_reference as R
import test_guard_arena_cpu as HDR
import transition_learner_reference as TL

# what reordering a float64 sum of batch x cells = 1 600 terms can change, relative to max|g|: below 1 600 x 2^-53 = 1.8e-13 of the terms'
# magnitude; nine orders of magnitude below anything the GPU tests resolve
WB_REORDER = 1e-13
ENTRY_POINTS = ("sgk_ppo_cnn_epochs_trans", "sgk_ppo_cnn_trans_workspace_bytes")


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in TL.CASES if c.batch == 64 and c.variant == "clip"], ids=TL.case_id)
def test_with_channel_0_weights_zero_the_reference_is_the_one_board_reference_on_channel_1(case):
    """w1[:, 0] = wb[:, 0] = 0 in both networks: the previous board no longer counts, and the scalars, ratios, values and every gradient
    but channel 0's own are ppo_cnn_epoch64's on the current board with w1[:, 1:2] and wb[:, 1:2] -- exactly, in float64 (the zero
    products add nothing). Channel 0's gradients are not zero: the loss still depends on those weights.

    One tensor is held to WB_REORDER instead of bit equality: the 1 x 1 convolution's weight gradient is a sum over batch x cells that
    torch's backward evaluates in another order for a [C, 2] weight than for a [C, 1] one (measured: 1.2e-16 to 6.2e-16 of max|g|, all
    terms equal). Every other quantity, the 3 x 3 conv1's gradient included, is equal bit for bit."""
    d = TL.trans_inputs(case)
    obs, actions, returns = TL.gather(d, d["rows"])
    assert obs.shape == (case.batch, 2, 5, 5)

    def cut(params, zero):
        out = [p.copy() for p in params]
        for i in (0, 4):
            if zero:
                out[i][:, 0] = 0.0
            else:
                out[i] = out[i][:, 1:2].copy()
        return out

    kw = TL.loss_kw(case)
    two = TL.trans_epoch64(cut(d["cur"], True), cut(d["old"], True)[:10], obs, actions, returns, **kw)
    one = R.ppo_cnn_epoch64(cut(d["cur"], False), cut(d["old"], False)[:10], obs[:, 1], actions, returns, **kw)
    assert two["stats"] == one["stats"]
    for k in ("ratio", "values", "advantage"):
        assert (two[k] == one[k]).all(), k
    for i, k in enumerate(TL.TENSORS):
        g2 = two["grads"][i][:, 1:2] if i in (0, 4) else two["grads"][i]
        assert g2.shape == one["grads"][i].shape, k
        if k == "wb":
            assert R.rel_err(g2, one["grads"][i]) <= WB_REORDER, k
        else:
            assert (g2 == one["grads"][i]).all(), k
    for i in (0, 4):
        assert np.abs(two["grads"][i][:, 0]).max() > 0.0


def test_the_planes_are_not_interchangeable():
    """Swapping the two planes of the observation changes w1's and wb's float64 gradients by far more than any bound of the GPU test."""
    case = TL.CASES[1]
    d, r64, _ = TL.yardstick(case)
    obs, actions, returns = TL.gather(d, d["rows"])
    swapped = TL.trans_epoch64(d["cur"], d["old"][:10], obs[:, ::-1].copy(), actions, returns, **TL.loss_kw(case))
    for i in (0, 4):
        assert R.rel_err(swapped["grads"][i], r64["grads"][i]) > 1e3 * R.CAP


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_ones_the_gpu_file_runs():
    keys = [(c.channels, c.batch, c.variant) for c in TL.CASES]
    assert keys[:5] == [(4, 64, "clip"), (5, 64, "clip"), (8, 64, "clip"), (5, 2, "clip"), (5, 37, "clip")]
    assert sorted(c.variant for c in TL.CASES[5:]) == ["defaults", "tie"] and len(TL.CASES) == 7
    assert len({c.seed for c in TL.CASES}) == len(TL.CASES)
    assert [c.channels for c in TL.PLUMBING_CASES] == [5, 8]
    assert (TL.T, TL.N) == (3, 37)
    for key, seed in TL.RESEED.items():
        assert any((c.channels, c.batch, c.variant) == key and c.seed == seed for c in TL.CASES), key


@pytest.mark.parametrize("case", TL.CASES, ids=TL.case_id)
def test_row_conditions_and_a_satisfiable_bound(case):
    """The minibatch holds what its docstring says, in float64; both planes hold 0..5 and differ; and torch-float32's own error on these
    inputs is below CAP / 8 for every gradient tensor and every statistic, so that max(8 err_t, 16 x 2^-23) <= 1e-5 can be met."""
    d, r64, err_t = TL.yardstick(case)
    bad = [k for k, ok in TL.row_conditions(case, d).items() if not ok]
    assert not bad, bad
    for k in ("states", "prev_states"):
        assert d[k].shape == (TL.T, TL.N, 25) and d[k].min() == 0 and d[k].max() == 5, k
    assert [tuple(p.shape) for p in d["cur"]] == TL.param_shapes(case.channels)
    assert sorted(err_t) == sorted(TL.TENSORS + TL.STATS)
    for k, e in err_t.items():
        assert e < R.CAP / 8, (k, e)
        assert R.bound(e) <= R.CAP
    for g in r64["grads"]:
        assert np.isfinite(g).all() and np.abs(g).max() > 0


# ---- the header and the binding ---------------------------------------------------------------------------------------------------------
def _params(fn):
    m = re.search(r"SGK_API\s+[\w\s\*]+?\b%s\s*\(([^)]*)\)\s*;" % fn, HDR._header())
    assert m, "include/sgk.h does not declare " + fn
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_the_header_declares_the_entry_points_without_a_writable_pointer(fn):
    params = _params(fn)
    assert params[0] == "sgk_env *h"
    for p in params:
        assert HDR._writable(p) == [], (fn, p)
    assert not [k for k in HDR.header_writable_pointers() if k.startswith(fn + ".")]
    if fn == "sgk_ppo_cnn_epochs_trans":
        assert params[1:] == ["const sgk_ppo_cnn_learner *learner", "const int8_t *prev_states"]
    else:
        assert params[1:] == ["int32_t n_channels", "int32_t batch"]


def test_the_binding_has_both_entry_points():
    import ctypes

    from safe_grid_agents_amd import _lib

    for fn in ENTRY_POINTS:
        assert fn in _lib.EXPORTED_SYMBOLS, fn
    res, args = _lib._SIGNATURES["sgk_ppo_cnn_epochs_trans"]
    assert res is ctypes.c_int and len(args) == 3 and args[1] is ctypes.POINTER(_lib.SgkPpoCnnLearner) and args[2] is ctypes.c_void_p
    res, args = _lib._SIGNATURES["sgk_ppo_cnn_trans_workspace_bytes"]
    assert res is ctypes.c_int64 and list(args[1:]) == [ctypes.c_int32, ctypes.c_int32]


# ---- the workspace ----------------------------------------------------------------------------------------------------------------------
def test_the_workspace_formula():
    """The header states 4 (1088 + batch (5 C 25 + P2)) with P2 = P + 10 C and quotes 530 432 bytes at C = 5, batch 64; the helper the GPU
    file holds the library's answer against computes that formula. (The library answers only on a handle, which needs a device:
    tests/test_gpu_transition_learn.py asks it for C = 4, 5, 8 and batch 2 and 64.)"""
    text = " ".join(open(HDR.os.path.join(HDR.ROOT, "include", "sgk.h")).read().split())
    assert "4 * (1088 + batch * (5 * C * 25 + P2))" in text and "P2 = P + 10 * C" in text and "530 432" in text
    assert TL.workspace_bytes(5, 64) == 530432
    for C in (4, 5, 8):
        cells = 25
        p1 = 9 * C + C + 3 * (9 * C * C + C) + C + C + 5 * C * cells + 5  # the 14 one-board tensors, added up
        assert p1 == sum(int(np.prod(s)) for s in TL.param_shapes(C)) - 10 * C
        for batch in (2, 64):
            assert TL.workspace_bytes(C, batch) == 4 * (1088 + batch * (5 * C * cells + p1 + 10 * C))


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_the_fused_transition_learn_flag_is_absent_unless_given_and_needs_the_transition_policy():
    from safe_grid_agents_amd import trainer  # (the parser and the two checks: no torch, no device)

    parser = trainer.prepare_parser()
    need = ["-l", "0.001", "-r", "4", "-e", "2"]  # (the reference's required flags)
    for agent in ("ppo-cnn", "ppo-crmdp"):
        plain = parser.parse_args(["-N", "64", "trans-boat", agent, "--transition-policy"] + need)
        assert not hasattr(plain, "fused_transition_learn") and trainer.check_fused_transition_learn(plain) is False
        given = parser.parse_args(["-N", "64", "trans-boat", agent, "--transition-policy", "--fused-transition-learn"] + need)
        assert given.fused_transition_learn is True and given.transition_policy is True
        assert trainer.check_transition_policy(given) is True and trainer.check_fused_transition_learn(given) is True
        alone = parser.parse_args(["-N", "64", "trans-boat", agent, "--fused-transition-learn"] + need)
        with pytest.raises(SystemExit, match="--transition-policy") as ei:
            trainer.check_fused_transition_learn(alone)
        assert isinstance(ei.value.code, str)  # (a plain message, not argparse's exit status)
    with pytest.raises(SystemExit):  # (argparse: the flag belongs to the two conv agents)
        parser.parse_args(["-N", "64", "trans-boat", "ppo-mlp", "--fused-transition-learn"] + need)
