"""The conditions tests/test_gpu_transition_body.py stands on, checked without a GPU and from tests/transition_reference.py's emulation
alone (the oracle steps, the float64 forward on [previous board, board] chooses): with the integer weights of each channel count

  (a) every greedy decision of the emulated rollouts has a top-two gap >= 1 (the scores are integers: no ties, so "the first maximum"
      never decides and the kernel's action must be the emulation's) and every partial sum stays below 2^24 (float32 is exact);
  (b) the policy takes at least two actions;
  (c) in at least a quarter of the (env, step) pairs the decision differs from the same weights fed [current, current] -- otherwise a
      kernel that ignores channel 0 would pass;
  (d) the 103-step run contains, for every env, a step behind an auto-reset whose observation [board, board] differs from
      [last board of the old episode, board] -- otherwise a kernel that forgets the reset would pass;

and of the header

  (e) the three entry points exist and none has a non-const pointer parameter (tests/test_guard_arena_cpu.py lists those of the
      whole header in an existing table);
  (f) every pointer field of sgk_convq_transition names a guard-band test of tests/test_gpu_transition_body.py."""
import importlib
import re

import numpy as np
import pytest

import test_guard_arena_cpu as HDR
import transition_reference as TR

ENTRY_POINTS = ("sgk_convq_act_trans", "sgk_convq_sample_trans", "sgk_convq_rollout_trans")


@pytest.mark.parametrize("channels", TR.CHANNELS)
def test_the_emulated_rollouts_meet_the_conditions_the_gpu_tests_stand_on(channels):
    long = TR.emulated(channels, TR.N, 103, True, False)
    gap, taken, differs, shown = TR.rollout_conditions(long)
    print("C = %d: smallest gap %g, %d actions taken, %.3f of the decisions differ from [current, current], %d of %d envs show the reset"
          % (channels, gap, taken, differs, shown, TR.N))
    assert gap >= 1.0                      # (a)
    assert taken >= 2                      # (b)
    assert differs >= 0.25                 # (c)
    assert shown == TR.N                   # (d)
    # (d), spelled out: behind a reset the emulation's channel 0 IS the board, and the old episode's last board is another one
    b = long["behind_reset"]
    assert b.any(0).all() and (long["prev_states"][b] == long["states"][b]).all()
    assert (long["stale_prev"][b] != long["states"][b]).any(1).all()
    assert b[91].all() and (long["recs"][90, :, 2] != 0).all()  # PRE_STEPS = 9: the 100-step episodes end at step 90 of the rollout
    for res in (TR.emulated(channels, TR.N, 12, False, False), TR.emulated(channels, TR.N, 103, False, True)):
        assert res["gap"].min() >= 1.0     # (a) for the other cases
    w = TR.rollout_weights(channels)
    for res in (long,):
        T = len(res["states"])
        top = max(TR.abs_sum_bound(res["prev_states"][k], res["states"][k], w) for k in range(0, T, 7))
        assert top < TR.EXACT_LIMIT, top


def test_the_masked_run_idles_and_zeroes_behind_the_episode_end():
    res = TR.emulated(5, TR.N, 103, False, True)
    assert (res["recs"][90, :, 2] != 0).all()
    for k in ("states", "prev_states"):
        assert (res[k][91:] == 0).all() and (res[k][:91] != 0).any(2).all()
    assert (res["actions"][91:] == 0).all() and (res["fields"]["game_over"] == 1).all()
    # an idle env still moves on: what the launch leaves as previous boards is the (unchanged) current board
    assert (res["prev_boards"] == res["boards"]).all()


def test_two_launches_are_one():
    """7 + 5 steps, `fresh` on the first launch only and its prev_boards carried into the second, equal the 12."""
    w = TR.rollout_weights(5)
    whole = TR.emulated(5, TR.N, 12, False, False)
    a = TR.emulate_rollout(w, TR.N, 7, False)
    b = TR.emulate_rollout(w, TR.N, 5, False, prev=a["prev_boards"], batch=a["batch"], metrics=a["metrics"], t_begin=TR.PRE_STEPS + 7)
    for k in ("states", "prev_states", "actions", "recs"):
        assert (np.concatenate((a[k], b[k])) == whole[k]).all(), k
    assert (b["prev_boards"] == whole["prev_boards"]).all() and (b["boards"] == whole["boards"]).all()
    assert (whole["prev_boards"] == whole["states"][-1]).all()  # nothing was reset: the board the last action was chosen on


def test_the_acting_inputs_are_half_fresh_half_stepped_and_exact():
    prev, cur = TR.act_inputs(TR.N)
    assert (prev[1::2] == cur[1::2]).all() and (prev[0::2] != cur[0::2]).any(1).mean() > 0.5
    for c in TR.CHANNELS:
        w = TR.weights("integer", c, 7100 + c)
        assert TR.abs_sum_bound(prev, cur, w) < TR.EXACT_LIMIT
        s = TR.forward(prev, cur, w)
        assert (s == np.round(s)).all()
        assert (TR.forward(cur, cur, w) != s).any()  # channel 0 matters to the scores


def test_pass_sizes():
    assert TR.ENVS_PER_PASS == 17 and TR.N == 17 + 17 + 6
    n = TR.second_pass_n(256)
    assert n == (256 * 4) * 17 + 23 and -(-n // 17) > 256 * 4


# ---- the header ----------------------------------------------------------------------------------------------------------------------
def _params(fn):
    m = re.search(r"SGK_API\s+[\w\s\*]+?\b%s\s*\(([^)]*)\)\s*;" % fn, HDR._header())
    assert m, fn
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_the_entry_points_have_no_writable_pointer_parameter(fn):
    params = _params(fn)
    assert params[0] == "sgk_env *h" and "const sgk_convq_weights *w" in params and "const sgk_convq_transition *tr" in params
    for p in params:
        assert HDR._writable(p) == [], (fn, p)
    assert not [k for k in HDR.header_writable_pointers() if k.startswith(fn + ".")]


def _struct_pointer_fields():
    body = re.search(r"typedef struct sgk_convq_transition \{(.*?)\} sgk_convq_transition;", HDR._header(), flags=re.S).group(1)
    return [n for decl in body.split(";") for n in HDR._writable(decl, field=True)]


def test_every_pointer_field_of_the_descriptor_names_a_guard_band_test():
    fields = _struct_pointer_fields()
    assert fields[:2] == ["prev_boards_dev", "prev_states_out_dev"] and len(fields) == 6
    gpu = importlib.import_module("test_gpu_transition_body")
    assert sorted(gpu.GUARD_BAND_TESTS) == sorted(fields)
    for field, names in gpu.GUARD_BAND_TESTS.items():
        assert names, field
        for name in names:
            assert name.startswith("test_") and callable(getattr(gpu, name, None)), (field, name)


def test_the_binding_mirrors_the_descriptor():
    from safe_grid_agents_amd import _lib

    body = re.search(r"typedef struct sgk_convq_transition \{(.*?)\} sgk_convq_transition;", HDR._header(), flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert [f[0] for f in _lib.SgkConvQTransition._fields_] == names
    for fn in ENTRY_POINTS:
        assert fn in _lib.EXPORTED_SYMBOLS


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_the_transition_policy_flag_is_absent_unless_given_and_refused_off_trans_boat():
    from safe_grid_agents_amd import trainer

    parser = trainer.prepare_parser()
    need = ["-l", "0.001", "-r", "4", "-e", "2"]  # (the reference's required flags)
    for agent in ("ppo-cnn", "ppo-crmdp"):
        plain = parser.parse_args(["-N", "64", "trans-boat", agent] + need)
        assert not hasattr(plain, "transition_policy") and trainer.check_transition_policy(plain) is False
        given = parser.parse_args(["-N", "64", "trans-boat", agent, "--transition-policy"] + need)
        assert given.transition_policy is True and trainer.check_transition_policy(given) is True
        with pytest.raises(SystemExit, match="trans-boat only"):
            trainer.check_transition_policy(parser.parse_args(["-N", "64", "boat", agent, "--transition-policy"] + need))
    with pytest.raises(SystemExit, match="no population form"):
        trainer.check_transition_policy(parser.parse_args(["trans-boat", "ppo-cnn", "--transition-policy", "--members", "2"] + need))
    with pytest.raises(SystemExit):  # (argparse: the flag belongs to the two conv agents)
        parser.parse_args(["-N", "64", "trans-boat", "ppo-mlp", "--transition-policy"] + need)
