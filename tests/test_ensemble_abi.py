"""Ensemble acting (include/sgk.h: sgk_policy_act_members_all, sgk_members_vote, sgk_members_vote_host; safe_grid_agents_amd/ensemble.py)
as far as a box without a GPU can tell: the symbols are declared, exported and bound with the header's signatures and the ABI version
stays; every bad argument is refused before the handle is looked at, with a message, and nothing is written; the host vote equals the
numpy reference (tests/ensemble_reference.py) on random actions, constructed ties, a voter subset, a live mask and accumulating
counters; the --ensemble-eval grammar; and the reference itself against hand-written cases."""
import ctypes
import os
import re

import numpy as np
import pytest

import ensemble_reference as ER
import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib, ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
N_ENVS = 200


def _header():
    return open(os.path.join(ROOT, "include", "sgk.h")).read()


def _declared(name):
    m = re.search(r"SGK_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "include/sgk.h does not declare int %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _vote_host(member_actions, members=None, live=None, dissent=None, with_votes=True):
    """sgk_members_vote_host -> (actions, votes, dissent); `dissent`: the int64 [2] the call adds to (default: zeros)."""
    a = np.ascontiguousarray(member_actions, dtype=np.uint8)
    M, n = a.shape
    ids = None if members is None else np.ascontiguousarray(members, dtype=np.int32)
    mask = None if live is None else np.ascontiguousarray(live, dtype=np.uint8)
    actions, votes = np.full(n, 9, dtype=np.uint8), np.full((n, 4), 77, dtype=np.uint16)
    dissent = np.zeros(2, dtype=np.int64) if dissent is None else dissent
    rc = _lib.load().sgk_members_vote_host(a.ctypes.data, M, n, None if ids is None else ids.ctypes.data, 0 if ids is None else len(ids),
                                           None if mask is None else mask.ctypes.data, actions.ctypes.data,
                                           votes.ctypes.data if with_votes else None, dissent.ctypes.data)
    assert rc == _lib.SGK_OK, _lib.load().sgk_last_error()
    return actions, votes, dissent


def _same(got, want):
    for g, w, what in zip(got, want, ("actions", "votes", "dissent")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, g, w)


# ---- the reference itself, against cases worked out by hand -------------------------------------------------------------------------------
def test_the_reference_on_hand_written_cases():
    a = np.array([[0, 1, 3, 2],
                  [0, 2, 3, 1],
                  [1, 2, 0, 0]], dtype=np.uint8)  # three members, four envs
    actions, votes, dissent = ER.vote(a)
    assert actions.tolist() == [0, 2, 3, 0]  # 2-1, 2-1, 2-1, and 1-1-1 over the actions 0, 1, 2: the lowest
    assert votes.tolist() == [[2, 1, 0, 0], [0, 1, 2, 0], [1, 0, 0, 2], [1, 1, 1, 0]]
    assert dissent.tolist() == [1 + 1 + 1 + 2, 12]
    assert ER.vote(a, live=[1, 0, 0, 1])[2].tolist() == [1 + 2, 6]
    actions, votes, dissent = ER.vote(a, members=[2, 0])
    assert actions.tolist() == [0, 1, 0, 0] and dissent.tolist() == [1 + 1 + 1 + 1, 8]  # every env a 1-1 tie: the lower action
    assert votes.dtype == np.uint16 and actions.dtype == np.uint8 and dissent.dtype == np.int64


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    assert _declared("sgk_policy_act_members_all") == ["sgk_env *h", "const sgk_mlp_weights *w", "int32_t n_members",
                                                       "uint8_t *member_actions_out_dev", "float *member_scores_out_dev"]
    assert _declared("sgk_members_vote") == ["sgk_env *h", "const uint8_t *member_actions_dev", "int32_t n_members",
                                             "const int32_t *member_ids_dev", "int32_t n_voters", "uint8_t *actions_out_dev",
                                             "uint16_t *votes_out_dev", "int64_t *dissent_dev"]
    assert _declared("sgk_members_vote_host") == ["const uint8_t *member_actions", "int32_t n_members", "int64_t n_envs",
                                                  "const int32_t *member_ids", "int32_t n_voters", "const uint8_t *live",
                                                  "uint8_t *actions_out", "uint16_t *votes_out", "int64_t *dissent"]
    want = {"sgk_policy_act_members_all": (ctypes.c_int, [V, ctypes.POINTER(_lib.SgkMlpWeights), I32, V, V]),
            "sgk_members_vote": (ctypes.c_int, [V, V, I32, V, I32, V, V, V]),
            "sgk_members_vote_host": (ctypes.c_int, [V, I32, I64, V, I32, V, V, V, V])}
    lib = _lib.load()  # (resolves every bound symbol in libsgk.so: a missing export is an AttributeError here)
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name] == (res, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert lib.sgk_abi_version() == 4  # added symbols: the ABI version stays
    header = " ".join(_header().split())
    assert "policy_base.py:47-52" in header and "value.py:89-92" in header  # the greedy act's reference lines


def test_every_bad_argument_is_refused_before_the_handle_and_nothing_is_written():
    """The handle is NULL in every call: a refusal that names the bad argument was made before the handle was looked at, so the same
    check guards a real handle. Valid arguments with a NULL handle are refused for the handle. The buffers are host memory that a
    launch would never be given; they keep their bytes."""
    lib = _lib.load()
    M, n = 3, 8
    ma = np.zeros((M, n), dtype=np.uint8)
    ids = np.arange(M, dtype=np.int32)
    actions, votes, dissent = np.full(n, 9, dtype=np.uint8), np.full((n, 4), 77, dtype=np.uint16), np.array([5, 6], dtype=np.int64)
    scores = np.full((M, n, 4), 2.5, dtype=np.float32)
    blob = np.zeros(64, dtype=np.float32)
    w = _lib.SgkMlpWeights(*([blob.ctypes.data] * 6), 100)
    mp, ip, ap, vp, dp = (x.ctypes.data for x in (ma, ids, actions, votes, dissent))
    act_cases = [
        ((None, M, ap, None), b"NULL weights"), ((ctypes.byref(_lib.SgkMlpWeights(*([blob.ctypes.data] * 5), None, 100)), M, ap, None), b"NULL weights"),
        ((ctypes.byref(w), M, None, None), b"member_actions_out_dev is NULL"),
        ((ctypes.byref(_lib.SgkMlpWeights(*([blob.ctypes.data] * 6), 96)), M, ap, None), b"n_hidden"),
        ((ctypes.byref(w), 0, ap, None), b"n_members"), ((ctypes.byref(w), -1, ap, None), b"n_members"), ((ctypes.byref(w), 4097, ap, None), b"n_members"),
        ((ctypes.byref(w), M, ap, scores.ctypes.data + 4), b"16-byte aligned"),
    ]
    for args, message in act_cases:
        assert lib.sgk_policy_act_members_all(None, *args) == _lib.ERR_INVALID, message
        assert message in lib.sgk_last_error(), (message, lib.sgk_last_error())
    assert lib.sgk_policy_act_members_all(None, ctypes.byref(w), M, ap, scores.ctypes.data) == _lib.ERR_INVALID
    assert b"handle is NULL" in lib.sgk_last_error()
    vote_cases = [
        ((None, M, None, 0, ap, vp, dp), b"member_actions is NULL"), ((mp, M, None, 0, None, vp, dp), b"actions_out is NULL"),
        ((mp, 0, None, 0, ap, vp, dp), b"n_members"), ((mp, -2, None, 0, ap, vp, dp), b"n_members"), ((mp, 4097, None, 0, ap, vp, dp), b"n_members"),
        ((mp, M, None, 2, ap, vp, dp), b"every member votes"), ((mp, M, ip, 0, ap, vp, dp), b"n_voters"), ((mp, M, ip, M + 1, ap, vp, dp), b"n_voters"),
        ((mp, M, ip, -1, ap, vp, dp), b"n_voters"), ((mp, M, None, 0, ap, vp + 2, dp), b"votes_out must be 8-byte aligned"),
    ]
    for args, message in vote_cases:
        assert lib.sgk_members_vote(None, *args) == _lib.ERR_INVALID, message
        assert message in lib.sgk_last_error(), (message, lib.sgk_last_error())
        host = args[:2] + (n,) + args[2:4] + (None,) + args[4:]
        assert lib.sgk_members_vote_host(*host) == _lib.ERR_INVALID and message in lib.sgk_last_error(), message
    assert lib.sgk_members_vote(None, mp, M, None, 0, ap, vp, dp + 4) == _lib.ERR_INVALID and b"dissent_dev must be 8-byte aligned" in lib.sgk_last_error()
    assert lib.sgk_members_vote_host(mp, M, -1, None, 0, None, ap, vp, dp) == _lib.ERR_INVALID and b"n_envs" in lib.sgk_last_error()
    for voters in ((None, 0), (None, M), (ip, 1), (ip, M)):  # valid arguments, the optional outputs absent or present: only the handle is missing
        for outs in ((vp, dp), (None, None)):
            assert lib.sgk_members_vote(None, mp, M, *voters, ap, *outs) == _lib.ERR_INVALID
            assert b"handle is NULL" in lib.sgk_last_error()
    assert (actions == 9).all() and (votes == 77).all() and dissent.tolist() == [5, 6] and (scores == 2.5).all()


# ---- the host vote ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 4, 7, 4096])
def test_the_host_vote_equals_the_reference_on_random_actions(M):
    rng = np.random.default_rng(1000 + M)
    a = rng.integers(0, 4, size=(M, N_ENVS), dtype=np.uint8)
    got = _vote_host(a)
    _same(got, ER.vote(a))
    assert got[1].sum(axis=1).tolist() == [M] * N_ENVS and got[2][1] == M * N_ENVS
    if M == 4096:  # one action for everybody in some env: a count of 4096 fits the 16 bits, its neighbours stay zero
        a[:, 17] = 2
        actions, votes, _ = _vote_host(a)
        assert votes[17].tolist() == [0, 0, 4096, 0] and actions[17] == 2
    actions_only = _vote_host(a, with_votes=False)  # votes_out is optional
    assert actions_only[0].tobytes() == ER.vote(a)[0].tobytes() and (actions_only[1] == 77).all()


def test_ties_go_to_the_lowest_action_and_absent_actions_get_no_votes():
    ties = {
        "2-2": ([3, 1, 1, 3], 1), "2-2 low": ([0, 2, 2, 0], 0), "1-1-1-1": ([3, 2, 1, 0], 0), "1-1": ([3, 2], 2),
        "2-2-1": ([1, 3, 0, 3, 1], 1), "3-3": ([2, 3, 3, 2, 2, 3], 2), "unanimous": ([3, 3, 3], 3), "one voter": ([2], 2),
    }
    for name, (column, winner) in ties.items():
        a = np.array(column, dtype=np.uint8).reshape(-1, 1)
        got = _vote_host(a)
        _same(got, ER.vote(a))
        assert got[0][0] == winner, name
        for k in range(4):
            assert got[1][0][k] == column.count(k), (name, k)  # 0-vote actions included
        assert got[2].tolist() == [len(column) - column.count(winner), len(column)], name


def test_a_voter_subset_the_live_mask_and_accumulating_counters():
    rng = np.random.default_rng(77)
    a = rng.integers(0, 4, size=(7, N_ENVS), dtype=np.uint8)
    for members in ([2, 0], [6], [5, 4, 3, 2, 1, 0], list(range(7))):
        _same(_vote_host(a, members=members), ER.vote(a, members=members))
    assert _vote_host(a, members=[2, 0])[0].tobytes() != _vote_host(a)[0].tobytes()  # the subset decides otherwise somewhere
    live = rng.integers(0, 2, size=N_ENVS).astype(np.uint8)
    live[:3] = (0, 1, 255)  # any non-zero byte is "live"
    got = _vote_host(a, live=live)
    _same(got, ER.vote(a, live=live))
    assert 0 < got[2][1] < 7 * N_ENVS  # some envs excluded, not all
    _same(_vote_host(a, members=[1, 3, 5], live=live), ER.vote(a, members=[1, 3, 5], live=live))
    assert _vote_host(a, live=np.zeros(N_ENVS, dtype=np.uint8))[2].tolist() == [0, 0]
    # two calls into the same counters: the sums of the two
    b = rng.integers(0, 4, size=(7, N_ENVS), dtype=np.uint8)
    counters = np.array([1000, 5], dtype=np.int64)
    _vote_host(a, live=live, dissent=counters)
    _vote_host(b, members=[0, 6], dissent=counters)
    assert counters.tolist() == (np.array([1000, 5]) + ER.vote(a, live=live)[2] + ER.vote(b, members=[0, 6])[2]).tolist()
    # an id outside the population and a byte that is no action cast no vote
    c = a.copy()
    c[3, :50] = 4 + (c[3, :50] & 3)
    ids = np.array([0, 7, 3, -1], dtype=np.int32)
    got = _vote_host(c, members=ids)
    want_rows = np.stack([c[0], np.where(c[3] < 4, c[3], 255)])
    assert got[1].tobytes() == np.stack([(want_rows == k).sum(axis=0) for k in range(4)], axis=1).astype(np.uint16).tobytes()
    assert got[2][1] == 2 * N_ENVS - 50


# ---- the command line -----------------------------------------------------------------------------------------------------------------
PPO_ARGS = ["ppo-mlp", "-l", "1e-3", "-r", "2", "-e", "2", "-b", "7"]
CNN_ARGS = ["ppo-cnn", "-l", "1e-3", "-r", "2", "-e", "2", "-b", "7"]
DQN_ARGS = ["deep-q", "-l", "1e-3"]


def _parse(core, agent):
    return S.prepare_parser().parse_args(core + ["boat"] + agent)


def test_the_ensemble_flag_parses_from_both_positions():
    behind = _parse(["-S", "3"], PPO_ARGS + ["--members", "3", "--ensemble-eval"])
    core = _parse(["-M", "3", "--ensemble-eval"], PPO_ARGS)
    for args in (behind, core):
        assert args.ensemble_eval is True and ensemble.check_ensemble_eval(args) is True
    assert ensemble.check_ensemble_eval(_parse(["-N", "12", "--ensemble-eval"], DQN_ARGS + ["-M", "3"])) is True
    assert ensemble.check_ensemble_eval(_parse(["-N", "12"], DQN_ARGS + ["-M", "3", "-EN"])) is True
    without = _parse([], PPO_ARGS + ["--members", "3"])
    assert without.ensemble_eval is False and ensemble.check_ensemble_eval(without) is False


def test_ensemble_refusals_are_plain_messages():
    with pytest.raises(SystemExit, match="--ensemble-eval needs --members"):
        ensemble.check_ensemble_eval(_parse([], PPO_ARGS + ["--ensemble-eval"]))
    with pytest.raises(SystemExit, match="--ensemble-eval needs --members"):
        ensemble.check_ensemble_eval(_parse(["--ensemble-eval", "-N", "8"], DQN_ARGS))
    for args in (_parse(["--ensemble-eval"], CNN_ARGS + ["--members", "3"]), _parse([], CNN_ARGS + ["--members", "3", "--ensemble-eval"]),
                 _parse(["--ensemble-eval"], CNN_ARGS)):
        with pytest.raises(SystemExit, match="ppo-mlp or deep-q agents, not 'ppo-cnn'"):
            ensemble.check_ensemble_eval(args)
    with pytest.raises(SystemExit, match="ppo-mlp or deep-q agents, not 'tabular-q'"):
        ensemble.check_ensemble_eval(_parse(["--ensemble-eval", "-N", "4"], ["tabular-q", "-l", "0.1"]))
    # the entry point stops before it makes a directory or touches a device
    from safe_grid_agents_amd.__main__ import main

    with pytest.raises(SystemExit, match="--ensemble-eval needs --members"):
        main(["-S", "3", "boat"] + PPO_ARGS + ["--ensemble-eval"])
    with pytest.raises(SystemExit, match="not 'ppo-cnn'"):
        main(["-S", "3", "boat"] + CNN_ARGS + ["--members", "3", "--ensemble-eval"])


def test_a_selection_is_validated_before_any_device():
    class Pop(ensemble.EnsembleMixin):
        n_members = 4
        _ens = {"selection": None}

    for members, message in (([], "selects nobody"), ([1, 1], "twice"), ([0, 4], "members 0 .. 3"), ([-1], "members 0 .. 3"), (3, "sequence")):
        with pytest.raises(ValueError, match=message):
            Pop()._ensemble_members(members)
