"""The tabular agents' consensus (include/sgk.h: sgk_tabq_consensus, sgk_tabq_load_shared, sgk_tabq_consensus_host;
safe_grid_agents_amd/consensus.py) as far as a box without a GPU can tell: the symbols are declared, exported and bound with the header's
signatures and the ABI version stays; the host vote -- the same rule, the same code as the kernel's -- equals the numpy restatement
(tests/consensus_reference.py) on random tables with all-zero rows, negative-only rows, exact ties, -0.0-only rows, every kind of
mask and agent counts around the wave size; NULL arguments and negative counts are refused with a message; the --consensus-eval
grammar and its four refusals; and the restatement itself against cases worked out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import consensus_reference as CR
import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib, consensus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, I64 = ctypes.c_void_p, ctypes.c_int64


def _header():
    return open(os.path.join(ROOT, "include", "sgk.h")).read()


def _declared(name):
    m = re.search(r"SGK_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "include/sgk.h does not declare int %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _vote_host(tables, mask=None, with_voters=True):
    """sgk_tabq_consensus_host -> (votes, voters); the outputs start out as garbage: the call overwrites them."""
    t = np.ascontiguousarray(tables, dtype=np.float64)
    A, ns, _ = t.shape
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    votes, voters = np.full((ns, 4), -77, dtype=np.int64), np.full(ns, -55, dtype=np.int64)
    rc = _lib.load().sgk_tabq_consensus_host(t.ctypes.data, A, ns, None if m is None else m.ctypes.data, votes.ctypes.data,
                                             voters.ctypes.data if with_voters else None)
    assert rc == _lib.SGK_OK, _lib.load().sgk_last_error()
    return votes, voters


def _tables(rng, A, ns):
    """Random tables with every special row planted on purpose (as far as A x ns has room): all zeros, negatives only, exact ties
    between the actions (0, 2) and (1, 3), -0.0 only, a lone non-zero entry, a -0.0 among zeros and one negative."""
    t = rng.standard_normal((A, ns, 4))
    t[rng.random((A, ns)) < 0.25] = 0.0                      # rows never learnt
    special = [np.zeros(4), np.array([-1.5, -0.25, -3.0, -0.25]), np.array([2.0, 1.0, 2.0, -1.0]), np.array([0.5, 3.0, -2.0, 3.0]),
               np.array([-0.0, -0.0, -0.0, -0.0]), np.array([0.0, 0.0, 0.0, 1e-300]), np.array([-0.0, 0.0, -4.0, 0.0]),
               np.array([-2.0, -2.0, -2.0, -2.0])]
    flat = t.reshape(-1, 4)
    where = rng.permutation(len(flat))[:len(special)]
    for i, row in zip(where, special):
        flat[i] = row
    return t


# ---- the restatement itself, against cases worked out by hand -------------------------------------------------------------------------
def test_the_reference_on_hand_written_cases():
    t = np.zeros((3, 4, 4))
    t[0, 0] = (1.0, 2.0, 2.0, 0.0)    # tie 1-2: the first, 1
    t[1, 0] = (-1.0, -3.0, -1.0, -2.0)  # negatives, tie 0-2: 0
    t[2, 0] = (0.0, 0.0, 0.0, 5.0)    # 3
    t[0, 1] = (-0.0, -0.0, -0.0, -0.0)  # no vote
    t[1, 1] = (0.0, -1.0, 0.0, 0.0)   # a vote for 0: the zeros ARE the maximum of a learnt row
    t[2, 2] = (0.0, 0.0, 7.0, 7.0)    # 2
    votes, voters = CR.vote(t)
    assert votes.tolist() == [[1, 1, 0, 1], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]] and voters.tolist() == [3, 1, 1, 0]
    assert CR.policy(votes).tolist() == [0, 0, 2, 0]
    votes, voters = CR.vote(t, mask=[0, 1, 255])
    assert votes.tolist() == [[1, 0, 0, 1], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]] and voters.tolist() == [2, 1, 1, 0]
    assert votes.dtype == np.int64 and voters.dtype == np.int64


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    assert _declared("sgk_tabq_consensus") == ["sgk_tabq *q", "const uint8_t *voters_mask_dev", "int64_t *votes_out_dev",
                                               "int64_t *voters_out_dev"]
    assert _declared("sgk_tabq_load_shared") == ["sgk_tabq *q", "const double *table_dev"]
    assert _declared("sgk_tabq_consensus_host") == ["const double *table_host", "int64_t n_agents", "int64_t n_states",
                                                    "const uint8_t *voters_mask_host", "int64_t *votes_out_host", "int64_t *voters_out_host"]
    want = {"sgk_tabq_consensus": (ctypes.c_int, [V, V, V, V]),
            "sgk_tabq_load_shared": (ctypes.c_int, [V, V]),
            "sgk_tabq_consensus_host": (ctypes.c_int, [V, I64, I64, V, V, V])}
    lib = _lib.load()  # (resolves every bound symbol in libsgk.so: a missing export is an AttributeError here)
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name] == (res, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert lib.sgk_abi_version() == 4  # added symbols: the ABI version stays
    header = " ".join(_header().split())
    for promise in ("-0.0 counts as zero", "the first maximum, as np.argmax picks", "OVERWRITTEN", "No allocation, no host synchronisation"):
        assert promise in header, promise
    assert "sgk_tabq_consensus.hip" in open(os.path.join(ROOT, "safe-grid-agents_amd", "csrc", "Makefile")).read()


def test_null_arguments_and_negative_counts_are_refused_with_a_message():
    lib = _lib.load()
    t = np.ones((2, 3, 4))
    votes, voters = np.full((3, 4), 9, dtype=np.int64), np.full(3, 9, dtype=np.int64)
    tp, vp, wp = t.ctypes.data, votes.ctypes.data, voters.ctypes.data
    for args, message in (((None, 2, 3, None, vp, wp), b"table_host is NULL"), ((tp, 2, 3, None, None, wp), b"votes_out_host is NULL"),
                          ((None, 0, 0, None, None, None), b"NULL"), ((tp, -1, 3, None, vp, wp), b"n_agents < 0"),
                          ((tp, 2, -3, None, vp, wp), b"n_states < 0")):
        assert lib.sgk_tabq_consensus_host(*args) == _lib.ERR_INVALID, message
        assert message in lib.sgk_last_error(), (message, lib.sgk_last_error())
    assert (votes == 9).all() and (voters == 9).all()  # nothing was written
    # the device calls: a NULL handle is refused for the handle, whatever else is given
    assert lib.sgk_tabq_consensus(None, None, vp, wp) == _lib.ERR_INVALID and b"handle is NULL" in lib.sgk_last_error()
    assert lib.sgk_tabq_consensus(None, None, None, None) == _lib.ERR_INVALID and b"handle is NULL" in lib.sgk_last_error()
    assert lib.sgk_tabq_load_shared(None, tp) == _lib.ERR_INVALID and b"handle is NULL" in lib.sgk_last_error()
    assert lib.sgk_tabq_load_shared(None, None) == _lib.ERR_INVALID and b"handle is NULL" in lib.sgk_last_error()
    # no agents, no states: nothing to count is not an error
    assert lib.sgk_tabq_consensus_host(tp, 0, 3, None, vp, wp) == _lib.SGK_OK and (votes == 0).all() and (voters == 0).all()
    assert lib.sgk_tabq_consensus_host(tp, 2, 0, None, vp, None) == _lib.SGK_OK


# ---- the host vote ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 25, 48])
@pytest.mark.parametrize("A", [1, 63, 64, 65, 200])
def test_the_host_vote_equals_the_reference(A, ns):
    rng = np.random.default_rng(100 * A + ns)
    t = _tables(rng, A, ns)
    one = np.zeros(A, dtype=np.uint8)
    one[A - 1] = 1  # a single voter: the last agent
    some = rng.integers(0, 2, size=A).astype(np.uint8)
    some[0] = 255   # any non-zero byte may vote
    for mask in (None, np.ones(A, dtype=np.uint8), np.zeros(A, dtype=np.uint8), one, some):
        votes, voters = _vote_host(t, mask)
        want_votes, want_voters = CR.vote(t, mask)
        assert votes.tobytes() == want_votes.tobytes(), (A, ns, mask)
        assert voters.tobytes() == want_voters.tobytes(), (A, ns, mask)
        assert (votes.sum(axis=1) == voters).all()
    assert _vote_host(t, np.zeros(A, dtype=np.uint8))[0].sum() == 0
    assert _vote_host(t, one)[1].max() <= 1
    votes_only, untouched = _vote_host(t, with_voters=False)  # voters_out is optional
    assert votes_only.tobytes() == CR.vote(t)[0].tobytes() and (untouched == -55).all()


def test_zero_rows_negative_rows_ties_and_negative_zero_by_hand():
    rows = {
        "never learnt": ([0.0, 0.0, 0.0, 0.0], None), "-0.0 only": ([-0.0, -0.0, -0.0, -0.0], None), "mixed zeros": ([0.0, -0.0, 0.0, -0.0], None),
        "negatives": ([-3.0, -1.0, -2.0, -1.0], 1), "all equal negatives": ([-2.0, -2.0, -2.0, -2.0], 0),
        "tie 0-2": ([4.0, 1.0, 4.0, 0.0], 0), "tie 1-3": ([0.5, 3.0, -2.0, 3.0], 1), "learnt below zero": ([0.0, -1.0, 0.0, 0.0], 0),
        "-0.0 before a zero": ([-4.0, -0.0, 0.0, -1.0], 1), "tiny": ([0.0, 0.0, 0.0, 5e-324], 3), "inf": ([1.0, np.inf, np.inf, 0.0], 1),
    }
    for name, (row, action) in rows.items():
        t = np.array(row, dtype=np.float64).reshape(1, 1, 4)
        votes, voters = _vote_host(t)
        want = [0, 0, 0, 0]
        if action is not None:
            want[action] = 1
        assert votes[0].tolist() == want and voters[0] == (action is not None), name
        assert votes.tobytes() == CR.vote(t)[0].tobytes(), name


# ---- the Python surface that needs no device ----------------------------------------------------------------------------------------
def test_the_agent_has_the_consensus_surface():
    for name in ("consensus", "load_shared_table", "consensus_agent", "evaluate_consensus"):
        assert callable(getattr(S.BatchedTabularQAgent, name)), name
    assert issubclass(S.BatchedTabularQAgent, consensus.ConsensusMixin)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
TABQ = ["tabular-q", "-l", "0.5"]


def _parse(core, agent, env="boat"):
    return S.prepare_parser().parse_args(core + [env] + agent)


def test_the_consensus_flag_parses_from_both_positions_and_is_absent_without_it():
    behind = _parse(["-S", "3", "-N", "64"], TABQ + ["--consensus-eval"])
    core = _parse(["-N", "64", "--consensus-eval"], TABQ)
    short = _parse(["-N", "64"], TABQ + ["-CE"])
    for args in (behind, core, short):
        assert args.consensus_eval is True and consensus.check_consensus_eval(args) is True
    without = _parse(["-N", "64"], TABQ)
    assert not hasattr(without, "consensus_eval") and consensus.check_consensus_eval(without) is False  # nothing changes without it


def test_consensus_refusals_are_plain_messages():
    with pytest.raises(SystemExit, match="private tabular-q agents, not 'deep-q'"):
        consensus.check_consensus_eval(_parse(["-N", "64", "--consensus-eval"], ["deep-q", "-l", "1e-3"]))
    with pytest.raises(SystemExit, match="private tabular-q agents, not 'ppo-mlp'"):
        consensus.check_consensus_eval(_parse(["--consensus-eval"], ["ppo-mlp", "-l", "1e-3", "-r", "2", "-e", "2"]))
    with pytest.raises(SystemExit, match="cannot run on tomato"):
        consensus.check_consensus_eval(_parse(["-N", "64"], TABQ + ["--consensus-eval"], env="tomato"))
    for core in (["-N", "1"], []):
        with pytest.raises(SystemExit, match="--consensus-eval needs -N > 1"):
            consensus.check_consensus_eval(_parse(core, TABQ + ["--consensus-eval"]))
    with pytest.raises(SystemExit, match="runs on one device"):
        consensus.check_consensus_eval(_parse(["-N", "64", "--devices", "2"], TABQ + ["--consensus-eval"]))
    # the entry point stops before it makes a directory or touches a device
    from safe_grid_agents_amd.__main__ import main

    with pytest.raises(SystemExit, match="--consensus-eval needs -N > 1"):
        main(["-S", "3", "-N", "1", "boat"] + TABQ + ["--consensus-eval"])
    with pytest.raises(SystemExit, match="not 'deep-q'"):
        main(["-S", "3", "-N", "8", "--consensus-eval", "boat", "deep-q", "-l", "1e-3"])
    with pytest.raises(SystemExit, match="cannot run on tomato"):
        main(["-S", "3", "-N", "8", "tomato"] + TABQ + ["--consensus-eval"])
    with pytest.raises(SystemExit, match="runs on one device"):
        main(["-S", "3", "-N", "8", "--devices", "2", "boat"] + TABQ + ["--consensus-eval"])
