"""The hashed levels' consensus by board key (include/sgk.h: sgk_tabq_hash_consensus, sgk_tabq_hash_load_shared and their host
restatements; safe_grid_agents_amd/consensus.py) as far as a box without a GPU can tell: the dictionary restatement
(tests/hash_consensus_reference.py) against cases worked out by hand; the symbols are declared, exported and bound with the header's
signatures and the ABI version stays; every field of the descriptor names a guard-band case of tests/test_gpu_hash_consensus.py; the host
vote -- the same rule, the same code as the kernels' -- equals the restatement on synthetic tables and on the 322-agent dictionary run,
whose properties are asserted first; the host load equals a dictionary's sequential insertion; refusals carry a message; the
--hash-consensus-eval grammar and its refusals, and the pinned refusals of --consensus-eval."""
import ctypes
import importlib
import os
import re
from collections import Counter

import numpy as np
import pytest

import hash_consensus_reference as HC
import hash_grow_plans as HP
import hashed_tabq_reference as HR
import safe_grid_agents_amd as S
import test_tabq_consensus_abi as TA
from safe_grid_agents_amd import _lib, consensus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
EMPTY = HC.EMPTY
DELUSION = 0x200000 | 10  # a delusion board: shown = 0x2000, bit 21 of the key
POOL = [0, 0x3F, 0x40, 0x1FFFFF, DELUSION, 0x13, 0x200010, 0x3FFFFF, 0x41, 0x7F, 0x80, 0x1234, 0x100000]

# Every pointer of sgk_tabq_hash_votes the library writes through -> the guard-band tests of tests/test_gpu_hash_consensus.py that carve it
# from a guard_arena.Arena. (The descriptor is passed by const pointer, so tests/test_guard_arena_cpu.py's parser does not see its fields;
# this table is that file's COVERED for them.)
VOTES_COVERED = {
    "sgk_tabq_hash_votes.keys": ("test_gpu_hash_consensus.test_the_vote_and_the_load_stay_inside_their_guard_bands",),
    "sgk_tabq_hash_votes.votes": ("test_gpu_hash_consensus.test_the_vote_and_the_load_stay_inside_their_guard_bands",),
    "sgk_tabq_hash_votes.voters": ("test_gpu_hash_consensus.test_the_vote_and_the_load_stay_inside_their_guard_bands",),
    "sgk_tabq_hash_votes.count": ("test_gpu_hash_consensus.test_the_vote_and_the_load_stay_inside_their_guard_bands",),
    "sgk_tabq_hash_votes.workspace": ("test_gpu_hash_consensus.test_the_vote_and_the_load_stay_inside_their_guard_bands",),
}


def _header():
    return open(os.path.join(ROOT, "include", "sgk.h")).read()


def _declared(name, result="int"):
    m = re.search(r"SGK_API\s+%s\s+%s\s*\(([^)]*)\)\s*;" % (result, name), _header())
    assert m, "include/sgk.h does not declare %s %s" % (result, name)
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    return [" ".join(d.split()) for d in body.split(";") if d.strip()]


# ---- the restatement itself, against cases worked out by hand -------------------------------------------------------------------------
def test_the_reference_on_hand_written_cases():
    agents = [
        {5: [1.0, 2.0, 2.0, 0.0], 9: [-0.0, -0.0, -0.0, -0.0], 7: [0.0, 0.0, 0.0, 0.0]},    # tie 1-2: 1; a -0.0 row and a zero row: no vote
        {5: [-1.0, -3.0, -1.0, -2.0], 9: [0.0, -1.0, 0.0, 0.0]},                            # negatives, tie 0-2: 0; a learnt row: 0
        {5: [0.0, 0.0, 0.0, 5.0], 0x200010: [0.0, 0.0, 7.0, 7.0], 7: [-0.0, 0.0, 0.0, 0.0]},  # 3; tie 2-3: 2
    ]
    votes = HC.vote(agents)
    assert votes == {5: [1, 1, 0, 1], 9: [1, 0, 0, 0], 0x200010: [0, 0, 1, 0]}  # key 7: claimed twice, voted by nobody, absent
    assert HC.vote(agents, mask=[0, 1, 255]) == {5: [1, 0, 0, 1], 9: [1, 0, 0, 0], 0x200010: [0, 0, 1, 0]}
    assert HC.vote(agents, mask=[1, 0, 0]) == {5: [0, 1, 0, 0]}
    keys, counts, voters, U = HC.arrays(votes, 5)
    assert keys.tolist() == [5, 9, 0x200010, EMPTY, EMPTY] and U == 3 and voters.tolist() == [3, 1, 1, 0, 0]
    assert counts.tolist() == [[1, 1, 0, 1], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    keys, counts, voters, U = HC.arrays(votes, 2)  # truncated: the first two keys in ascending order, U is the true number
    assert keys.tolist() == [5, 9] and counts.tolist() == [[1, 1, 0, 1], [1, 0, 0, 0]] and U == 3
    assert HC.policy(counts).tolist() == [0, 0]
    table, dropped = HC.load([4, 8, 4, EMPTY, 6, 2], [[1.0] * 4, [2.0] * 4, [3.0] * 4, [9.0] * 4, [4.0] * 4, [5.0] * 4], capacity=3)
    assert table == {4: [3.0] * 4, 8: [2.0] * 4, 6: [4.0] * 4} and dropped == [2]  # the duplicate takes the later row, the fourth key is dropped


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    assert _declared("sgk_tabq_hash_consensus_workspace_bytes", "int64_t") == ["sgk_tabq *q"]
    assert _declared("sgk_tabq_hash_consensus") == ["sgk_tabq *q", "const uint8_t *voters_mask_dev", "const sgk_tabq_hash_votes *out"]
    assert _declared("sgk_tabq_hash_load_shared") == ["sgk_tabq *q", "const uint8_t *agents_mask_dev", "const uint32_t *keys_dev",
                                                      "const double *rows_dev", "const int64_t *count_dev", "int64_t max_keys",
                                                      "const sgk_tabq_hash_votes *scratch"]
    assert _declared("sgk_tabq_hash_consensus_host") == ["const uint32_t *keys_host", "const double *rows_host", "int64_t n_agents",
                                                         "int32_t capacity", "const uint8_t *voters_mask_host", "const sgk_tabq_hash_votes *out"]
    assert _declared("sgk_tabq_hash_load_shared_host") == ["const uint32_t *keys_in", "const double *rows_in", "int64_t count",
                                                           "int32_t capacity", "const sgk_tabq_hash_table *out"]
    assert _struct_fields("sgk_tabq_hash_votes") == ["uint32_t *keys", "int64_t *votes", "int64_t *voters", "int64_t *count", "int64_t max_keys",
                                                     "void *workspace", "int64_t workspace_bytes"]
    assert _struct_fields("sgk_tabq_hash_table") == ["uint32_t *keys", "double *rows", "int32_t *overflowed"]
    assert [k for k, _ in _lib.SgkTabqHashVotes._fields_] == ["keys", "votes", "voters", "count", "max_keys", "workspace", "workspace_bytes"]
    assert ctypes.sizeof(_lib.SgkTabqHashVotes) == 7 * 8 and ctypes.sizeof(_lib.SgkTabqHashTable) == 3 * 8
    VP, TP = ctypes.POINTER(_lib.SgkTabqHashVotes), ctypes.POINTER(_lib.SgkTabqHashTable)
    want = {"sgk_tabq_hash_consensus_workspace_bytes": (I64, [V]),
            "sgk_tabq_hash_consensus": (ctypes.c_int, [V, V, VP]),
            "sgk_tabq_hash_load_shared": (ctypes.c_int, [V, V, V, V, V, I64, VP]),
            "sgk_tabq_hash_consensus_host": (ctypes.c_int, [V, V, I64, I32, V, VP]),
            "sgk_tabq_hash_load_shared_host": (ctypes.c_int, [V, V, I64, I32, TP])}
    lib = _lib.load()  # (resolves every bound symbol in libsgk.so: a missing export is an AttributeError here)
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name] == (res, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert lib.sgk_abi_version() == 4  # added symbols: the ABI version stays
    header = " ".join(_header().split())
    assert "#define SGK_TABQ_HASH_KEY_BITS 22" in header
    for promise in ("in ASCENDING order", "*count still says U", "A key nobody votes on is ABSENT", "a later duplicate key overwrites the earlier row",
                    "Agents not selected keep every byte", "count_dev is read ON THE DEVICE", "nothing indexes past the bitmap"):
        assert promise in header, promise
    csrc = os.path.join(ROOT, "safe-grid-agents_amd", "csrc")
    assert "sgk_tabq_hash_consensus.hip" in open(os.path.join(csrc, "Makefile")).read()
    # ONE vote_of_row, in the header both files include
    assert "vote_of_row(double" in open(os.path.join(csrc, "sgk_tabq_vote.h")).read()
    for f in ("sgk_tabq_consensus.hip", "sgk_tabq_hash_consensus.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "sgk_tabq_vote.h"' in text and "int vote_of_row(" not in text, f


def test_every_field_of_the_descriptor_names_a_guard_band_test():
    pointers = [d for d in _struct_fields("sgk_tabq_hash_votes") if "*" in d]
    assert all("const" not in d.split("*")[0].split() for d in pointers)
    assert sorted("sgk_tabq_hash_votes." + d.split("*")[1].strip() for d in pointers) == sorted(VOTES_COVERED)
    for key, tests in VOTES_COVERED.items():
        assert tests, key
        for t in tests:
            module, _, name = t.rpartition(".")
            owner = importlib.import_module(module)
            assert callable(getattr(owner, name, None)) and name.startswith("test_"), (key, t)
            src = open(owner.__file__).read()
            assert "guard_arena" in src and '"%s"' % key.split(".")[1] in src, (key, t)
    # and the parameters themselves stay out of the header-wide tables' reach: const
    for fn in ("sgk_tabq_hash_consensus", "sgk_tabq_hash_load_shared", "sgk_tabq_hash_consensus_host", "sgk_tabq_hash_load_shared_host"):
        assert all("*" not in p or p.startswith("const ") or p == "sgk_tabq *q" for p in _declared(fn)), fn


# ---- the host vote on synthetic tables ----------------------------------------------------------------------------------------------
def _synthetic(rng, A, cap):
    """keys [A, cap], rows [A, cap, 4]: every agent holds a random subset of POOL and of a few random keys at RANDOM slots (the same key
    at different slots in different agents); the rows carry every special row of test_tabq_consensus_abi._tables."""
    rows = TA._tables(rng, A, cap)
    keys = np.full((A, cap), EMPTY, dtype=np.uint32)
    extra = rng.integers(0, 1 << 22, size=40).tolist()
    for e in range(A):
        mine = [k for k in POOL + extra if rng.random() < 0.6]
        if e == 0:
            mine = list(POOL) + extra[:8]
        slots = rng.permutation(cap)[:len(mine)]
        keys[e, slots] = mine
    rows[keys == EMPTY] = rng.standard_normal(4)  # what an empty slot's row holds must not matter
    return keys, rows


def _assert_vote(keys, rows, mask, max_keys=None):
    want = HC.vote(HC.tables_as_dicts(keys, rows), mask)
    U = len(want)
    for K in ([max(U, 1), U + 7] + ([U - 3] if U > 3 else [])) if max_keys is None else [max_keys]:
        got = HC.host_vote(keys, rows, mask, max_keys=K)
        wk, wv, ww, wu = HC.arrays(want, K)
        assert got[3] == wu == U
        assert got[0].tobytes() == wk.tobytes() and got[1].tobytes() == wv.tobytes() and got[2].tobytes() == ww.tobytes(), (K, U)
    return want


@pytest.mark.parametrize("cap", [64, 128])
@pytest.mark.parametrize("A", [1, 63, 64, 65, 257])
def test_the_host_vote_equals_the_dictionary_on_synthetic_tables(A, cap):
    rng = np.random.default_rng(1000 * A + cap)
    keys, rows = _synthetic(rng, A, cap)
    one = np.zeros(A, dtype=np.uint8)
    one[A - 1] = 1
    some = rng.integers(0, 2, size=A).astype(np.uint8)
    some[0] = 255  # any non-zero byte may vote
    want = None
    for mask in (None, np.ones(A, dtype=np.uint8), np.zeros(A, dtype=np.uint8), one, some):
        got = _assert_vote(keys, rows, mask)
        want = got if mask is None else want
    for k in (0, 0x3F, 0x40, 0x1FFFFF, DELUSION):  # the bitmap's first bit, a word's last and the next word's first, bit 21
        assert k in {int(x) for x in keys[0]}
    assert len(want) >= 5  # (agent 0 alone holds 21 keys, a quarter of them with rows never learnt)
    # the same key at different slots in different agents
    if A > 1:
        where = [set(np.nonzero(keys[e] == 0x3F)[0].tolist()) for e in range(A)]
        assert len(set().union(*where)) > 1
    votes_only = HC.host_vote(keys, rows, None, with_voters=False)  # voters is optional: untouched
    assert votes_only[1].tobytes() == HC.arrays(want, A * cap)[1].tobytes() and (votes_only[2] == -55).all()


def test_the_special_rows_vote_as_the_state_vote_says():
    rows = np.array([[0.0, 0.0, 0.0, 0.0], [-0.0, -0.0, -0.0, -0.0], [-3.0, -1.0, -2.0, -1.0], [4.0, 1.0, 4.0, 0.0], [0.5, 3.0, -2.0, 3.0],
                     [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 5e-324], [1.0, np.inf, np.inf, 0.0]])
    action = [None, None, 1, 0, 1, 0, 3, 1]
    keys = np.full((1, 64), EMPTY, dtype=np.uint32)
    table = np.zeros((1, 64, 4))
    keys[0, 10:18] = np.arange(100, 108)
    table[0, 10:18] = rows
    out_keys, votes, voters, U = HC.host_vote(keys, table, max_keys=8)
    assert U == 6 and out_keys.tolist() == [102, 103, 104, 105, 106, 107, EMPTY, EMPTY]
    assert votes[:6].argmax(axis=1).tolist() == action[2:] and voters.tolist() == [1] * 6 + [0, 0]
    # a key that cannot be (>= 1 << 22, not the empty marker) is skipped
    keys[0, 30], table[0, 30] = 1 << 22, (1.0, 0.0, 0.0, 0.0)
    keys[0, 31], table[0, 31] = 0xFFFFFFFE, (1.0, 0.0, 0.0, 0.0)
    assert HC.host_vote(keys, table, max_keys=8)[3] == 6


# ---- the 322-agent dictionary run ---------------------------------------------------------------------------------------------------
def run_dicts():
    """The cached 322-agent run (capacity 64, 99 steps, the fused rollout's order) as one {key: row} per agent."""
    _, agents, _ = HR.run(64, 99, claim_start_on_reset=True)
    R = HP.rules()
    return agents, [{HP.board_key(R, b): list(r) for b, r in a.rows.items()} for a in agents]


def arrays_of(dicts, cap, rng=None):
    """[A, cap] keys and [A, cap, 4] rows holding the dictionaries, each agent's boards at slots of its own."""
    rng = rng or np.random.default_rng(7)
    keys, rows = np.full((len(dicts), cap), EMPTY, dtype=np.uint32), np.zeros((len(dicts), cap, 4))
    for e, d in enumerate(dicts):
        slots = rng.permutation(cap)[:len(d)]
        keys[e, slots] = list(d)
        rows[e, slots] = list(d.values())
    return keys, rows


def test_the_dictionary_run_provides_what_the_vote_must_face():
    """The conditions the issue lists, recomputed from the dictionary alone (profiles/hash_consensus/coverage.log has the same values): a
    weaker input cannot pass silently."""
    agents, dicts = run_dicts()
    assert len(dicts) == 322
    claimed = set().union(*dicts)
    votes = HC.vote(dicts)
    assert len(claimed) == 10064 and len(votes) == 10044 and len(claimed) - len(votes) == 20
    zero_and_voted = sum(1 for k in votes if any(k in d and not any(q != 0.0 for q in d[k]) for d in dicts))
    assert zero_and_voted == 108
    cast = {k: sum(c) for k, c in votes.items()}
    assert max(cast.values()) == 322 and sum(1 for c in cast.values() if c == 1) == 6920 and sum(cast.values()) == 18942
    assert sum(1 for c in votes.values() if sorted(c)[-1] == sorted(c)[-2]) == 1647  # the first-maximum rule decides
    assert min(votes) == 0x13 and max(votes) == 0x200010
    words = Counter(k >> 6 for k in votes)
    assert len(words) == 2094 and max(words.values()) == 28 and 0 in words
    assert [len(c) for c in HR.classes(agents)] == [184, 16, 122]  # room / exactly full / refused: all three classes vote
    assert len(HC.vote(dicts, [e % 3 == 0 for e in range(322)])) == 4445
    assert len(HC.vote(dicts, [e == 7 for e in range(322)])) == 61


def test_the_host_vote_equals_the_dictionary_on_the_322_agent_run():
    _, dicts = run_dicts()
    keys, rows = arrays_of(dicts, 64)
    for mask in (None, np.arange(322) % 3 == 0, np.arange(322) == 7):
        want = _assert_vote(keys, rows, mask)
    assert len(want) == 61
    _assert_vote(keys, rows, None, max_keys=4096)  # below U: the first 4 096 keys, count = U


# ---- the host load ------------------------------------------------------------------------------------------------------------------
def test_the_host_load_equals_sequential_insertion_into_a_dictionary():
    rng = np.random.default_rng(11)
    keys = rng.permutation(1 << 22)[:100].astype(np.uint32)
    keys[40], keys[77] = keys[3], keys[3]     # a key three times: the last row stays
    keys[50] = EMPTY                          # the empty marker names no board
    rows = rng.standard_normal((100, 4))
    rows[5] = 0.0
    for cap in (128, 256):
        got_keys, got_rows, over = HC.host_load(keys, rows, cap)
        want, dropped = HC.load(keys, rows, cap)
        assert not over and not dropped and HC.table_as_dict(got_keys, got_rows) == want and len(want) == 97
        assert want[int(keys[3])] == rows[77].tolist()
        assert (got_rows[got_keys == EMPTY] == 0.0).all() and int((got_keys != EMPTY).sum()) == 97
    # a prefix only
    got_keys, got_rows, over = HC.host_load(keys, rows, 128, count=30)
    assert HC.table_as_dict(got_keys, got_rows) == HC.load(keys[:30], rows[:30], 128)[0]
    # more distinct keys than slots: exactly the keys a sequential insertion drops are missing, and the overflow is reported
    got_keys, got_rows, over = HC.host_load(keys, rows, 64)
    want, dropped = HC.load(keys, rows, 64)
    assert over == 1 and len(dropped) == 97 - 64 and HC.table_as_dict(got_keys, got_rows) == want and len(want) == 64
    assert int(keys[77]) in want and want[int(keys[77])] == rows[77].tolist()  # admitted early, overwritten late: still the later row
    # nothing to insert: an empty table
    got_keys, got_rows, over = HC.host_load(keys, rows, 64, count=0)
    assert (got_keys == EMPTY).all() and (got_rows == 0.0).all() and over == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_a_message_and_nothing_is_written():
    lib = _lib.load()
    keys, rows = np.full((2, 64), EMPTY, dtype=np.uint32), np.ones((2, 64, 4))
    ok, ov, ow, oc = np.full(8, 9, dtype=np.uint32), np.full((8, 4), 9, dtype=np.int64), np.full(8, 9, dtype=np.int64), np.full(1, 9, dtype=np.int64)

    def desc(keys_p=ok.ctypes.data, votes_p=ov.ctypes.data, voters_p=ow.ctypes.data, count_p=oc.ctypes.data, K=8, ws_p=None, ws_n=0):
        return ctypes.byref(_lib.SgkTabqHashVotes(keys_p, votes_p, voters_p, count_p, K, ws_p, ws_n))

    kp, rp = keys.ctypes.data, rows.ctypes.data
    for args, message in (((kp, rp, 2, 64, None, None), b"out is NULL"), ((kp, rp, 2, 64, None, desc(keys_p=None)), b"out->keys is NULL"),
                          ((kp, rp, 2, 64, None, desc(votes_p=None)), b"out->votes is NULL"), ((kp, rp, 2, 64, None, desc(count_p=None)), b"out->count is NULL"),
                          ((kp, rp, 2, 64, None, desc(K=0)), b"max_keys < 1"), ((None, rp, 2, 64, None, desc()), b"keys_host is NULL"),
                          ((kp, None, 2, 64, None, desc()), b"rows_host is NULL"), ((kp, rp, -1, 64, None, desc()), b"n_agents < 0"),
                          ((kp, rp, 2, 0, None, desc()), b"capacity < 1"), ((kp, rp, 2, 64, None, desc(votes_p=ov.ctypes.data + 4)), b"8-byte aligned"),
                          ((kp, rp, 2, 64, None, desc(keys_p=ok.ctypes.data + 2)), b"4-byte aligned")):
        assert lib.sgk_tabq_hash_consensus_host(*args) == _lib.ERR_INVALID, message
        assert message in lib.sgk_last_error(), (message, lib.sgk_last_error())
    assert (ok == 9).all() and (ov == 9).all() and (ow == 9).all() and (oc == 9).all()
    assert lib.sgk_tabq_hash_consensus_workspace_bytes(None) == _lib.ERR_INVALID and b"handle is NULL" in lib.sgk_last_error()
    # the host load
    tk, tr = np.full(64, 9, dtype=np.uint32), np.full((64, 4), 9.0)

    def table(keys_p=tk.ctypes.data, rows_p=tr.ctypes.data):
        return ctypes.byref(_lib.SgkTabqHashTable(keys_p, rows_p, None))

    for args, message in (((kp, rp, 4, 64, None), b"out is NULL"), ((kp, rp, 4, 64, table(keys_p=None)), b"out->keys is NULL"),
                          ((kp, rp, 4, 64, table(rows_p=None)), b"out->rows is NULL"), ((kp, rp, -1, 64, table()), b"count < 0"),
                          ((None, rp, 4, 64, table()), b"keys_in is NULL"), ((kp, None, 4, 64, table()), b"rows_in is NULL"),
                          ((kp, rp, 4, 96, table()), b"power of two"), ((kp, rp, 4, 32, table()), b"power of two")):
        assert lib.sgk_tabq_hash_load_shared_host(*args) == _lib.ERR_INVALID, message
        assert message in lib.sgk_last_error(), (message, lib.sgk_last_error())
    assert (tk == 9).all() and (tr == 9.0).all()


def test_the_device_calls_refuse_every_bad_argument_before_the_handle_is_looked_at():
    """The handle is NULL in every call: a refusal that names the bad argument was made before the handle was looked at, so the same
    check guards a real handle. Valid arguments with a NULL handle are refused for the handle. (A workspace that is too SMALL needs the
    handle's capacity: tests/test_gpu_hash_consensus.py.)"""
    lib = _lib.load()
    ok, ov, oc = np.full(8, 9, dtype=np.uint32), np.full((8, 4), 9, dtype=np.int64), np.full(1, 9, dtype=np.int64)
    rows, ws = np.zeros((8, 4)), np.zeros(4096, dtype=np.uint8)
    base = ws.ctypes.data + (-ws.ctypes.data) % 16

    def desc(**kw):
        f = dict(keys=ok.ctypes.data, votes=ov.ctypes.data, voters=None, count=oc.ctypes.data, max_keys=8, workspace=base, workspace_bytes=2048)
        f.update(kw)
        return ctypes.byref(_lib.SgkTabqHashVotes(*[f[k] for k, _ in _lib.SgkTabqHashVotes._fields_]))

    for d, message in ((None, b"out is NULL"), (desc(keys=None), b"out->keys is NULL"), (desc(votes=None), b"out->votes is NULL"),
                       (desc(count=None), b"out->count is NULL"), (desc(max_keys=0), b"max_keys < 1"), (desc(workspace=None), b"workspace is NULL"),
                       (desc(workspace=base + 8), b"workspace must be 16-byte aligned"), (desc(count=oc.ctypes.data + 4), b"8-byte aligned"),
                       (desc(), b"handle is NULL")):
        assert lib.sgk_tabq_hash_consensus(None, None, d) == _lib.ERR_INVALID, message
        assert message in lib.sgk_last_error(), (message, lib.sgk_last_error())
    kp, rp, cp = ok.ctypes.data, rows.ctypes.data, oc.ctypes.data
    for args, message in (((None, rp, cp, 8, desc()), b"keys_dev is NULL"), ((kp, None, cp, 8, desc()), b"rows_dev is NULL"),
                          ((kp, rp, None, 8, desc()), b"count_dev is NULL"), ((kp, rp, cp, 0, desc()), b"max_keys must be in 1"),
                          ((kp, rp, cp, 1 << 31, desc()), b"max_keys must be in 1"), ((kp, rp, cp, 8, None), b"scratch is NULL"),
                          ((kp, rp, cp, 8, desc(workspace=None)), b"scratch->workspace is NULL"),
                          ((kp, rp, cp, 8, desc(workspace=base + 4)), b"scratch->workspace must be 16-byte aligned"),
                          ((kp + 2, rp, cp, 8, desc()), b"keys_dev must be 4-byte aligned"), ((kp, rp, cp, 8, desc()), b"handle is NULL")):
        assert lib.sgk_tabq_hash_load_shared(None, None, *args) == _lib.ERR_INVALID, message
        assert message in lib.sgk_last_error(), (message, lib.sgk_last_error())
    assert (ok == 9).all() and (ov == 9).all() and (oc == 9).all() and (ws == 0).all()


# ---- the Python surface that needs no device ----------------------------------------------------------------------------------------
def test_the_agent_has_the_hashed_consensus_surface():
    for name in ("hash_consensus", "load_shared_hash_table", "hash_consensus_agent", "evaluate_hash_consensus"):
        assert callable(getattr(S.BatchedTabularQAgent, name)), name
    for name in ("n_keys", "agreement", "as_dict"):
        assert callable(getattr(consensus.HashedConsensus, name)), name
    assert isinstance(consensus.HashedConsensus.policy, property)
    cap = S.BatchedTabularQAgent._hash_capacity_for
    assert [cap(0, 0), cap(63, 0), cap(64, 0), cap(10044, 0), cap(10044, 109), cap(16383, 0), cap(16382, 1)] == [64, 64, 128, 16384, 16384, 16384, 32768]


# ---- the command line -----------------------------------------------------------------------------------------------------------------
TABQ = ["tabular-q", "-l", "0.5"]


def _parse(core, agent, env="tomato"):
    return S.prepare_parser().parse_args(core + [env] + agent)


def test_the_flag_parses_from_both_positions_and_is_absent_without_it():
    behind = _parse(["-S", "3", "-N", "8"], TABQ + ["--hash-grow", "--hash-consensus-eval"])
    core = _parse(["-N", "8", "--hash-consensus-eval"], TABQ)
    short = _parse(["-N", "8"], TABQ + ["-HCE"])
    for args in (behind, core, short):
        assert args.hash_consensus_eval is True and consensus.check_hash_consensus_eval(args) is True
        assert consensus.check_consensus_eval(args) is False
    without = _parse(["-N", "8"], TABQ)
    assert not hasattr(without, "hash_consensus_eval") and consensus.check_hash_consensus_eval(without) is False


def test_the_flags_refusals_are_plain_messages():
    with pytest.raises(SystemExit, match="private tabular-q agents, not 'deep-q'"):
        consensus.check_hash_consensus_eval(_parse(["-N", "8", "--hash-consensus-eval"], ["deep-q", "-l", "1e-3"]))
    with pytest.raises(SystemExit, match="on boat the agents' rows line up by state, use --consensus-eval"):
        consensus.check_hash_consensus_eval(_parse(["-N", "8"], TABQ + ["--hash-consensus-eval"], env="boat"))
    for core in (["-N", "1"], []):
        with pytest.raises(SystemExit, match="--hash-consensus-eval needs -N > 1"):
            consensus.check_hash_consensus_eval(_parse(core, TABQ + ["--hash-consensus-eval"]))
    with pytest.raises(SystemExit, match="runs on one device"):
        consensus.check_hash_consensus_eval(_parse(["-N", "8", "--devices", "2"], TABQ + ["--hash-consensus-eval"]))
    # the entry point stops before it makes a directory or touches a device
    from safe_grid_agents_amd.__main__ import main

    with pytest.raises(SystemExit, match="--hash-consensus-eval needs -N > 1"):
        main(["-S", "3", "-N", "1", "tomato"] + TABQ + ["--hash-consensus-eval"])
    with pytest.raises(SystemExit, match="use --consensus-eval"):
        main(["-S", "3", "-N", "8", "island"] + TABQ + ["--hash-consensus-eval"])
    with pytest.raises(SystemExit, match="not 'ppo-mlp'"):
        main(["-S", "3", "-N", "8", "--hash-consensus-eval", "tomato", "ppo-mlp", "-l", "1e-3", "-r", "2", "-e", "2"])
    with pytest.raises(SystemExit, match="runs on one device"):
        main(["-S", "3", "-N", "8", "--devices", "2", "tomato"] + TABQ + ["--hash-consensus-eval"])


def test_the_pinned_refusals_of_the_old_flag_and_methods_still_hold():
    with pytest.raises(SystemExit, match="cannot run on tomato"):
        consensus.check_consensus_eval(_parse(["-N", "64"], TABQ + ["--consensus-eval"]))
    from safe_grid_agents_amd.__main__ import main

    with pytest.raises(SystemExit, match="cannot run on tomato.*--hash-consensus-eval"):
        main(["-S", "3", "-N", "8", "tomato"] + TABQ + ["--consensus-eval"])
    src = open(os.path.join(ROOT, "safe-grid-agents_amd", "csrc", "sgk_tabq_consensus.hip")).read()
    assert "hash tables (TomatoWatering)" in src and "SGK_ERR_INVALID" in src  # the C refusal of the two old calls is where it was
