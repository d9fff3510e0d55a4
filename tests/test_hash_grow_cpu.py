"""Growing the hashed Q-tables of TomatoWatering, as far as a box without a GPU can tell.

1. The inputs of tests/test_gpu_hash_grow.py. The growth plans (tests/hash_grow_plans.py) must provide, on the dictionary alone, the
   situations the GPU tests are about -- tables grown while below capacity, exactly full, and after refusals; a second overflow; a
   run that never refuses and equals one that started large -- so that those tests cannot pass on inputs that never exercise growth.
2. The rehash itself. sgk_tabq_hash_grow's loop (csrc/sgk_tabq_hash.h: tabq_rehash_agent) compiled for the host, on tables built by
   inserting the dictionary's boards through the host build of hash_slot: key sets, rows by key as float64 bits, empty slots,
   reachability of every key from its home slot at the new capacity, determinism, the tag words."""
import ctypes

import numpy as np
import pytest

import hash_grow_plans as G
import hashed_tabq_reference as HR
import hostlib

EMPTY = G.EMPTY


# ---- 1. the plans ------------------------------------------------------------------------------------
@pytest.mark.parametrize("claim", [True, False])
def test_plan_a_grows_full_and_overflowed_tables_and_then_has_room(claim):
    leg1, leg2 = G.run_plan(G.PLANS["A"], claim)
    below, full, over = leg1.classes()
    assert (len(below), len(full), len(over)) == (184, 16, 122)
    assert sum(leg1.refused_in_leg) == 2559 and all(leg1.agents[i].refused == 0 for i in full)
    assert leg2.fullest() == 115 and leg2.capacity == 128 and not any(leg2.refused_in_leg)
    assert HR.hash_info(leg2.agents) == (128, 115, True)  # the flag is sticky: leg 1 raised it


@pytest.mark.parametrize("claim", [True, False])
def test_plan_b_overflows_again_behind_the_growth(claim):
    _, leg2 = G.run_plan(G.PLANS["B"], claim)
    below, full, over = leg2.classes()
    assert (len(below), len(full), len(over)) == (114, 3, 205)


@pytest.mark.parametrize("claim", [True, False])
def test_plan_c_never_refuses(claim):
    legs = G.run_plan(G.PLANS["C"], claim)
    assert [l.fullest() for l in legs] == [43, 81, 148]
    assert not any(any(l.refused_in_leg) for l in legs) and not any(a.overflowed for a in legs[-1].agents)


@pytest.mark.parametrize("claim", [True, False])
def test_plan_d_equals_a_run_that_started_large(claim):
    legs = G.run_plan(G.PLANS["D"], claim)
    assert not any(any(l.refused_in_leg) for l in legs)
    _, roomy, acts = HR.run(256, 150, claim_start_on_reset=claim)
    assert np.concatenate([l.acts for l in legs]).tobytes() == acts.tobytes()
    for a, b in zip(legs[-1].agents, roomy):
        assert list(a.rows.items()) == list(b.rows.items()) and not a.overflowed and not b.overflowed
    assert legs[-1].fullest() == 117 and sum(a.n_rows > 64 for a in legs[-1].agents) == 319


def test_the_two_boundary_orders_give_the_same_tables_on_these_plans():
    for name, legs in G.PLANS.items():
        for a, b in zip(G.run_plan(legs, True), G.run_plan(legs, False)):
            assert a.acts.tobytes() == b.acts.tobytes(), name
            assert all(x.rows == y.rows and x.refused == y.refused for x, y in zip(a.agents, b.agents)), name


# ---- 2. the host rehash -------------------------------------------------------------------------------
def _host():
    L = hostlib.load()
    V = ctypes.c_void_p
    L.sgk_debug_tabq_hash_slot.argtypes = [V, ctypes.c_int32, ctypes.c_uint32, V]
    L.sgk_debug_tabq_rehash.argtypes = [V, V, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, V, V, V, V]
    return L


def _home(key, cap):
    return (((key * 0x9E3779B1) & 0xFFFFFFFF) >> 8) & (cap - 1)


_BUILT = {}


def _tables_at_64():
    """(keys uint32 [N, 64], table float64 [N, 64, 4], [{key: row bits}]) of plan A's first leg: every board of every dictionary,
    in admission order, through the host build of hash_slot -- 184 tables with room, 138 with all 64 slots claimed."""
    if not _BUILT:
        L, R = _host(), G.rules()
        agents = G.run_plan(G.PLANS["A"], True)[0].agents
        keys = np.full((HR.N, 64), EMPTY, dtype=np.uint32)
        table = np.zeros((HR.N, 64, 4), dtype=np.float64)
        by_key = []
        ov = ctypes.c_int32(0)
        for i, a in enumerate(agents):
            rows = {}
            for board, row in a.rows.items():
                key = G.board_key(R, board)
                slot = L.sgk_debug_tabq_hash_slot(keys[i].ctypes.data, 64, key, ctypes.byref(ov))
                assert 0 <= slot < 64 and keys[i, slot] == key and key not in rows
                table[i, slot] = row
                rows[key] = np.array(row, dtype=np.float64).view(np.uint64).tolist()
            by_key.append(rows)
        assert ov.value == 0
        assert sum(len(r) == 64 for r in by_key) == 138 and any(any(any(v) for v in r.values()) for r in by_key)
        _BUILT["t"] = (keys, table, by_key)
    return _BUILT["t"]


def _rehash(keys, table, cap_new, tags=None):
    L = _host()
    n, cap_old = keys.shape
    keys_new = np.full((n, cap_new), 0x12345678, dtype=np.uint32)  # (garbage: the call makes them empty / zero itself)
    table_new = np.full((n, cap_new, 4), 7.0, dtype=np.float64)
    ov = ctypes.c_int32(0)
    rc = L.sgk_debug_tabq_rehash(keys.ctypes.data, table.ctypes.data, n, cap_old, cap_new, keys_new.ctypes.data, table_new.ctypes.data,
                                 None if tags is None else tags.ctypes.data, ctypes.byref(ov))
    assert rc == 0 and ov.value == 0
    return keys_new, table_new


@pytest.mark.parametrize("cap_new", [128, 256])
def test_rehash_keeps_every_row_by_key_and_every_key_reachable(cap_new):
    keys, table, by_key = _tables_at_64()
    keys0, table0 = keys.copy(), table.copy()
    keys_new, table_new = _rehash(keys, table, cap_new)
    assert keys.tobytes() == keys0.tobytes() and table.tobytes() == table0.tobytes()  # the old arrays are only read
    bits = table_new.view(np.uint64)
    for i, rows in enumerate(by_key):
        occ = np.nonzero(keys_new[i] != EMPTY)[0]
        held = [int(k) for k in keys_new[i, occ]]
        assert len(held) == len(set(held)) and set(held) == set(rows), i
        for k, s in zip(held, occ):
            assert bits[i, s].tolist() == rows[k], (i, hex(k))
            j = _home(k, cap_new)  # a lookup at the new capacity finds the key before it meets an empty slot
            while keys_new[i, j] != k:
                assert keys_new[i, j] != EMPTY, (i, hex(k), "unreachable from its home slot")
                j = (j + 1) & (cap_new - 1)
            assert j == s
        assert not bits[i][keys_new[i] == EMPTY].any(), (i, "an unclaimed slot's row is not all zero")
    again = _rehash(keys, table, cap_new)
    assert again[0].tobytes() == keys_new.tobytes() and again[1].tobytes() == table_new.tobytes()  # two runs: equal bytes


def test_rehash_to_the_same_capacity_is_the_identity():
    keys, table, _ = _tables_at_64()
    keys_new, table_new = _rehash(keys, table, 64)
    assert keys_new.tobytes() == keys.tobytes() and table_new.tobytes() == table.tobytes()


def test_the_pending_slot_of_a_tag_follows_its_board_and_the_kept_row_is_dropped():
    keys, table, by_key = _tables_at_64()
    rng = np.random.RandomState(5)
    tags = np.empty(HR.N, dtype=np.uint64)
    want = []
    for i in range(HR.N):
        occ = np.nonzero(keys[i] != EMPTY)[0]
        low = EMPTY if i % 5 == 0 else int(occ[rng.randint(len(occ))])
        high = EMPTY if i % 3 == 0 else int(occ[rng.randint(len(occ))])
        tags[i] = low | (high << 32)
        want.append(None if low == EMPTY else int(keys[i, low]))
    keys_new, _ = _rehash(keys, table, 256, tags)
    for i, key in enumerate(want):
        low, high = int(tags[i]) & 0xFFFFFFFF, int(tags[i]) >> 32
        assert high == EMPTY, i
        assert (low == EMPTY) if key is None else (keys_new[i, low] == key), i


def test_arguments_that_cannot_be_right_are_refused():
    L = _host()
    keys, table, _ = _tables_at_64()
    out_k, out_t = np.zeros((HR.N, 128), dtype=np.uint32), np.zeros((HR.N, 128, 4))
    ov = ctypes.c_int32(0)
    for cap_old, cap_new in [(64, 32), (64, 96), (48, 128)]:
        assert L.sgk_debug_tabq_rehash(keys.ctypes.data, table.ctypes.data, HR.N, cap_old, cap_new, out_k.ctypes.data, out_t.ctypes.data,
                                       None, ctypes.byref(ov)) == hostlib.ERR_INVALID
    assert not out_k.any() and not out_t.any()
