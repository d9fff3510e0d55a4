"""The hashed levels' consensus (include/sgk.h: sgk_tabq_hash_consensus, sgk_tabq_hash_load_shared) restated on Python dictionaries --
helper of test_hash_consensus_cpu.py and test_gpu_hash_consensus.py. CPU only. It never evaluates the product's hash function: a
table here is {key: row}.

vote():  agents = one {key: [4 floats]} per agent. Agent e votes on key k iff it may, it holds k, and its row of k has an entry != 0.0
         (-0.0 is zero); its vote is the first maximum. -> {key: [4 counts]} of the keys with at least one voter.
load():  the dictionary a sequential insertion leaves: later duplicates overwrite, at most `capacity` distinct keys are admitted.
host_vote() / host_load() call the library's host restatements of both on numpy arrays (garbage-filled outputs first)."""
import ctypes

import numpy as np

EMPTY = 0xFFFFFFFF


def vote(agents, mask=None):
    out = {}
    for e, rows in enumerate(agents):
        if mask is not None and not mask[e]:
            continue
        for key, row in rows.items():
            if any(float(q) != 0.0 for q in row):
                best = 0
                for a in range(1, 4):
                    if row[a] > row[best]:
                        best = a
                out.setdefault(int(key), [0, 0, 0, 0])[best] += 1
    return out


def arrays(votes, max_keys):
    """(keys uint32 [max_keys], votes int64 [max_keys, 4], voters int64 [max_keys], U) as the C ABI writes a vote: ascending keys, the
    first max_keys of them, 0xffffffff / 0 behind the last."""
    keys, counts = np.full(max_keys, EMPTY, dtype=np.uint32), np.zeros((max_keys, 4), dtype=np.int64)
    for j, k in enumerate(sorted(votes)[:max_keys]):
        keys[j], counts[j] = k, votes[k]
    return keys, counts, counts.sum(axis=1), len(votes)


def load(keys, rows, capacity):
    """-> ({key: row}, dropped keys in order): the first `capacity` distinct keys are admitted, a key seen again takes the later row."""
    table, dropped = {}, []
    for k, row in zip(keys, rows):
        k = int(k)
        if k == EMPTY:
            continue
        if k not in table and len(table) >= capacity:
            dropped.append(k)
            continue
        table[k] = [float(q) for q in row]
    return table, dropped


def policy(counts):
    """The first action with the most votes, per row of an int64 [U, 4]."""
    return np.argmax(np.asarray(counts), axis=1).astype(np.uint8)


def tables_as_dicts(keys, rows):
    """[agent][slot] arrays (sgk_tabq_copy_keys / sgk_tabq_copy_table) -> one {key: row} per agent."""
    out = []
    for kr, rr in zip(np.asarray(keys), np.asarray(rows)):
        out.append({int(k): [float(q) for q in r] for k, r in zip(kr, rr) if int(k) != EMPTY})
    return out


# ---- the C ABI's host calls, for both test files ------------------------------------------------------------------------------------------
def host_vote(keys, rows, mask=None, max_keys=None, with_voters=True, expect=0):
    """sgk_tabq_hash_consensus_host on [A, cap] keys and [A, cap, 4] rows -> (keys, votes, voters, U). The outputs start out as garbage:
    the call overwrites every element. max_keys defaults to A * cap (at least 1)."""
    from safe_grid_agents_amd import _lib

    k = np.ascontiguousarray(keys, dtype=np.uint32)
    r = np.ascontiguousarray(rows, dtype=np.float64)
    A, cap = k.shape
    assert r.shape == (A, cap, 4)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    K = max(A * cap, 1) if max_keys is None else int(max_keys)
    out_keys, votes = np.full(K, 0x12345678, dtype=np.uint32), np.full((K, 4), -77, dtype=np.int64)
    voters, count = np.full(K, -55, dtype=np.int64), np.full(1, -33, dtype=np.int64)
    desc = _lib.SgkTabqHashVotes(out_keys.ctypes.data, votes.ctypes.data, voters.ctypes.data if with_voters else None, count.ctypes.data, K,
                                 None, 0)
    rc = _lib.load().sgk_tabq_hash_consensus_host(k.ctypes.data, r.ctypes.data, A, cap, None if m is None else m.ctypes.data, ctypes.byref(desc))
    assert rc == expect, _lib.load().sgk_last_error()
    return out_keys, votes, voters, int(count[0])


def host_load(keys, rows, capacity, count=None):
    """sgk_tabq_hash_load_shared_host -> (keys uint32 [capacity], rows float64 [capacity, 4], overflowed); garbage first, as above."""
    from safe_grid_agents_amd import _lib

    k = np.ascontiguousarray(keys, dtype=np.uint32)
    r = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 4)
    n = len(k) if count is None else int(count)
    out_keys, out_rows, over = np.full(capacity, 0x12345678, dtype=np.uint32), np.full((capacity, 4), -7.5), np.full(1, -3, dtype=np.int32)
    desc = _lib.SgkTabqHashTable(out_keys.ctypes.data, out_rows.ctypes.data, over.ctypes.data)
    rc = _lib.load().sgk_tabq_hash_load_shared_host(k.ctypes.data, r.ctypes.data, n, capacity, ctypes.byref(desc))
    assert rc == 0, _lib.load().sgk_last_error()
    return out_keys, out_rows, int(over[0])


def table_as_dict(keys, rows):
    return tables_as_dicts([keys], [rows])[0]
