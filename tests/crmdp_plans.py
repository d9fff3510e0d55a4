"""What the CRMDP tests share: the reference's recorded plans (tests/golden/crmdp_plans.npz, tests/golden/make_golden_crmdp.py), the
dictionary restatement run over them once, and sgk_crmdp_filter_host on numpy arrays."""
import ctypes
import functools
import os

import numpy as np

import crmdp_reference as R
from safe_grid_agents_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUTPUTS = ("rewards_out", "order", "n_corrupt", "safe_index", "unbounded")
TABLES = ("mem_flag", "mem_reward", "mem_rllb")


@functools.lru_cache(maxsize=None)
def plans():
    with np.load(os.path.join(GOLDEN, "crmdp_plans.npz")) as z:
        g = {k: z[k] for k in z.files}
    for v in g.values():
        v.setflags(write=False)
    return g


def metric(width=5, n_cells=25, kind=_lib.CRMDP_METRIC_TRANS_BOAT):
    return _lib.SgkCrmdpMetric(kind, width, n_cells)


def fresh_tables(n_agents, n_keys=625):
    return {"mem_flag": np.zeros((n_agents, n_keys), np.uint8), "mem_reward": np.zeros((n_agents, n_keys), np.int32),
            "mem_rllb": np.full((n_agents, n_keys), R.NONE, np.int32)}


def fresh_outputs(n, t_max, fill=0):
    return {"rewards_out": np.full((n, t_max), fill, np.float32), "order": np.full((n, t_max), fill, np.int32),
            "n_corrupt": np.full(n, fill, np.int32), "safe_index": np.full(n, fill, np.int32), "unbounded": np.full(n, fill, np.int32)}


def buffers(arrays):
    """SgkCrmdpBuffers over numpy arrays (by name; a missing name is a NULL pointer)."""
    return _lib.SgkCrmdpBuffers(**{k: (arrays[k].ctypes.data if arrays.get(k) is not None else None)
                                   for k, _ in _lib.SgkCrmdpBuffers._fields_})


def filter_host(keys, rewards, lengths, n_agents, tables, m=None, check=True):
    """sgk_crmdp_filter_host -> its five outputs; `tables` (fresh_tables) are updated in place."""
    keys, rewards = np.ascontiguousarray(keys, np.int32), np.ascontiguousarray(rewards, np.float32)
    lengths = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
    n, t_max = keys.shape
    out = fresh_outputs(n, t_max, fill=-7)
    m = m or metric()
    rc = _lib.load().sgk_crmdp_filter_host(keys.ctypes.data, rewards.ctypes.data, None if lengths is None else lengths.ctypes.data, n, t_max,
                                           n_agents, ctypes.byref(m), ctypes.byref(buffers({**out, **tables})))
    if check:
        _lib.check(rc)
    return out


@functools.lru_cache(maxsize=None)
def restated():
    """The dictionary restatement over the plans, computed once: per trajectory the order list, n_corrupt, the safe index, the
    modified rewards (float32 [t_max], the input kept where there is no bound), the unbounded count and the tables afterwards."""
    g = plans()
    n, t_max = g["keys"].shape
    per_agent = n // int(g["n_agents"])
    out = fresh_outputs(n, t_max, fill=0)
    out["order"][:] = -1
    out["none"] = np.zeros((n, t_max), bool)
    tables = {k: np.zeros((n, 625), np.uint8 if k == "mem_flag" else np.int32) for k in TABLES}
    mem = None
    for i in range(n):
        if i % per_agent == 0:
            mem = R.Memory(int(g["width"]), int(g["n_cells"]))
        L = int(g["lengths"][i])
        order, safe, modified = mem.filter(g["keys"][i, :L], g["rewards"][i, :L])
        out["order"][i, :len(order)] = order
        out["n_corrupt"][i], out["safe_index"][i] = len(order), (-1 if safe is None else safe)
        out["rewards_out"][i] = g["rewards"][i]
        for t, v in enumerate(modified):
            if v is None:
                out["none"][i, t] = True
            else:
                out["rewards_out"][i, t] = v
        out["unbounded"][i] = int(out["none"][i].sum())
        tables["mem_flag"][i], tables["mem_reward"][i], tables["mem_rllb"][i] = mem.tables()
    for v in list(out.values()) + list(tables.values()):
        v.setflags(write=False)
    return out, tables
