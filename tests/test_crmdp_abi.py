"""ppo-crmdp's C-ABI (include/sgk.h: sgk_crmdp_keys, sgk_crmdp_filter, sgk_crmdp_filter_host; sgk_crmdp_metric, sgk_crmdp_buffers) as far
as a box without a GPU can tell: the symbols are declared, exported and bound with the header's signatures and the ABI version stays;
every pointer the library writes through travels in sgk_crmdp_buffers, passed by const pointer, and every field of it names a guard-band
test of tests/test_gpu_crmdp.py; the Python wrappers refuse a wrong tensor before it reaches the library. (The refusals of the calls
themselves: tests/test_crmdp_cpu.py.)"""
import ctypes
import importlib
import os
import re

import pytest
import torch

from safe_grid_agents_amd import _lib, crmdp
from safe_grid_agents_amd.envs import BatchedGridworldEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
GUARD_TEST = ("test_gpu_crmdp.test_the_buffers_stay_inside_their_guard_bands",)
# Every pointer of sgk_crmdp_buffers -> the guard-band tests of tests/test_gpu_crmdp.py that carve it from a guard_arena.Arena. (The
# descriptor is passed by const pointer, so tests/test_guard_arena_cpu.py's parser does not see its fields; this table is that file's
# COVERED for them.)
BUFFERS_COVERED = {"sgk_crmdp_buffers.%s" % k: GUARD_TEST for k in ("keys", "rewards_out", "order", "n_corrupt", "safe_index", "unbounded",
                                                                     "mem_flag", "mem_reward", "mem_rllb")}


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sgk.h")).read(), flags=re.S)


def _declared(name):
    m = re.search(r"SGK_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "include/sgk.h does not declare int %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _struct_fields(name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S)
    assert m, "include/sgk.h does not define %s" % name
    out = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            out.append((decl, re.match(r".*?(\w+)$", decl).group(1)))
    return out


def test_the_symbols_are_declared_exported_and_bound():
    assert _declared("sgk_crmdp_keys") == ["sgk_env *h", "const int8_t *states_dev", "const int8_t *last_boards_dev", "int32_t n_steps",
                                           "int64_t n_envs", "int32_t n_cells", "int32_t agent_value", "const sgk_crmdp_buffers *buffers"]
    tail = ["const int32_t *lengths_dev", "int64_t n_trajectories", "int32_t t_max", "int32_t n_agents", "const sgk_crmdp_metric *metric",
            "const sgk_crmdp_buffers *buffers"]
    assert _declared("sgk_crmdp_filter") == ["sgk_env *h", "const int32_t *keys_dev", "const float *rewards_dev"] + tail
    assert _declared("sgk_crmdp_filter_host") == ["const int32_t *keys", "const float *rewards", "const int32_t *lengths"] + tail[1:]
    assert _struct_fields("sgk_crmdp_metric") == [("int32_t kind, width, n_cells", "n_cells")]
    assert [k for k, _ in _lib.SgkCrmdpMetric._fields_] == ["kind", "width", "n_cells"] and ctypes.sizeof(_lib.SgkCrmdpMetric) == 12
    fields = [name for _, name in _struct_fields("sgk_crmdp_buffers")]
    assert fields == [k for k, _ in _lib.SgkCrmdpBuffers._fields_] and len(fields) == 9
    assert ctypes.sizeof(_lib.SgkCrmdpBuffers) == 9 * ctypes.sizeof(ctypes.c_void_p)
    M, B = ctypes.POINTER(_lib.SgkCrmdpMetric), ctypes.POINTER(_lib.SgkCrmdpBuffers)
    want = {"sgk_crmdp_keys": (ctypes.c_int, [V, V, V, I32, I64, I32, I32, B]),
            "sgk_crmdp_filter": (ctypes.c_int, [V, V, V, V, I64, I32, I32, M, B]),
            "sgk_crmdp_filter_host": (ctypes.c_int, [V, V, V, I64, I32, I32, M, B])}
    lib = _lib.load()  # (resolves every bound symbol in libsgk.so: a missing export is an AttributeError here)
    for name, sig in want.items():
        assert name in _lib.EXPORTED_SYMBOLS and _lib._SIGNATURES[name] == sig
        assert getattr(lib, name).argtypes == sig[1] and getattr(lib, name).restype is sig[0]
    assert lib.sgk_abi_version() == 4  # added symbols: the ABI version stays
    raw = open(os.path.join(ROOT, "include", "sgk.h")).read()
    for name, value in (("SGK_CRMDP_T_MAX", _lib.CRMDP_T_MAX), ("SGK_CRMDP_MAX_KEYS", _lib.CRMDP_MAX_KEYS),
                        ("SGK_CRMDP_METRIC_TRANS_BOAT", _lib.CRMDP_METRIC_TRANS_BOAT), ("SGK_CRMDP_UNKNOWN", _lib.CRMDP_UNKNOWN),
                        ("SGK_CRMDP_SAFE", _lib.CRMDP_SAFE), ("SGK_CRMDP_CORRUPT", _lib.CRMDP_CORRUPT)):
        assert re.search(r"#define %s %d\b" % (name, value), raw), name
    assert "#define SGK_CRMDP_NONE (-2147483647 - 1)" in raw and _lib.CRMDP_NONE == -2 ** 31
    flat = " ".join(raw.split())
    assert "travels in sgk_crmdp_buffers" in flat and "test_guard_arena_cpu.py" in flat  # the header says why a descriptor


def test_every_field_of_the_descriptor_names_a_guard_band_test():
    """tests/test_guard_arena_cpu.py's rule for the pointers its parser cannot see: each field of sgk_crmdp_buffers is a non-const
    pointer the library writes through, and each names an existing test of the GPU file that carves it from an arena."""
    fields = _struct_fields("sgk_crmdp_buffers")
    for decl, _ in fields:
        assert "*" in decl and "const" not in decl.split("*")[0].split(), decl
    found = {"sgk_crmdp_buffers.%s" % name for _, name in fields}
    assert found == set(BUFFERS_COVERED), (sorted(found - set(BUFFERS_COVERED)), sorted(set(BUFFERS_COVERED) - found))
    for key, tests in BUFFERS_COVERED.items():
        assert tests, key
        for t in tests:
            module, _, name = t.rpartition(".")
            owner = importlib.import_module(module)
            assert callable(getattr(owner, name, None)) and name.startswith("test_"), (key, t)
            src = open(owner.__file__).read()
            assert "guard_arena" in src and '"%s"' % key.split(".")[1] in src, (key, t)
    # the three calls take no non-const pointer but the handle: the header-wide tables have nothing new to list
    for fn in ("sgk_crmdp_keys", "sgk_crmdp_filter", "sgk_crmdp_filter_host"):
        for p in _declared(fn):
            assert "*" not in p or p.startswith("const ") or p == "sgk_env *h", (fn, p)


class _OnDevice0(torch.Tensor):
    """A host tensor that reports cuda:0 as its device: the wrappers' checks raise before any pointer is taken."""
    device = property(lambda self: torch.device("cuda", 0))


def _dev(t):
    return t.as_subclass(_OnDevice0)


def test_the_wrappers_refuse_a_wrong_tensor_with_a_value_error():
    env = object.__new__(BatchedGridworldEnv)
    env.device, env.n_envs, env.n_cells = 0, 6, 25
    n, T = 6, 9
    states, last = _dev(torch.zeros((T, n, 25), dtype=torch.int8)), _dev(torch.zeros((n, 25), dtype=torch.int8))
    keys, rewards = _dev(torch.zeros((n, T), dtype=torch.int32)), _dev(torch.zeros((n, T), dtype=torch.float32))
    for kwargs, message in ((dict(states=torch.zeros((T, n, 25), dtype=torch.int8)), "states lives on cpu"), (dict(last_boards=_dev(torch.zeros((n, 24), dtype=torch.int8))), "last_boards has shape"),
                            (dict(out=_dev(torch.zeros((n, T), dtype=torch.int64))), "out has dtype"), (dict(out=_dev(torch.zeros((T, n), dtype=torch.int32))), "out has shape")):
        a = dict(states=states, last_boards=last, out=keys)
        a.update(kwargs)
        with pytest.raises(ValueError, match=message):
            crmdp.crmdp_keys(env, a["states"], a["last_boards"], a["out"])
    memory = crmdp.CRMDPMemory(2, _lib.SgkCrmdpMetric(1, 5, 25))
    out = {k: _dev(v) for k, v in crmdp.filter_outputs(n, T, "cpu").items()}
    for bad_out, bad_rewards, message in (({"n_corrupt": _dev(torch.zeros(n + 1, dtype=torch.int32))}, rewards, "n_corrupt has shape"),
                                          ({"rewards_out": _dev(torch.zeros((n, T), dtype=torch.float64))}, rewards, "rewards_out has dtype"),
                                          ({}, _dev(torch.zeros((n, T + 1), dtype=torch.float32)), "rewards has shape"),
                                          ({}, rewards, "mem_flag lives on cpu")):
        with pytest.raises(ValueError, match=message):
            crmdp.crmdp_filter(env, keys, bad_rewards, None, memory, {**out, **bad_out})
    with pytest.raises(ValueError):
        crmdp.CRMDPMemory(1, _lib.SgkCrmdpMetric(1, 5, 65))
    with pytest.raises(KeyError):
        crmdp.metric_for("boat", 5, 5)
    m = crmdp.metric_for("trans-boat", 5, 5)
    assert (m.kind, m.width, m.n_cells) == (1, 5, 25)
    assert memory.states(1) == {} and memory.rllb(0) == {} and memory.n_corrupt() == 0
    memory.flag[1, 27], memory.reward[1, 27], memory.bound[1, 27] = _lib.CRMDP_CORRUPT, -3, -5
    memory.flag[1, 2], memory.reward[1, 2] = _lib.CRMDP_SAFE, 1
    assert memory.states(1) == {(1, 2): (False, -3), (0, 2): (True, 1)} and memory.rllb(1) == {(1, 2): -5} and memory.rllb(0) == {}
