"""The C-ABI library loads on a CPU-only box and exports exactly what include/sgk.h declares (no compute calls)."""
import os
import re

import pytest

import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "sgk.h")).read()
    return sorted(set(re.findall(r"SGK_API[^;(]*?\b(sgk_\w+)\s*\(", text)))


def test_library_is_built_and_loads():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = _lib.load()
    assert lib.sgk_abi_version() == 4


def test_the_default_library_refuses_the_test_hooks():
    """A process that did not set SGK_ENABLE_TEST_HOOKS=1 before loading libsgk.so gets SGK_ERR_INVALID from every sgk_debug_* entry
    point -- "make the next host allocation fail" and "plant a stale exit word" among them -- and nothing is armed; this test-suite's
    own process (tests/conftest.py sets the variable) gets answers."""
    import subprocess
    import sys

    code = r"""
import ctypes, os, sys
assert "SGK_ENABLE_TEST_HOOKS" not in os.environ
lib = ctypes.CDLL(sys.argv[1])
lib.sgk_last_error.restype = ctypes.c_char_p
lib.sgk_debug_reset_word.restype = ctypes.c_uint64
out5, out4 = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 4)()
dims, templ, agent = (ctypes.c_int32 * 4)(), (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
word, g0, g1 = ctypes.c_uint64(0), ctypes.c_int32(-7), ctypes.c_int32(-7)
assert lib.sgk_debug_host_transition(0, 6, 255, 1, out5) == -1 and b"SGK_ENABLE_TEST_HOOKS" in lib.sgk_last_error()
assert lib.sgk_debug_host_step(0, ctypes.c_uint64(0), 1, 1, ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.byref(word), out4, None) == -1
assert lib.sgk_debug_reset_word(0, ctypes.c_uint64(0), ctypes.c_uint64(0), 1, None) == 2**64 - 1
assert lib.sgk_debug_level(0, dims, templ, agent) == -1
assert lib.sgk_debug_graph_count(None, None, ctypes.byref(g0), ctypes.byref(g1)) == -1 and (g0.value, g1.value) == (-7, -7)
assert lib.sgk_debug_launch_grids(None, dims) == -1 and list(dims) == [0, 0, 0, 0]
assert lib.sgk_debug_server_stale_exit_word(None) == -1 and b"SGK_ENABLE_TEST_HOOKS" in lib.sgk_last_error()
assert lib.sgk_debug_fail_host_alloc(1) == -1   # refused ...
assert lib.sgk_debug_fail_host_alloc(0) == -1   # ... and not armed: the countdown a working hook would hand back is 1, not an error
print("REFUSED")
"""
    env = {k: v for k, v in os.environ.items() if k != "SGK_ENABLE_TEST_HOOKS"}
    r = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "REFUSED" in r.stdout, r.stdout + r.stderr
    lib = _lib.load()  # this process asked for the hooks before the library was loaded
    assert os.environ.get("SGK_ENABLE_TEST_HOOKS") == "1"
    assert lib.sgk_debug_fail_host_alloc(0) == 0


def test_every_declared_symbol_is_exported_and_bound():
    declared = _declared()
    assert len(declared) >= 40
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared


def test_no_gpu_means_loud_failure_not_fallback():
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.SgkError) as ei:
        S.make("BoatRace-v0")
    assert ei.value.code == _lib.ERR_NODEVICE
    with pytest.raises(_lib.SgkError):
        S.BatchedGridworldEnv("IslandNavigation-v0", 16)


def test_unknown_env_is_a_keyerror():
    with pytest.raises(KeyError):
        S.make("TomatoCrmdp-v0")
    with pytest.raises(KeyError):
        S.make("nope")


def test_host_rng_helper_matches_oracle_stream():
    from oracle import oracle as O

    lib = _lib.load()
    for seed, env, t in [(0, 0, 0), (0x5AFE, 7, 63), (0x5AFE, 7, 64), (2**40 + 3, 2**33 + 1, 12345)]:
        assert lib.sgk_random_action(seed, env, t) == O.random_action(seed, env, t)


def test_host_epsilon_helper_matches_oracle():
    from oracle import oracle as O

    lib = _lib.load()
    for eps, anneal in [(0.01, 100000), (0.05, 7), (0.3, 1), (0.0, 50)]:
        for t in (0, 1, 2, 5, 6, 7, 49, 50, 99999, 100000, 10**7):
            assert lib.sgk_tabq_epsilon(eps, anneal, t) == O.epsilon(eps, anneal, t)


def test_rccl_probe_is_side_effect_free_and_answers_on_any_box():
    """sgk_comm_available: loads librccl and resolves the entry points, or says why not -- never a socket or a thread (what the
    ranks other than 0 call before the communicator is made)."""
    import ctypes
    import threading

    lib = _lib.load()
    before = threading.active_count()
    ver = ctypes.c_int32(-1)
    rc = lib.sgk_comm_available(ctypes.byref(ver))
    assert rc in (_lib.SGK_OK, _lib.ERR_NODEVICE)
    if rc == _lib.SGK_OK:
        assert ver.value >= 0
    else:
        assert b"rccl" in lib.sgk_last_error().lower()
    assert threading.active_count() == before
