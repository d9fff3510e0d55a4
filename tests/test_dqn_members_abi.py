"""sgk_dqn_members_workspace_bytes / sgk_dqn_sgd_step_members (include/sgk.h) -- a population of independent Deep-Q agents trained in
one call -- as far as a box without a GPU can tell: the symbols are declared, exported by libsgk.so and bound with the header's
signatures; the ABI version stays; a NULL handle is refused with a message by both; stacking member state dicts on the member axis and
taking them apart again loses no bit (pure torch on CPU tensors); the default member seeds are the PPO population's function, imported."""
import ctypes
import os
import re

import numpy as np
import torch

from safe_grid_agents_amd import _lib, deepq_population as DP, ppo_population as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(name, result):
    text = open(os.path.join(ROOT, "include", "sgk.h")).read()
    m = re.search(r"SGK_API\s+%s\s+%s\s*\(([^)]*)\)\s*;" % (result, name), text)
    assert m, "include/sgk.h does not declare %s %s" % (result, name)
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_symbols_are_declared_exported_and_bound():
    V, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert _declared("sgk_dqn_members_workspace_bytes", "int64_t") == ["sgk_env *h", "int32_t n_hidden", "int32_t n_members"]
    assert _declared("sgk_dqn_sgd_step_members", "int") == ["sgk_env *h", "const sgk_dqn_learner *learner", "int32_t n_members",
                                                            "const uint64_t *member_keys_dev", "void *workspace"]
    want = {"sgk_dqn_members_workspace_bytes": (I64, [V, I32, I32]),
            "sgk_dqn_sgd_step_members": (ctypes.c_int, [V, ctypes.POINTER(_lib.SgkDqnLearner), I32, V, V])}
    lib = _lib.load()  # (resolves every bound symbol in libsgk.so: a missing export is an AttributeError here)
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name] == (res, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert lib.sgk_abi_version() == 4  # added symbols: the ABI version stays


def test_a_null_handle_is_refused_with_a_message():
    lib = _lib.load()
    L = _lib.SgkDqnLearner()
    ws = ctypes.create_string_buffer(64)
    assert lib.sgk_dqn_members_workspace_bytes(None, 100, 3) == -1
    assert b"NULL" in lib.sgk_last_error()
    assert lib.sgk_dqn_sgd_step_members(None, ctypes.byref(L), 3, None, ws) == _lib.ERR_INVALID
    assert b"NULL" in lib.sgk_last_error()


def test_the_default_member_seeds_are_the_ppo_populations():
    assert DP.default_member_seed is PP.default_member_seed


def _state_dict(rng, k0, h):
    shapes = {"0.0.weight": (h, k0), "0.0.bias": (h,), "1.0.0.weight": (h, h), "1.0.0.bias": (h,), "2.weight": (4, h), "2.bias": (4,)}
    assert tuple(shapes) == DP.MEMBER_KEYS
    # raw bit patterns, denormals, infinities and NaN payloads included: a round trip must not touch them
    return {k: torch.from_numpy(rng.integers(0, 2 ** 32, s, dtype=np.uint32).view(np.float32).copy()) for k, s in shapes.items()}


def test_member_keys_are_the_q_networks_own_state_dict_keys():
    from safe_grid_agents_amd.deepq_batched import BatchedDeepQAgent

    class Shell:  # what build_Q reads of an agent
        torch, q_body, action_n = torch, "mlp", 4

    net = BatchedDeepQAgent.build_Q(Shell(), 25, 2, 64)
    assert tuple(net.state_dict()) == DP.MEMBER_KEYS


def test_stacking_and_unstacking_member_state_dicts_round_trips_bit_for_bit():
    rng = np.random.default_rng(12)
    for k0, h, members in ((25, 64, 3), (63, 100, 5), (36, 100, 1)):
        dicts = [_state_dict(rng, k0, h) for m in range(members)]
        stacked = DP.stack_state_dicts(dicts)
        assert tuple(stacked) == DP.PARAMS
        for key, name in zip(DP.MEMBER_KEYS, DP.PARAMS):
            assert tuple(stacked[name].shape) == (members,) + tuple(dicts[0][key].shape)
            assert stacked[name].is_contiguous() and stacked[name].dtype == torch.float32
        for m in range(members):
            back = DP.unstack_state_dict(stacked, m)
            assert tuple(back) == DP.MEMBER_KEYS
            for key in DP.MEMBER_KEYS:
                assert back[key].numpy().tobytes() == dicts[m][key].numpy().tobytes(), (m, key)
                assert back[key].data_ptr() != stacked[DP.PARAMS[DP.MEMBER_KEYS.index(key)]][m].data_ptr()  # a copy
        again = DP.stack_state_dicts([DP.unstack_state_dict(stacked, m) for m in range(members)])
        for name in DP.PARAMS:
            assert again[name].numpy().tobytes() == stacked[name].numpy().tobytes()
