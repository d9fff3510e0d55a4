"""sgk_policy_rollout_members / sgk_ppo_epochs_members (include/sgk.h) -- a population of independent PPO-MLP agents gathered and
trained in one launch each -- as far as a box without a GPU can tell: the symbols are declared, exported by libsgk.so and bound with
the header's signatures; the ABI version stays; the population's default member seeds are distinct, deterministic and the documented
function; stacking member state dicts on the member axis and taking them apart again loses no bit (pure torch on CPU tensors)."""
import ctypes
import inspect
import os
import re

import numpy as np
import torch

from safe_grid_agents_amd import _lib, ppo_population as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(name):
    text = open(os.path.join(ROOT, "include", "sgk.h")).read()
    m = re.search(r"SGK_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "include/sgk.h does not declare %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_symbols_are_declared_exported_and_bound():
    V, I32, U64, U32, F64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double
    assert _declared("sgk_policy_rollout_members") == [
        "sgk_env *h", "const sgk_mlp_weights *w", "int32_t n_members", "int32_t mode", "double epsilon", "uint64_t draw_index0",
        "int32_t n_steps", "uint32_t flags", "int8_t *states_out_dev", "uint8_t *actions_out_dev", "sgk_step_rec *recs_out_dev",
        "int64_t *member_metrics_dev"]
    assert _declared("sgk_ppo_epochs_members") == ["sgk_env *h", "const sgk_ppo_learner *learner", "int32_t n_members",
                                                   "const uint64_t *member_keys_dev"]
    want = {"sgk_policy_rollout_members": [V, ctypes.POINTER(_lib.SgkMlpWeights), I32, I32, F64, U64, I32, U32, V, V, V, V],
            "sgk_ppo_epochs_members": [V, ctypes.POINTER(_lib.SgkPpoLearner), I32, V]}
    lib = _lib.load()  # (resolves every bound symbol in libsgk.so: a missing export is an AttributeError here)
    for name, args in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        res, bound = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and bound == args, name
        assert getattr(lib, name).argtypes == args
    assert lib.sgk_abi_version() == 4  # added symbols: the ABI version stays


def test_a_null_handle_is_refused_with_a_message():
    lib = _lib.load()
    w, L = _lib.SgkMlpWeights(), _lib.SgkPpoLearner()
    for rc in (lib.sgk_policy_rollout_members(None, ctypes.byref(w), 3, 1, 0.0, 0, 5, 0, None, None, None, None),
               lib.sgk_ppo_epochs_members(None, ctypes.byref(L), 3, None)):
        assert rc == _lib.ERR_INVALID
        assert b"NULL" in lib.sgk_last_error()


def test_default_member_seeds_are_distinct_deterministic_and_documented():
    seeds = [PP.default_member_seed(7, m) for m in range(4096)]
    assert len(set(seeds)) == len(seeds)
    assert all(0 <= s < 2 ** 64 for s in seeds)
    assert seeds == [PP.default_member_seed(7, m) for m in range(4096)]
    assert set(seeds).isdisjoint(PP.default_member_seed(8, m) for m in range(4096))

    def documented(seed, m):  # the function as default_member_seed's docstring states it
        mask = 2 ** 64 - 1
        z = (seed + (m + 1) * 0x9E3779B97F4A7C15) & mask
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        return z ^ (z >> 31)

    doc = inspect.getdoc(PP.default_member_seed)
    for constant in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", ">> 30", ">> 27", ">> 31"):
        assert constant in doc, constant
    for seed, m in ((0, 0), (7, 3), (499, 1023), (2 ** 63 + 5, 2)):
        assert PP.default_member_seed(seed, m) == documented(seed, m)
    assert PP.default_member_seed(0, 0) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0
    torch.manual_seed(max(seeds))  # every seed is one torch accepts


def _state_dict(rng, k0, h, with_old):
    shapes = {"network.0.0.weight": (h, k0), "network.0.0.bias": (h,), "network.1.0.0.weight": (h, h), "network.1.0.0.bias": (h,),
              "actor.weight": (4, h), "actor.bias": (4,), "critic.weight": (1, h), "critic.bias": (1,)}
    assert tuple(shapes) == PP.MEMBER_KEYS
    # raw bit patterns, denormals, infinities and NaN payloads included: a round trip must not touch them
    sd = {k: torch.from_numpy(rng.integers(0, 2 ** 32, s, dtype=np.uint32).view(np.float32).copy()) for k, s in shapes.items()}
    if with_old:
        sd.update({"old_policy." + k: torch.zeros(s) for k, s in shapes.items()})
    return sd


def test_stacking_and_unstacking_member_state_dicts_round_trips_bit_for_bit():
    rng = np.random.default_rng(11)
    for k0, h, members in ((25, 64, 3), (63, 100, 5), (36, 100, 1)):
        dicts = [_state_dict(rng, k0, h, with_old=m % 2 == 0) for m in range(members)]
        stacked = PP.stack_state_dicts(dicts)
        assert tuple(stacked) == PP.PARAMS
        for key, name in zip(PP.MEMBER_KEYS, PP.PARAMS):
            assert tuple(stacked[name].shape) == (members,) + tuple(dicts[0][key].shape)
            assert stacked[name].is_contiguous() and stacked[name].dtype == torch.float32
        for m in range(members):
            back = PP.unstack_state_dict(stacked, m)
            assert tuple(back) == PP.MEMBER_KEYS
            for key in PP.MEMBER_KEYS:
                assert back[key].numpy().tobytes() == dicts[m][key].numpy().tobytes(), (m, key)
                assert back[key].data_ptr() != stacked[PP.PARAMS[PP.MEMBER_KEYS.index(key)]][m].data_ptr()  # a copy
        again = PP.stack_state_dicts([PP.unstack_state_dict(stacked, m) for m in range(members)])
        for name in PP.PARAMS:
            assert again[name].numpy().tobytes() == stacked[name].numpy().tobytes()
