"""Per-member hyper-parameters for the populations (include/sgk.h: sgk_ppo_epochs_members_hyper, sgk_ppo_cnn_epochs_members_hyper,
sgk_dqn_sgd_step_members_hyper, sgk_policy_rollout_members_eps, sgk_discounted_returns_members, sgk_discount_powers) as far as a box
without a GPU can tell: the symbols are declared, exported and bound with the header's signatures and the ABI version stays; a NULL
handle and a NULL per-member pointer are refused with a message; the host table of discount powers is float32(d ** t) and gives the
reference's returns; the `--sweep` grammar (grid order, member -> point, every refusal); the constructors' ValueErrors that are
raised before anything touches a device."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib, member_hyper as MH, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, I32, I64, U64, U32, F64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double


def _header():
    return open(os.path.join(ROOT, "include", "sgk.h")).read()


def _declared(name, result="int"):
    m = re.search(r"SGK_API\s+%s\s+%s\s*\(([^)]*)\)\s*;" % (result, name), _header())
    assert m, "include/sgk.h does not declare %s %s" % (result, name)
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _struct_fields(name):
    m = re.search(r"typedef struct %s \{([^}]*)\} %s;" % (name, name), _header())
    assert m, "include/sgk.h does not define %s" % name
    return " ".join(m.group(1).split())


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    # every new call is its shared-hyper sibling's argument list plus the per-member pointer at the end
    assert _declared("sgk_ppo_epochs_members_hyper") == _declared("sgk_ppo_epochs_members") + ["const sgk_ppo_member_hyper *hyper_dev"]
    assert _declared("sgk_ppo_cnn_epochs_members_hyper") == _declared("sgk_ppo_cnn_epochs_members") + ["const sgk_ppo_member_hyper *hyper_dev"]
    assert _declared("sgk_dqn_sgd_step_members_hyper") == _declared("sgk_dqn_sgd_step_members") + ["const sgk_dqn_member_hyper *hyper_dev"]
    assert _declared("sgk_policy_rollout_members_eps") == _declared("sgk_policy_rollout_members") + ["const double *member_epsilon_dev"]
    assert _declared("sgk_discounted_returns_members") == [
        "sgk_env *h", "const float *rewards_dev", "const int32_t *lengths_dev", "float *returns_dev", "int64_t n_trajectories",
        "int32_t t_max", "int32_t n_members", "const float *gamma_pow_dev"]
    assert _declared("sgk_discount_powers") == ["double discount", "int32_t t_max", "float *out_host"]
    assert _struct_fields("sgk_ppo_member_hyper") == "double lr, clipping, critic_coeff, entropy_bonus;"
    assert _struct_fields("sgk_dqn_member_hyper") == "double lr, discount;"
    # the Python mirrors of the structs: plain doubles in the header's order (a float64 [M, 4] / [M, 2] tensor holds the rows)
    assert _lib.PPO_MEMBER_HYPER_FIELDS == ("lr", "clipping", "critic_coeff", "entropy_bonus") and ctypes.sizeof(_lib.SgkPpoMemberHyper) == 32
    assert _lib.DQN_MEMBER_HYPER_FIELDS == ("lr", "discount") and ctypes.sizeof(_lib.SgkDqnMemberHyper) == 16
    assert MH.PPO_NAMES[:4] == _lib.PPO_MEMBER_HYPER_FIELDS and MH.DQN_NAMES[:2] == _lib.DQN_MEMBER_HYPER_FIELDS
    want = {"sgk_ppo_epochs_members_hyper": (ctypes.c_int, [V, ctypes.POINTER(_lib.SgkPpoLearner), I32, V, V]),
            "sgk_ppo_cnn_epochs_members_hyper": (ctypes.c_int, [V, ctypes.POINTER(_lib.SgkPpoCnnLearner), I32, V, V]),
            "sgk_dqn_sgd_step_members_hyper": (ctypes.c_int, [V, ctypes.POINTER(_lib.SgkDqnLearner), I32, V, V, V]),
            "sgk_policy_rollout_members_eps": (ctypes.c_int, [V, ctypes.POINTER(_lib.SgkMlpWeights), I32, I32, F64, U64, I32, U32, V, V, V, V, V]),
            "sgk_discounted_returns_members": (ctypes.c_int, [V, V, V, V, I64, I32, I32, V]),
            "sgk_discount_powers": (ctypes.c_int, [F64, I32, V])}
    lib = _lib.load()  # (resolves every bound symbol in libsgk.so: a missing export is an AttributeError here)
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name] == (res, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert lib.sgk_abi_version() == 4  # added symbols: the ABI version stays


def test_a_null_handle_and_a_null_per_member_pointer_are_refused_with_a_message():
    lib = _lib.load()
    w, P, C, D = _lib.SgkMlpWeights(), _lib.SgkPpoLearner(), _lib.SgkPpoCnnLearner(), _lib.SgkDqnLearner()
    some = (ctypes.c_double * 8)()  # a non-NULL per-member pointer (never read: the handle is refused first)
    ptr = ctypes.cast(some, V)
    null_handle = (
        lambda: lib.sgk_ppo_epochs_members_hyper(None, ctypes.byref(P), 3, None, ptr),
        lambda: lib.sgk_ppo_cnn_epochs_members_hyper(None, ctypes.byref(C), 3, None, ptr),
        lambda: lib.sgk_dqn_sgd_step_members_hyper(None, ctypes.byref(D), 3, None, ptr, ptr),
        lambda: lib.sgk_policy_rollout_members_eps(None, ctypes.byref(w), 3, 0, 0.0, 0, 5, 0, None, None, None, None, ptr),
        lambda: lib.sgk_discounted_returns_members(None, ptr, None, ptr, 6, 4, 3, ptr))
    for call in null_handle:
        assert call() == _lib.ERR_INVALID
        assert b"NULL" in lib.sgk_last_error()
    # a NULL hyper_dev / epsilon pointer / gamma table is refused by name, before the handle is looked at (so without a device)
    null_member = (
        (lambda: lib.sgk_ppo_epochs_members_hyper(None, ctypes.byref(P), 3, None, None), b"hyper_dev is NULL"),
        (lambda: lib.sgk_ppo_cnn_epochs_members_hyper(None, ctypes.byref(C), 3, None, None), b"hyper_dev is NULL"),
        (lambda: lib.sgk_dqn_sgd_step_members_hyper(None, ctypes.byref(D), 3, None, ptr, None), b"hyper_dev is NULL"),
        (lambda: lib.sgk_policy_rollout_members_eps(None, ctypes.byref(w), 3, 0, 0.0, 0, 5, 0, None, None, None, None, None),
         b"member_epsilon_dev is NULL"),
        (lambda: lib.sgk_discounted_returns_members(None, ptr, None, ptr, 6, 4, 3, None), b"gamma_pow_dev is NULL"))
    for call, message in null_member:
        assert call() == _lib.ERR_INVALID
        assert message in lib.sgk_last_error(), lib.sgk_last_error()
    out = (ctypes.c_float * 4)()
    assert lib.sgk_discount_powers(0.9, 4, None) == _lib.ERR_INVALID and b"NULL" in lib.sgk_last_error()
    for t_max in (0, -1, 1025):
        assert lib.sgk_discount_powers(0.9, t_max, ctypes.cast(out, V)) == _lib.ERR_INVALID
        assert b"t_max" in lib.sgk_last_error()


# ---- the discount powers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("discount", [0.9, 0.99, 0.9995, 1.0])
def test_discount_powers_are_float32_of_python_pow(discount):
    got = _lib.discount_powers(discount, 1024)
    want = np.array([np.float32(discount ** t) for t in range(1024)], dtype=np.float32)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert _lib.discount_powers(discount, 7).tobytes() == want[:7].tobytes()  # a shorter row is the prefix


def test_discount_powers_are_the_table_behind_the_reference_returns(golden_dir):
    """The scan multiplies the rewards by this table and sums every suffix left to right in float32: with the rows of
    sgk_discount_powers that is discounted_returns_f32, and the reference's recorded returns."""
    import json

    cases = json.load(open(os.path.join(golden_dir, "discounted_returns.json")))
    assert cases
    for c in cases:
        r = np.array([float.fromhex(x) for x in c["rewards"]], dtype=np.float32)
        d = _lib.discount_powers(c["discount"], len(r)) * r
        got = np.array([np.cumsum(d[t:], dtype=np.float32)[-1] for t in range(len(r))], dtype=np.float32)
        assert got.tobytes() == S.discounted_returns_f32(r, c["discount"]).tobytes(), (c["discount"], len(r))
        assert [float(x).hex() for x in got] == c["returns"], (c["discount"], len(r))


# ---- --sweep ------------------------------------------------------------------------------------------------------------------------
PPO_ARGS = ["ppo-mlp", "-l", "1e-3", "-r", "4", "-e", "2", "-b", "7"]
DQN_ARGS = ["deep-q", "-l", "1e-3"]


def _parse(core, agent):
    return S.prepare_parser().parse_args(core + ["boat"] + agent)


def test_sweep_builds_the_cartesian_grid_first_flag_slowest_and_member_m_runs_point_m_mod_g():
    args = _parse(["-S", "3"], PPO_ARGS + ["--members", "12", "--sweep", "lr=1e-3,1e-2", "--sweep", "clipping=0.1,0.2,0.5"])
    names, grid = trainer.sweep_grid(args)
    assert names == ["lr", "clipping"]
    assert grid == [(1e-3, 0.1), (1e-3, 0.2), (1e-3, 0.5), (1e-2, 0.1), (1e-2, 0.2), (1e-2, 0.5)]  # G = 6, the first flag slowest
    mh = MH.sweep_member_hyper(names, grid, 12)
    assert sorted(mh) == ["clipping", "lr"]
    for m in range(12):  # member m: point m % G, replica m // G
        assert (mh["lr"][m], mh["clipping"][m]) == grid[m % 6]
    # the flag spelling of a name, the short alias and the core position are taken too; one flag is a grid of its own length
    args = _parse(["-M", "4", "-W", "entropy-bonus=0,0.01"], PPO_ARGS)
    assert trainer.sweep_grid(args) == (["entropy_bonus"], [(0.0,), (0.01,)])
    args = _parse(["-N", "12"], DQN_ARGS + ["-M", "3", "-W", "epsilon=0.01,0.1,0.5"])
    assert trainer.sweep_grid(args) == (["epsilon"], [(0.01,), (0.1,), (0.5,)])
    assert trainer.sweep_grid(_parse([], PPO_ARGS + ["--members", "3"])) is None  # no flag: no sweep
    # the seeds do not depend on the sweep: member m's stays default_member_seed(seed, m)
    assert len({S.default_member_seed(3, m) for m in range(12)}) == 12


def test_sweep_refusals_list_the_valid_names():
    ppo_names, dqn_names = "lr, clipping, critic_coeff, entropy_bonus, discount", "lr, discount, epsilon"
    with pytest.raises(SystemExit, match=r"G = 6.*--members 8 is no multiple of G = 6"):  # M % G != 0 names G
        trainer.sweep_grid(_parse([], PPO_ARGS + ["--members", "8", "--sweep", "lr=1e-3,1e-2", "--sweep", "clipping=0.1,0.2,0.5"]))
    with pytest.raises(SystemExit, match="needs --members.*" + ppo_names):  # a sweep without a population
        trainer.sweep_grid(_parse([], PPO_ARGS + ["--sweep", "lr=1e-3,1e-2"]))
    with pytest.raises(SystemExit, match="epsilon=0.1.*" + ppo_names):  # a name this agent does not have
        trainer.sweep_grid(_parse([], PPO_ARGS + ["--members", "2", "--sweep", "epsilon=0.1,0.2"]))
    with pytest.raises(SystemExit, match="clipping=0.1.*" + dqn_names):
        trainer.sweep_grid(_parse(["-N", "4"], DQN_ARGS + ["--members", "2", "--sweep", "clipping=0.1,0.2"]))
    with pytest.raises(SystemExit, match="batch_size.*" + ppo_names):  # shape and schedule are not swept
        trainer.sweep_grid(_parse([], PPO_ARGS + ["--members", "2", "--sweep", "batch_size=7,8"]))
    for empty in ("lr=", "lr", "lr=1e-3,,1e-2", "lr= "):  # an empty list, an empty item
        with pytest.raises(SystemExit, match=ppo_names):
            trainer.sweep_grid(_parse([], PPO_ARGS + ["--members", "2", "--sweep", empty]))
    with pytest.raises(SystemExit, match="floats.*" + ppo_names):
        trainer.sweep_grid(_parse([], PPO_ARGS + ["--members", "2", "--sweep", "lr=fast,slow"]))
    with pytest.raises(SystemExit, match="swept twice.*" + ppo_names):
        trainer.sweep_grid(_parse([], PPO_ARGS + ["--members", "4", "--sweep", "lr=1e-3,1e-2", "--sweep", "lr=1e-1,1"]))
    with pytest.raises(SystemExit, match="ppo-mlp, ppo-cnn or deep-q"):  # an agent without a population
        trainer.sweep_grid(_parse(["-M", "2", "-N", "4", "-W", "lr=0.1,0.2"], ["tabular-q", "-l", "0.1"]))
    # the entry point stops before it makes a directory or touches a device
    from safe_grid_agents_amd.__main__ import main

    with pytest.raises(SystemExit, match="no multiple of G = 2"):
        main(["-S", "3", "boat"] + PPO_ARGS + ["--members", "3", "--sweep", "lr=1e-3,1e-2"])


def test_the_sweep_table_is_mean_and_std_over_a_points_replicas():
    names, grid = ["lr"], [(1e-3,), (1e-2,)]
    lines = MH.sweep_table(names, grid, [1.0, 10.0, 3.0, 30.0], [0.5, 5.0, 0.5, 7.0])  # members 0, 2 -> point 0; 1, 3 -> point 1
    assert len(lines) == 2
    assert lines[0].startswith("lr=0.001") and "2.0000 +- 1.0000" in lines[0] and "0.5000 +- 0.0000" in lines[0] and "2 replicas" in lines[0]
    assert lines[1].startswith("lr=0.01") and "20.0000 +- 10.0000" in lines[1] and "6.0000 +- 1.0000" in lines[1]


# ---- validation that needs no device ------------------------------------------------------------------------------------------------
def test_validate_values_names_the_rule_that_is_broken():
    assert MH.validate_values("lr", (1e-3, 3e-3, 1e-2), 3) == [1e-3, 3e-3, 1e-2]
    assert MH.validate_values("epsilon", [0, 1], 2) == [0.0, 1.0] and MH.validate_values("discount", [1.0, 0.5], 2) == [1.0, 0.5]
    assert MH.validate_values("entropy_bonus", [0.0, -0.01], 2) == [0.0, -0.01]  # finite is all the others need
    for name, bad, message in (("lr", [1e-3, 0.0], "lr must be > 0"), ("lr", [1e-3, -1.0], "lr must be > 0"),
                               ("lr", [float("nan"), 1.0], "not finite"), ("clipping", [0.1, float("inf")], "not finite"),
                               ("epsilon", [0.5, 1.5], r"\[0, 1\]"), ("epsilon", [-0.1, 0.5], r"\[0, 1\]"),
                               ("discount", [0.0, 0.9], r"\(0, 1\]"), ("discount", [0.9, 1.01], r"\(0, 1\]"),
                               ("lr", [1e-3], "1 values, the population 2"), ("lr", [1e-3, 1e-2, 1e-1], "3 values, the population 2"),
                               ("lr", ["fast", 1.0], "sequence of 2 floats"), ("lr", 0.1, "sequence of 2 floats")):
        with pytest.raises(ValueError, match=message):
            MH.validate_values(name, bad, 2)
    got = MH.resolve({"lr": [1e-3, 1e-2]}, MH.DQN_NAMES, {"lr": 5e-4, "discount": 0.99, "epsilon": 0.01}, 2)
    assert got == {"lr": [1e-3, 1e-2], "discount": [0.99, 0.99], "epsilon": [0.01, 0.01]}  # names not given keep the shared value


def _fake_env(n_envs=12, n_cells=25, shape=(5, 5)):
    return types.SimpleNamespace(n_envs=n_envs, n_cells=n_cells, name="BoatRace-v0", device=0, action_space=types.SimpleNamespace(n=4),
                                 observation_space=types.SimpleNamespace(shape=(1,) + shape))


def _args(**kw):
    base = dict(lr=1e-3, discount=0.99, batch_size=7, epochs=2, clipping=0.2, entropy_bonus=0.01, critic_coeff=1.0, n_layers=2,
                n_hidden=100, n_channels=5, seed=3, epsilon=0.01, epsilon_anneal=1000, sync_every=10)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("cls, valid", [(S.BatchedPPOPopulation, MH.PPO_NAMES), (S.BatchedPPOCNNPopulation, MH.PPO_NAMES),
                                        (S.BatchedDeepQPopulation, MH.DQN_NAMES)])
def test_the_constructors_refuse_a_bad_member_hyper_before_touching_a_device(cls, valid):
    env, args = _fake_env(), _args()
    foreign = "epsilon" if "epsilon" not in valid else "clipping"
    for member_hyper, message in (({foreign: [0.1, 0.2, 0.3]}, "no %r here: the names are %s" % (foreign, ", ".join(valid))),
                                  ({"batch_size": [7, 8, 9]}, "no 'batch_size' here"),
                                  ({"lr": [1e-3, 1e-2]}, "2 values, the population 3"),
                                  ({"lr": [1e-3, 1e-2, 0.0]}, "lr must be > 0"),
                                  ({"discount": [0.9, 0.99, 1.5]}, r"\(0, 1\]"),
                                  ({"lr": [1e-3, float("nan"), 1e-2]}, "not finite"),
                                  ([1e-3, 1e-2, 1e-1], "must map a name")):
        with pytest.raises(ValueError, match=message):
            cls(env, args, 3, member_hyper=member_hyper)
    if "epsilon" in valid:
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            cls(env, args, 3, member_hyper={"epsilon": [0.01, 0.1, 1.5]})
