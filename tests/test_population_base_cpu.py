"""What the three populations (BatchedPPOPopulation, BatchedPPOCNNPopulation, BatchedDeepQPopulation) share, pinned without a device and
without a library call: the constructors' shape refusals (their exact messages and their order), stack_state_dicts / unstack_state_dict
of each module, and -- the last section -- that the shared parts exist ONCE (safe_grid_agents_amd/population.py).

The first two sections characterise behaviour: they passed before the shared parts were moved into population.py and pass unchanged
after. The last section ("one of each") describes the structure after the move and is the only part that fails on a tree in which every
population still carries its own copies.
"""
import importlib
import types

import pytest
import torch

import safe_grid_agents_amd as S
from safe_grid_agents_amd import deepq_population as DP
from safe_grid_agents_amd import ensemble, pbt
from safe_grid_agents_amd import ppo_cnn_population as PC
from safe_grid_agents_amd import ppo_population as PP


# the stub env and args of tests/test_member_hyper_abi.py: what a constructor reads before it touches a device
def _fake_env(n_envs=12, n_cells=25, shape=(5, 5)):
    return types.SimpleNamespace(n_envs=n_envs, n_cells=n_cells, name="BoatRace-v0", device=0, action_space=types.SimpleNamespace(n=4),
                                 observation_space=types.SimpleNamespace(shape=(1,) + shape))


def _args(**kw):
    base = dict(lr=1e-3, discount=0.99, batch_size=7, epochs=2, clipping=0.2, entropy_bonus=0.01, critic_coeff=1.0, n_layers=2,
                n_hidden=100, n_channels=5, seed=3, epsilon=0.01, epsilon_anneal=1000, sync_every=10)
    base.update(kw)
    return types.SimpleNamespace(**base)


# ---- the constructors' refusals -------------------------------------------------------------------------------------------------------
# per population: the faults in the constructor's order -- (env changes, args changes, the exact message) -- one thing changed at a time
_ENVS = "n_envs (10) is not a multiple of n_members (3): every member owns the same number of envs"
_MLP_BOARD = "the fused policy kernel does not cover BoatRace-v0 (16 cells, 4 actions)"
_SMALL = dict(n_cells=16, shape=(4, 4))
FAULTS = {
    "ppo": (S.BatchedPPOPopulation, [
        (dict(n_envs=10), {}, _ENVS),
        ({}, dict(n_layers=3), "a PPO population needs n_layers = 2 (the fused kernels' topology), not 3"),
        ({}, dict(n_hidden=32), "a PPO population needs n_hidden 64 or 100 (sgk_ppo_epochs_members), not 32"),
        ({}, dict(batch_size=1), "a PPO population needs 2 <= batch_size <= 64 (sgk_ppo_epochs_members), not 1"),
        (_SMALL, {}, _MLP_BOARD)],
        "a PPO population needs 2 <= batch_size <= 64 (sgk_ppo_epochs_members), not 65"),
    "ppo_cnn": (S.BatchedPPOCNNPopulation, [
        (dict(n_envs=10), {}, _ENVS),
        ({}, dict(n_layers=3), "a PPO-CNN population needs n_layers = 2 (the fused kernels' topology), not 3"),
        ({}, dict(n_channels=6), "a PPO-CNN population needs n_channels 4, 5 or 8 (sgk_ppo_cnn_epochs_members), not 6"),
        ({}, dict(batch_size=1), "a PPO-CNN population needs 2 <= batch_size <= 64 (sgk_ppo_cnn_epochs_members), not 1"),
        (_SMALL, {}, "the fused conv kernels do not cover BoatRace-v0 (a 4x4 board, 4 actions)")],
        "a PPO-CNN population needs 2 <= batch_size <= 64 (sgk_ppo_cnn_epochs_members), not 65"),
    "deepq": (S.BatchedDeepQPopulation, [
        (dict(n_envs=10), {}, _ENVS),
        ({}, dict(n_layers=3), "a Deep-Q population needs n_layers = 2 (the fused kernels' topology), not 3"),
        ({}, dict(n_hidden=32), "a Deep-Q population needs n_hidden 64 or 100 (sgk_dqn_sgd_step_members), not 32"),
        ({}, dict(batch_size=0), "a Deep-Q population needs 1 <= batch_size <= 64 (sgk_dqn_sgd_step_members), not 0"),
        (_SMALL, {}, _MLP_BOARD)],
        "a Deep-Q population needs 1 <= batch_size <= 64 (sgk_dqn_sgd_step_members), not 65"),
}
BAD_HYPER = {"lr": [1e-3, 1e-2]}  # two values for three members: the refusal that comes after every shape refusal


def _refused(cls, env_kw, args_kw, member_hyper=None):
    with pytest.raises(ValueError) as info:
        cls(_fake_env(**env_kw), _args(**args_kw), 3, member_hyper=member_hyper)
    return str(info.value)


@pytest.mark.parametrize("which", sorted(FAULTS))
def test_every_shape_refusal_has_its_exact_message(which):
    cls, faults, batch_65 = FAULTS[which]
    for env_kw, args_kw, message in faults:
        assert _refused(cls, env_kw, args_kw) == message
    assert _refused(cls, {}, dict(batch_size=65)) == batch_65
    assert _refused(cls, dict(n_envs=12), {}, member_hyper=BAD_HYPER) == "member_hyper['lr'] has 2 values, the population 3 members"


@pytest.mark.parametrize("which", sorted(FAULTS))
def test_two_faults_at_once_raise_the_earlier_one(which):
    """The order: member count, layers, hidden or channels, batch, board, then member_hyper."""
    cls, faults, _ = FAULTS[which]
    for i, (env_a, args_a, message) in enumerate(faults):
        for env_b, args_b, _later in faults[i + 1:]:
            assert _refused(cls, dict(env_a, **env_b), dict(args_a, **args_b)) == message
        assert _refused(cls, env_a, args_a, member_hyper=BAD_HYPER) == message  # every shape refusal comes before member_hyper's


# ---- stack_state_dicts / unstack_state_dict -------------------------------------------------------------------------------------------
H, CELLS, C = 4, 6, 2
SHAPES = {
    "ppo": (PP, ((H, CELLS), (H,), (H, H), (H,), (4, H), (4,), (1, H), (1,))),
    "ppo_cnn": (PC, ((C, 1, 3, 3), (C,), (C, C, 3, 3), (C,), (C, 1, 1, 1), (C,), (C, C, 3, 3), (C,), (4, C * CELLS), (4,), (C, C, 3, 3),
                     (C,), (1, C * CELLS), (1,))),
    "deepq": (DP, ((H, CELLS), (H,), (H, H), (H,), (4, H), (4,))),
}


def _state_dicts(module, shapes, n=3):
    """n CPU state dicts under the module's real keys: every float32 holds random BITS (NaN payloads, denormals, -0.0 included), so
    equality of the int32 views is equality bit for bit. Each dict also carries a key the functions must ignore."""
    assert len(module.MEMBER_KEYS) == len(module.PARAMS) == len(shapes)
    gen = torch.Generator().manual_seed(1234)
    dicts = []
    for _ in range(n):
        sd = {key: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, generator=gen).view(torch.float32)
              for key, shape in zip(module.MEMBER_KEYS, shapes)}
        sd["old_policy.extra"] = torch.zeros(3)
        dicts.append(sd)
    return dicts


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_stack(module, shapes, stack, unstack):
    dicts = _state_dicts(module, shapes)
    stacked = stack(dicts)
    assert tuple(stacked) == tuple(module.PARAMS)
    for key, name, shape in zip(module.MEMBER_KEYS, module.PARAMS, shapes):
        t = stacked[name]
        assert t.shape == (3,) + shape and t.dtype == torch.float32 and t.is_contiguous()
        for m, sd in enumerate(dicts):
            assert torch.equal(_bits(t[m]), _bits(sd[key])), (key, m)
    for m, sd in enumerate(dicts):
        own = unstack(stacked, m)
        assert tuple(own) == tuple(module.MEMBER_KEYS)
        for key, name in zip(module.MEMBER_KEYS, module.PARAMS):
            assert torch.equal(_bits(own[key]), _bits(sd[key])), (key, m)
            before = _bits(stacked[name]).clone()
            own[key].zero_()  # a copy: writing to it leaves the stacked tensor alone
            assert torch.equal(_bits(stacked[name]), before), (key, m)
    return dicts, stacked


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_stack_and_unstack_copy_every_member_bit_for_bit(which):
    module, shapes = SHAPES[which]
    dicts, _ = _check_stack(module, shapes, module.stack_state_dicts, module.unstack_state_dict)
    with pytest.raises(ValueError) as info:
        module.stack_state_dicts([])
    assert str(info.value) == "no members to stack"
    key = module.MEMBER_KEYS[2]
    dicts[1][key] = torch.zeros(tuple(d + 1 for d in shapes[2]))
    with pytest.raises(ValueError) as info:
        module.stack_state_dicts(dicts)
    assert str(info.value) == "members disagree on the shape of %s" % key


def test_the_package_exports_the_ppo_mlp_pair():
    assert S.stack_state_dicts is PP.stack_state_dicts and S.unstack_state_dict is PP.unstack_state_dict


# ---- one of each: holds once the shared parts live in population.py (the only section that fails before) ---------------------------------
POPULATIONS = (S.BatchedPPOPopulation, S.BatchedPPOCNNPopulation, S.BatchedDeepQPopulation)


def _function(cls, name):
    f = getattr(cls, name)
    return f.fget if isinstance(f, property) else f


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_the_generic_functions_give_what_the_modules_bindings_give(which):
    P = importlib.import_module("safe_grid_agents_amd.population")
    module, shapes = SHAPES[which]
    keys, names = module.MEMBER_KEYS, module.PARAMS
    dicts, stacked = _check_stack(module, shapes, lambda sds: P.stack_state_dicts(sds, keys, names),
                                  lambda st, m: P.unstack_state_dict(st, m, keys, names))
    dicts = _state_dicts(module, shapes)
    stacked, bound = P.stack_state_dicts(dicts, keys, names), module.stack_state_dicts(dicts)
    assert tuple(stacked) == tuple(bound)
    for name in names:
        assert torch.equal(_bits(stacked[name]), _bits(bound[name]))
    for m in range(3):
        a, b = P.unstack_state_dict(stacked, m, keys, names), module.unstack_state_dict(bound, m)
        assert tuple(a) == tuple(b) and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)
    with pytest.raises(ValueError) as info:
        P.stack_state_dicts([], keys, names)
    assert str(info.value) == "no members to stack"


def test_the_shared_methods_are_one_function_object():
    for name in ("evaluate", "_member_index", "reset_member_metrics", "member_batch_metrics", "set_member_hyper"):
        functions = [_function(cls, name) for cls in POPULATIONS]
        assert functions[0] is functions[1] is functions[2], name
    for name in ("gather_rollout", "_log_stats", "stats"):
        assert _function(S.BatchedPPOPopulation, name) is _function(S.BatchedPPOCNNPopulation, name), name
        assert name not in vars(S.BatchedDeepQPopulation)


def test_default_member_seed_is_one_object_under_its_three_paths():
    P = importlib.import_module("safe_grid_agents_amd.population")
    assert P.default_member_seed is PP.default_member_seed is S.default_member_seed
    assert P._MASK == 2 ** 64 - 1 and P._INT64_MIN == -(2 ** 63)
    assert P._as_i64([0, 2 ** 63, 2 ** 64 - 1, 2 ** 64 + 5]) == [0, -(2 ** 63), -1, 5]


def test_the_base_leaves_the_acting_launch_to_the_ensemble_mixin():
    P = importlib.import_module("safe_grid_agents_amd.population")
    bases = [b for b in vars(P).values() if isinstance(b, type) and all(issubclass(cls, b) for cls in POPULATIONS)
             and issubclass(b, ensemble.EnsembleMixin) and b is not ensemble.EnsembleMixin]
    assert bases, "population.py defines no base class over EnsembleMixin that the three populations share"
    for base in bases:
        assert issubclass(base, pbt.PBTMixin) and "_ensemble_act_all" not in vars(base)
    for cls in (S.BatchedPPOPopulation, S.BatchedDeepQPopulation):
        assert cls._ensemble_act_all is ensemble.EnsembleMixin._ensemble_act_all
    assert S.BatchedPPOCNNPopulation._ensemble_act_all is not ensemble.EnsembleMixin._ensemble_act_all
