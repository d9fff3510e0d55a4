"""The addresses recorded graphs depend on: every tensor of a population's tensors(), pbt_tensors(), hyper, member_metrics and member_keys
stays where the constructor put it through gather + learn (or warm-up + steps), set_member_hyper, load_member, exploit_explore and
evaluate -- for the three populations at the smallest shapes their kernels take (BoatRace, M = 3 members of E = 2 envs, batch 2, one
epoch, a horizon of 4 steps, a ring of 2 slices, 64 hidden units or 4 channels, member_hyper on lr). Along the way member_hyper_of()
returns what was set, and a population built without member_hyper refuses what needs one. No kernel here is new: the test guards the
host code the three populations share (safe_grid_agents_amd/population.py).

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import types

import pytest

import safe_grid_agents_amd as S
from safe_grid_agents_amd import deepq_population as DP
from safe_grid_agents_amd import ppo_cnn_population as PC
from safe_grid_agents_amd import ppo_population as PP

pytestmark = pytest.mark.gpu

M, E, HORIZON = 3, 2, 4
LR = [1e-3, 3e-3, 1e-2]
KINDS = {"ppo-mlp": (S.BatchedPPOPopulation, PP), "ppo-cnn": (S.BatchedPPOCNNPopulation, PC), "deep-q": (S.BatchedDeepQPopulation, DP)}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _build(kind, env, member_hyper):
    cls, _ = KINDS[kind]
    if kind == "deep-q":
        args = types.SimpleNamespace(batch_size=2, sync_every=2, epsilon_anneal=200, n_layers=2, n_hidden=64, seed=5, lr=1e-3, discount=0.99,
                                     epsilon=0.05)
        return cls(env, args, M, replay_slices=2, member_hyper=member_hyper)
    args = types.SimpleNamespace(batch_size=2, rollouts=E, epochs=1, n_layers=2, n_hidden=64, n_channels=4, device=0, log_gradients=False,
                                 cheat=False, seed=5, lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01, discount=0.99)
    return cls(env, args, M, member_hyper=member_hyper)


def _addresses(pop):
    named = {"tensors " + k: t for k, t in pop.tensors().items()}
    named.update({"pbt_tensors %d" % i: t for i, t in enumerate(pop.pbt_tensors())})
    named.update({"hyper " + k: t for k, t in pop.hyper.items()})
    named.update({"member_metrics": pop.member_metrics, "member_keys": pop.member_keys})
    return {k: (t.data_ptr(), tuple(t.shape), t.dtype) for k, t in named.items()}


def _iterate(kind, pop, env):
    if kind == "deep-q":
        pop.warmup(2)
        env.reset()
        for _ in range(2):
            pop.step(learn=True)
    else:
        pop.learn(pop.gather_rollout(horizon=HORIZON))
        pop.sync()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_no_tensor_moves_and_member_hyper_of_returns_what_was_set(kind):
    torch = _torch()
    module = KINDS[kind][1]
    env = S.BatchedGridworldEnv("BoatRace-v0", M * E, seed=11)
    try:
        # a population without member_hyper refuses what needs one, before anything is launched
        plain = _build(kind, env, None)
        assert plain.hyper is None and plain.member_values is None
        state = module.unstack_state_dict(plain.cur, 1)
        for refused in (lambda: plain.set_member_hyper("lr", LR), lambda: plain.load_member(0, state, hyper={"lr": 2e-3}),
                        lambda: plain.exploit_explore(fraction=1 / 3), plain.pull_member_hyper):
            with pytest.raises(ValueError, match="built without member_hyper"):
                refused()
        assert set(plain.member_hyper_of(0)) == set(plain.HYPER_NAMES) and plain.member_hyper_of(2)["lr"] == 1e-3
        del plain

        pop = _build(kind, env, {"lr": LR})
        assert [pop.member_hyper_of(m)["lr"] for m in range(M)] == LR
        before = _addresses(pop)
        _iterate(kind, pop, env)
        new = [2e-3, 4e-3, 8e-3]
        pop.set_member_hyper("lr", new)
        assert [pop.member_hyper_of(m)["lr"] for m in range(M)] == new
        pop.load_member(0, module.unstack_state_dict(pop.cur, 1), hyper={"lr": 5e-4})
        new[0] = 5e-4
        assert [pop.member_hyper_of(m)["lr"] for m in range(M)] == new
        others = {k: v for k, v in pop.member_hyper_of(1).items() if k != "lr"}
        assert others == {k: v for k, v in pop.member_hyper_of(0).items() if k != "lr"}  # (the names not given keep args' value)
        with pytest.raises(ValueError, match="no 'batch_size' here"):
            pop.set_member_hyper("batch_size", [1, 2, 3])
        scores = torch.tensor([2.0, -1.0, 1.0], dtype=torch.float64, device=pop.device)  # member 1 becomes member 0
        pop.exploit_explore(scores, fraction=1 / 3)
        assert pop.pbt_src.cpu().tolist() == [0, 0, 2]
        got = [pop.member_hyper_of(m)["lr"] for m in range(M)]  # (pulls the host mirror: one read-back)
        assert got[0] == new[0] and got[2] == new[2] and got[1] in (new[0] * 0.8, new[0] * 1.2)
        per_member, total = pop.evaluate(2)
        assert len(per_member) == M and total.episodes == sum(bm.episodes for bm in per_member) > 0
        torch.cuda.synchronize()
        after = _addresses(pop)
        assert sorted(k for k in after if k not in before) == ([] if kind == "deep-q" else ["hyper gamma_pow"])
        for k, where in before.items():
            assert after[k] == where, k
    finally:
        env.close()
