"""BatchedPPOCRMDPAgent(transitions=True) against the REFERENCE's own run (tests/golden/batched_ppo_crmdp_transboat.npz, made by
tests/golden/make_golden_transition.py: the reference's train() with its PPOCRMDPAgent on `trans-boat`, -r 6, three iterations, rollout
r = env index base + r, Categorical.sample() and torch.randint answered from the counter RNG): from the reference's initial weights
every iteration's gather holds both observation channels, the actions, the raw and the filtered rewards, the memory, the lengths and
the return bits exactly; the old policy's logits agree to rtol 1e-4 / atol 2e-5; with the fixture's minibatch rows the losses and the
weights after learn agree to rtol 2e-3 / atol 2e-5 (the tolerances tests/test_gpu_batched_golden.py uses for ppo-cnn); the evaluation
books the reference's episodes. The default agent (transitions=False: one input channel) does NOT take the reference's actions."""

import numpy as np
import pytest

import batched_golden as BG
import safe_grid_agents_amd as S

pytestmark = pytest.mark.gpu
NAME = "batched_ppo_crmdp_transboat.npz"


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _args(fx):
    a = fx.args(0)
    a.env_alias = "trans-boat"
    return a


def _metrics_agree(vec, want, O):
    got = {"sum_return": vec[O.M_SUM_RETURN], "sum_safety": vec[O.M_SUM_SAFETY], "sum_margin": vec[O.M_SUM_MARGIN],
           "sum_margin_pos": vec[O.M_SUM_MARGIN_POS], "episodes": vec[O.M_EPISODES], "margin_pos_count": vec[O.M_MARGIN_POS_COUNT]}
    for k, v in want.items():
        assert int(got[k]) == v, (k, int(got[k]), v)


def test_the_fixture_is_what_the_issue_asks_for():
    fx = BG.PpoFixture(NAME)
    m = fx.meta
    assert m["agent"] == "ppo-crmdp" and m["reference_env"] == "TransitionBoatRace-v0" and fx.n == 6 and 2 <= fx.iterations <= 3
    assert tuple(fx.weights(0)["network.0.0.weight"].shape) == (m["n_channels"], 2, 3, 3)
    assert tuple(fx.weights(0)["bottleneck.weight"].shape) == (m["n_channels"], 2, 1, 1)
    assert max(m["replaced_rewards"]) >= 1 and m["min_margin"] > 2e-5 and m["min_margin_later"] > 2e-4 and m["min_greedy_gap"] > 1e-4
    for k in range(fx.iterations):
        assert int((fx.it(k, "raw_rewards") != fx.it(k, "rewards")).sum()) == m["replaced_rewards"][k]
        assert (fx.it(k, "prev_states")[:, 0] == fx.it(k, "states")[:, 0]).all()
        assert (fx.it(k, "prev_states")[:, 1:] == fx.it(k, "states")[:, :-1]).all()


def test_the_transition_agent_reproduces_the_reference_run():
    from oracle import oracle as O

    torch = _torch()
    fx = BG.PpoFixture(NAME)
    m, T, n = fx.meta, fx.horizon, fx.n
    env = S.BatchedGridworldEnv(fx.env, n, seed=fx.seed, env_index_base=fx.base)
    env.bind_torch_stream()
    agent = S.BatchedPPOCRMDPAgent(env, _args(fx), transitions=True)
    try:
        assert agent.transitions and agent.fused_conv and agent.fused_rollout and not agent.fused_learn
        agent.net.load_state_dict({k: torch.as_tensor(v).to(agent.device) for k, v in fx.weights(0).items()}, strict=False)
        agent.sync()
        # the old policy's logits: the kernel's at the first step of a fresh episode, the module's on every observation of iteration 0
        env.reset()
        logits = torch.empty((n, 4), dtype=torch.float32, device=agent.device)
        env.convq_sample(agent._cw_old, 0, agent.n_channels, logits_out=logits, prev_boards=None)
        np.testing.assert_allclose(logits.cpu().numpy(), fx.it(0, "logits")[:, 0], rtol=1e-4, atol=2e-5)
        obs = np.stack((fx.it(0, "prev_states"), fx.it(0, "states")), axis=2).reshape(n * T, 2, 5, 5).astype(np.float32)
        with torch.no_grad():
            lg = agent.net.old_policy(torch.as_tensor(obs).to(agent.device))[0].cpu().numpy().reshape(n, T, 4)
        np.testing.assert_allclose(lg, fx.it(0, "logits"), rtol=1e-4, atol=2e-5)
        for k in range(fx.iterations):
            env.metrics_reset()
            ro = agent.gather_rollout(cheat=fx.cheat)
            assert (ro.lengths.cpu().numpy() == fx.it(k, "lengths")).all(), k
            bad = np.argwhere(ro.actions.cpu().numpy().T != fx.it(k, "actions"))
            assert bad.size == 0, (k, bad[:4], [float(fx.it(k, "margins")[i, t]) for i, t in bad[:4]])
            assert (ro.states.cpu().numpy().transpose(1, 0, 2) == fx.it(k, "states")).all(), k
            assert (ro.prev_states.cpu().numpy().transpose(1, 0, 2) == fx.it(k, "prev_states")).all(), k
            assert (agent._buffers["rewards"].cpu().numpy() == fx.it(k, "raw_rewards")).all(), k
            assert (ro.rewards.cpu().numpy() == fx.it(k, "rewards")).all(), k
            assert ro.returns.cpu().numpy().tobytes() == fx.it(k, "returns").tobytes(), k
            stats = agent.stats()
            assert stats["replaced_rewards"] == m["replaced_rewards"][k] and stats["first_unbounded"] == -1
            for mine, theirs in ((agent.memory.flag, "mem_flag"), (agent.memory.reward, "mem_reward"), (agent.memory.bound, "mem_rllb")):
                want = fx.it(k, theirs)
                got = mine[0].cpu().numpy()
                known = fx.it(k, "mem_flag") != 0 if theirs == "mem_reward" else np.ones_like(want, dtype=bool)
                assert (got[known] == want[known]).all(), (k, theirs)
            _metrics_agree(env.metrics(), fx.gather_metrics(k), O)
            w = S.RecordingWriter()
            agent.learn(ro, {"writer": w, "t": 0, "t_learn": 0}, rows=list(fx.it(k, "rows")))
            got = np.array([float.fromhex(c[2]) for c in w.calls]).reshape(m["epochs"], 3)
            np.testing.assert_allclose(got, fx.losses(k), rtol=2e-3, atol=2e-5)
            sd = agent.net.state_dict()
            for key, v in fx.weights(k + 1).items():
                np.testing.assert_allclose(sd[key].cpu().numpy(), v, rtol=2e-3, atol=2e-5, err_msg="%s after iteration %d" % (key, k))
            agent.sync()
        bm = S.batched_default_eval(agent, env, fx.eval_timesteps)
        BG.assert_eval_metrics(bm.vec, fx, O)
        assert bm.episodes == sum(len(a["eval_episodes"]) for a in fx.agents)
    finally:
        env.close()


def test_the_default_agent_does_not_take_the_reference_actions():
    """transitions=False with the reference's weights cut to the current board's channel -- the closest one-channel policy there is --
    gathers other actions than the reference: the NON-parity label of the default form was deserved."""
    torch = _torch()
    fx = BG.PpoFixture(NAME)
    n = fx.n
    env = S.BatchedGridworldEnv(fx.env, n, seed=fx.seed, env_index_base=fx.base)
    env.bind_torch_stream()
    agent = S.BatchedPPOCRMDPAgent(env, _args(fx), on_unbounded="keep")
    try:
        assert not agent.transitions
        sd = {k: torch.as_tensor(v[:, 1:2] if k in ("network.0.0.weight", "bottleneck.weight") else v).to(agent.device)
              for k, v in fx.weights(0).items()}
        agent.net.load_state_dict(sd, strict=False)
        agent.sync()
        ro = agent.gather_rollout()
        assert not hasattr(ro, "prev_states")
        differ = (ro.actions.cpu().numpy().T != fx.it(0, "actions")).mean()
        print("share of iteration 0's actions that differ from the reference's: %.3f" % differ)
        assert differ > 0
    finally:
        env.close()
