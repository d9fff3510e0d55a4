#!/usr/bin/env python3
"""Generate tests/golden/batched_ppo_crmdp_transboat.npz by RUNNING THE REFERENCE's train() with its PPOCRMDPAgent (spiky/agents.py:74-270)
on `trans-boat` in the build container, patched as make_golden.py's golden_batched_ppo patches ppo-mlp / ppo-cnn (which stays as it is;
see its docstring for the stubs): rollout r of a gather_rollout call is the episode of env index base + r (_RolloutEnv),
Categorical.sample() is answered from Philox stream 3, torch.randint from stream 5, and -- as make_golden_crmdp.py does and explains --
`np.argsort` in spiky.agents' namespace sorts stably. Only arrays and JSON are committed.

    python tests/golden/make_golden_transition.py

The agent acts on TransitionBoatRace's observation [last board, board] ([board, board] at a reset): PPOCNNAgent with two input
channels. Per iteration the fixture holds both observation channels, the old policy's logits, the actions, the raw and the filtered
rewards, the returns, the agent's `states` / `rllb` as tables over prev cell * 25 + cur cell, the minibatch rows, the three losses and
the weights after learn; then the reference's default_eval of every index. Read by tests/batched_golden.py's PpoFixture (the keys
golden_batched_ppo writes, and more)."""
import json
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the repository and the reference on sys.path, chdirs into the reference)
import make_golden_crmdp as MC  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

NAME = "batched_ppo_crmdp_transboat.npz"
# seed 9: the first (1, 2, ...) under which the reference neither stops on a corrupt state without a bound nor violates a draw margin
# or the greedy gap (1 - 8 each miss a draw margin), and replaces at least one reward
ARGV = ["-S", "9", "-E", "3", "-EE", "10", "-V", "150", "-EV", "0", "trans-boat", "ppo-crmdp", "-l", "0.001", "-r", "6", "-e", "2", "-b", "64"]
BASE = 3000
N_CELLS, NONE = 25, -2 ** 31


def golden_transition(name, argv, base):
    import train as ref_train
    import safe_grid_agents.common.agents.policy_base as pb
    import safe_grid_agents.common.eval as eval_mod
    import safe_grid_agents.spiky.agents as ref_agents
    from safe_grid_agents.common.utils.meters import make_meters
    from torch.distributions import Categorical

    args = MG._PARSER.parse_args(argv)
    args.device, args.log_dir = "cpu", "unused"
    args.eval_every = 10 ** 9  # the evaluation happens once, at the end
    seed, n, iterations, horizon = int(args.seed), int(args.rollouts), int(args.episodes), MG.PPO_HORIZON
    env_name = MG._made_name(args)
    assert env_name == "TransitionBoatRace-v0"
    env = MG._RolloutEnv(env_name, n, base)
    gym = sys.modules["gym"]
    rec = {"logits": [], "margins": [], "rows": [], "weights": [], "rollouts": [], "episodes": [], "raw": [], "memory": [], "randint_calls": 0}
    captured, writers, evals = {}, [], []

    class PhiloxCategorical(Categorical):
        def __init__(self, probs=None, logits=None, validate_args=None):
            self._raw = logits.detach().clone()
            super().__init__(logits=logits)

        def sample(self, sample_shape=torch.Size()):
            assert tuple(self._raw.shape) == (1, 4)
            raw = self._raw.numpy()[0]
            a, margin, _ = MG._categorical_draw(raw, seed, base + env.cur, env.iteration * horizon + env.t)
            rec["logits"].append((env.iteration, env.cur, env.t, raw.copy()))
            rec["margins"].append(margin)
            return torch.tensor([a])

    def randint(high, size=None, dtype=None, **kw):
        assert high == n * horizon and tuple(size) == (args.batch_size,)
        step = rec["randint_calls"]
        rec["randint_calls"] += 1
        picks = [MG._ppo_row(seed, b, step, [horizon] * n, horizon) for b in range(args.batch_size)]
        rec["rows"].append([t * n + r for t, r in picks])       # the batch's flat row: t * N + env
        return torch.tensor([r * horizon + t for t, r in picks], dtype=torch.long)  # the reference's: rollout-major

    def weights_of(agent):
        return {k: v.detach().clone().numpy() for k, v in agent.state_dict().items() if not k.startswith("old_")}

    def memory_of(agent):
        flag, rew, rllb = np.zeros(N_CELLS ** 2, np.uint8), np.zeros(N_CELLS ** 2, np.int32), np.full(N_CELLS ** 2, NONE, np.int32)
        key = lambda s: MC._key(np.frombuffer(s, dtype=np.float32).reshape(2, 5, 5))  # noqa: E731
        for s, (ok, reward) in agent.states.items():
            flag[key(s)], rew[key(s)] = (1 if ok else 2), int(reward)
        for s, bound in agent.rllb.items():
            assert bound is not None, "a corrupt state without a bound: pick another seed"
            rllb[key(s)] = int(bound)
        return flag, rew, rllb

    C = ref_agents.PPOCRMDPAgent
    orig = {"make": gym.make, "Categorical": pb.Categorical, "torch": pb.torch, "init": pb.PPOBaseAgent.__init__, "gather": C.gather_rollout,
            "modified": C.get_modified_rewards_for_rollout, "learn": pb.PPOBaseAgent.learn, "writer": ref_train.SummaryWriter,
            "eval_map": ref_train.EVAL_MAP, "tm": ref_agents.track_metrics, "np": ref_agents.np}

    class W(MG.RecordingWriter):
        def __init__(self, log_dir=None):
            super().__init__(log_dir)
            writers.append(self)

    def spy_init(self, env_, a):
        orig["init"](self, env_, a)
        if "agent" not in captured:  # (the deepcopy inside the constructor does not come through here)
            captured["agent"] = self
            rec["weights"].append(weights_of(self))

    def spy_modified(self, boards, rewards):
        rec["raw"].append([float(v) for v in rewards])
        out = orig["modified"](self, boards, rewards)
        assert all(v is not None for v in out), "a reward without a bound: pick another seed"
        return out

    def spy_gather(self, env_, env_state, history, a):
        ro = orig["gather"](self, env_, env_state, history, a)
        rec["rollouts"].append(ro)
        rec["memory"].append(memory_of(self))
        return ro

    def spy_learn(self, states, actions, rewards, returns, history, a):
        history = orig["learn"](self, states, actions, rewards, returns, history, a)
        rec["weights"].append(weights_of(self))
        return history

    def spy_tm(history, env_, eval=False, write=True):
        rec["episodes"].append((env.iteration, env.cur, MG.RecordingWriter._num(env_._env.episode_return),
                                MG.RecordingWriter._num(env_._env.get_last_performance())))
        return orig["tm"](history, env_, eval=eval, write=write)

    def eval_every_index(agent, env_, eval_history, a):
        """default_eval of the trained agent on every index's env (the batch evaluates all of them in lockstep)."""
        for single in env.envs:
            tracked, gaps = [], []
            orig_tm, orig_act = eval_mod.track_metrics, agent.act

            def spy_eval_tm(history, e_, eval=False, write=True):
                tracked.append([MG.RecordingWriter._num(e_._env.episode_return), MG.RecordingWriter._num(e_._env.get_last_performance())])
                return orig_tm(history, e_, eval=eval, write=write)

            def act(state):
                with torch.no_grad():
                    p, _ = agent(torch.tensor(state, requires_grad=False, dtype=torch.float32, device=agent.device))
                top = torch.sort(p.reshape(-1), descending=True).values
                gaps.append(float(top[0] - top[1]))
                return orig_act(state)

            eval_mod.track_metrics, agent.act = spy_eval_tm, act
            first = len(single.actions_log)
            try:
                eh = make_meters({})
                eh["writer"], eh["period"] = MG.RecordingWriter(), 0
                with torch.no_grad():
                    eval_mod.default_eval(agent, single, eh, types.SimpleNamespace(eval_timesteps=MG.PPO_EVAL_TIMESTEPS, eval_visualize_episodes=0))
            finally:
                eval_mod.track_metrics = orig_tm
                del agent.act
            evals.append({"eval_episodes": tracked, "eval_actions": "".join(str(int(x)) for x in single.actions_log[first:]), "min_gap": min(gaps)})
        return eval_history

    gym.make = lambda _name: env
    pb.Categorical, pb.torch = PhiloxCategorical, MG._TorchProxy(randint)
    pb.PPOBaseAgent.__init__, pb.PPOBaseAgent.learn = spy_init, spy_learn
    C.gather_rollout, C.get_modified_rewards_for_rollout = spy_gather, spy_modified
    ref_agents.track_metrics, ref_agents.np = spy_tm, MC._StableNumpy()
    ref_train.SummaryWriter = W
    ref_train.EVAL_MAP = {args.agent_alias: eval_every_index}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref_train.train(args)
    finally:
        torch.set_num_threads(threads)
        gym.make, pb.Categorical, pb.torch = orig["make"], orig["Categorical"], orig["torch"]
        pb.PPOBaseAgent.__init__, pb.PPOBaseAgent.learn = orig["init"], orig["learn"]
        C.gather_rollout, C.get_modified_rewards_for_rollout = orig["gather"], orig["modified"]
        ref_agents.track_metrics, ref_agents.np = orig["tm"], orig["np"]
        ref_train.SummaryWriter, ref_train.EVAL_MAP = orig["writer"], orig["eval_map"]
    assert len(rec["rollouts"]) == iterations and len(rec["weights"]) == iterations + 1 and len(rec["raw"]) == iterations * n
    assert rec["randint_calls"] == iterations * args.epochs
    assert tuple(captured["agent"].state_dict()["network.0.0.weight"].shape) == (args.n_channels, 2, 3, 3)
    arrays, replaced = {}, []
    for k, ro in enumerate(rec["rollouts"]):
        lengths = np.array([len(a) for a in ro.actions], dtype=np.int32)
        assert (lengths == horizon).all()
        obs = np.asarray(ro.states, dtype=np.float32).reshape(n, horizon, 2, N_CELLS)
        assert (obs == np.round(obs)).all()
        raw = np.asarray(rec["raw"][k * n:(k + 1) * n], dtype=np.float32)
        rw = np.asarray(ro.rewards, dtype=np.float32)
        rt = np.asarray([[float(x) for x in r] for r in ro.returns], dtype=np.float32)
        lg = np.zeros((n, horizon, 4), dtype=np.float32)
        mg = np.ones((n, horizon), dtype=np.float64)
        for (it, r, t, logits), margin in zip(rec["logits"], rec["margins"]):
            if it == k:
                lg[r, t], mg[r, t] = logits, margin
        flag, rew, rllb = rec["memory"][k]
        replaced.append(int((raw != rw).sum()))
        arrays.update({"it%d_states" % k: obs[:, :, 1].astype(np.int8), "it%d_prev_states" % k: obs[:, :, 0].astype(np.int8),
                       "it%d_actions" % k: np.asarray(ro.actions, dtype=np.uint8).reshape(n, horizon), "it%d_raw_rewards" % k: raw,
                       "it%d_rewards" % k: rw, "it%d_returns" % k: rt, "it%d_lengths" % k: lengths, "it%d_logits" % k: lg, "it%d_margins" % k: mg,
                       "it%d_mem_flag" % k: flag, "it%d_mem_reward" % k: rew, "it%d_mem_rllb" % k: rllb,
                       "it%d_rows" % k: np.asarray(rec["rows"][k * args.epochs:(k + 1) * args.epochs], dtype=np.int64)})
        assert (arrays["it%d_prev_states" % k][:, 0] == arrays["it%d_states" % k][:, 0]).all()      # [board, board] at a reset
        assert (arrays["it%d_prev_states" % k][:, 1:] == arrays["it%d_states" % k][:, :-1]).all()   # then the last board
    for k, w in enumerate(rec["weights"]):
        for key, v in w.items():
            arrays["w%d_%s" % (k, key)] = v
    min_margin = float(min(rec["margins"]))
    min_margin_later = float(min(mg for (it, _, _, _), mg in zip(rec["logits"], rec["margins"]) if it > 0))
    min_gap = float(min(e["min_gap"] for e in evals))
    assert min_margin > MG.PPO_DRAW_MARGIN, ("a draw lies on an interval boundary: pick another seed", min_margin)
    assert min_margin_later > MG.PPO_DRAW_MARGIN_LATER, ("pick another seed", min_margin_later)
    assert min_gap > MG.PPO_GREEDY_GAP, ("a greedy step is a near-tie: pick another seed", min_gap)
    assert max(replaced) >= 1, "no reward was replaced in any iteration: pick another seed"
    losses = [[c[1], c[2], c[3]] for c in writers[0].calls if c[0] == "scalar" and c[1] in
              ("Train/policy_loss", "Train/value_loss", "Train/policy_entropy")]
    meta = {"argv": argv, "env": "BoatRace-v0", "reference_env": env_name, "cheat": bool(args.cheat), "seed": seed, "base": base, "n": n,
            "horizon": horizon, "iterations": iterations, "learn": True, "eval_timesteps": MG.PPO_EVAL_TIMESTEPS, "lr": args.lr,
            "discount": args.discount, "batch_size": args.batch_size, "epochs": args.epochs, "clipping": args.clipping,
            "entropy_bonus": args.entropy_bonus, "critic_coeff": args.critic_coeff, "n_layers": args.n_layers, "n_hidden": None,
            "n_channels": args.n_channels, "agent": args.agent_alias, "min_margin": min_margin, "min_margin_later": min_margin_later,
            "min_greedy_gap": min_gap, "episodes": rec["episodes"], "losses": losses, "agents": evals, "replaced_rewards": replaced,
            "weight_keys": sorted(rec["weights"][0].keys()), "torch_version": torch.__version__}
    path = os.path.join(HERE, name)
    np.savez_compressed(path, meta=np.array(json.dumps(meta, separators=(",", ":"))), **arrays)
    print("wrote", name, os.path.getsize(path), "bytes; min draw margin %.2e (later %.2e), min greedy gap %.2e, replaced rewards %s"
          % (min_margin, min_margin_later, min_gap, replaced))


def main():
    MG._install_stubs()
    from safe_grid_agents.parsing import prepare_parser

    MG._PARSER = prepare_parser()  # (it consumes module-level YAML dicts: once per process)
    if sys.argv[1:]:  # try another seed: python make_golden_transition.py SEED writes batched_ppo_crmdp_transboat_seedSEED.npz
        golden_transition(NAME.replace(".npz", "_seed%d.npz" % int(sys.argv[1])), ["-S", sys.argv[1]] + ARGV[2:], BASE)
    else:
        golden_transition(NAME, ARGV, BASE)
    leaked = [os.path.join(d, f) for d, _, fs in os.walk(MG.REF) for f in fs if f.endswith(".pyc")]
    assert not leaked, leaked


if __name__ == "__main__":
    main()
