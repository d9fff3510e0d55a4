"""ppo-crmdp: the reference's PPOCRMDPAgent (spiky/agents.py:74-270) -- PPO with a CNN body that, between a rollout and its discounted
returns, looks for states whose reward breaks a Lipschitz condition against the other visited states, remembers them as corrupt and
learns from a lower Lipschitz bound in place of their reward. The detection runs in libsgk.so on integer keys and integer rewards
(include/sgk.h: sgk_crmdp_keys, sgk_crmdp_filter, sgk_crmdp_filter_host; the tie rule of the walk is fixed there).

  PPOCRMDPAgent          the single-env drop-in (the PARITY path): PPOCNNAgent on the two-board observation of TransitionBoatRace; its
                         gather_rollout keeps the successors and filters every episode's rewards through sgk_crmdp_filter_host; a seeded
                         CPU run reproduces the reference's own run (tests/golden/train_transboat_ppo_crmdp_*.json).
  CRMDPMemory            the tables of n_agents agents (flag, reward, bound per key) on a device or on the host, with states() / rllb()
                         read back as dictionaries keyed by (prev cell, cur cell).
  BatchedPPOCRMDPAgent   BatchedPPOAgent(body="cnn") on a batched BoatRace env: the existing gather, then keys -> filter -> the existing
                         returns scan on the filtered rewards, all on the device. ONE memory; env order is the reference's rollout order
                         (-r N). transitions=True is the PARITY form: the policy acts on [previous board, board] through the two-channel
                         fused kernels (sgk_convq_rollout_trans) and reproduces the reference's own `-r N trans-boat ppo-crmdp` run
                         (tests/golden/batched_ppo_crmdp_transboat.npz). The default stays a labelled NON-parity: the detector sees
                         transitions (board before, board after), the POLICY the current board only.

Only the metric of TransitionBoatRace exists (d_trans_boat); the reference's other three levels live in its fork of
ai-safety-gridworlds alone, and another level is the reference's KeyError. The reference's _purge_memory is never entered on this
level (at most 24 keys against a cap of 20 steps per episode) and is not restated."""
import ctypes

import numpy as np

from . import _lib
from .ppo import BatchedPPOAgent, PPOCNNAgent

AGENT_VALUE = 2  # the DeepMind boards draw the agent as 2 (spiky/agents.py:46)
# env alias -> (metric kind, the level whose boards it reads): ENV_TO_D (:66-71) without the three fork-only levels
ENV_TO_D = {"trans-boat": (_lib.CRMDP_METRIC_TRANS_BOAT, "BoatRace-v0")}
MIN_KEYS_CAP = 24  # BoatRace shows at most 24 (previous cell, current cell) pairs: below that cap the reference would purge


def metric_for(env_alias, height, width):
    """The sgk_crmdp_metric of a level (KeyError outside ENV_TO_D, as the reference's table lookup)."""
    kind, _ = ENV_TO_D[env_alias]
    return _lib.SgkCrmdpMetric(kind, int(width), int(height) * int(width))


def _buffers(**arrays):
    return _lib.SgkCrmdpBuffers(**{k: (None if v is None else ctypes.c_void_p(v.ctypes.data if isinstance(v, np.ndarray) else v.data_ptr()))
                                   for k, v in arrays.items()})


class CRMDPMemory:
    """flag uint8 / reward int32 / rllb int32 [n_agents, n_keys] of sgk_crmdp_filter: torch tensors on `device` ("cpu": the host call's)."""

    def __init__(self, n_agents, metric, device="cpu"):
        import torch

        self.n_agents, self.metric = int(n_agents), metric
        self.n_cells = int(metric.n_cells)
        self.n_keys = self.n_cells ** 2
        if self.n_agents < 1 or self.n_keys > _lib.CRMDP_MAX_KEYS:
            raise ValueError("CRMDPMemory needs n_agents >= 1 and n_cells^2 <= %d" % _lib.CRMDP_MAX_KEYS)
        self.flag = torch.zeros((self.n_agents, self.n_keys), dtype=torch.uint8, device=device)
        self.reward = torch.zeros((self.n_agents, self.n_keys), dtype=torch.int32, device=device)
        self.bound = torch.full((self.n_agents, self.n_keys), _lib.CRMDP_NONE, dtype=torch.int32, device=device)

    def fields(self):
        return {"mem_flag": self.flag, "mem_reward": self.reward, "mem_rllb": self.bound}

    def states(self, agent=0):
        """{(prev cell, cur cell): (safe?, reward)}: the reference's `states` of one agent."""
        flag, reward = self.flag[agent].cpu().numpy(), self.reward[agent].cpu().numpy()
        return {divmod(int(k), self.n_cells): (bool(flag[k] == _lib.CRMDP_SAFE), int(reward[k])) for k in np.flatnonzero(flag)}

    def rllb(self, agent=0):
        """{(prev cell, cur cell): bound}: the reference's `rllb` of one agent (a key without a bound is left out)."""
        bound = self.bound[agent].cpu().numpy()
        return {divmod(int(k), self.n_cells): int(bound[k]) for k in np.flatnonzero(bound != _lib.CRMDP_NONE)}

    def n_corrupt(self):
        """Keys marked corrupt, over all agents (synchronising)."""
        return int((self.flag == _lib.CRMDP_CORRUPT).sum().item())


def crmdp_keys(env, states, last_boards, out):
    """sgk_crmdp_keys on `env`'s stream: states int8 [T, N, cells], last_boards int8 [N, cells] -> out int32 [N, T]."""
    T, n, cells = (int(v) for v in states.shape)
    for name, t, shape, dtype in (("states", states, (T, n, cells), "int8"), ("last_boards", last_boards, (n, cells), "int8"),
                                  ("out", out, (n, T), "int32")):
        env._check(t, name, shape=shape, dtypes=(dtype,))
    env._sync_torch_to_lib()
    _lib.check(env.lib.sgk_crmdp_keys(env._h.ptr, ctypes.c_void_p(states.data_ptr()), ctypes.c_void_p(last_boards.data_ptr()), T, n, cells,
                                      AGENT_VALUE, ctypes.byref(_buffers(keys=out))))
    env._sync_lib_to_torch()
    return out


def crmdp_filter(env, keys, rewards, lengths, memory, out):
    """sgk_crmdp_filter on `env`'s stream. keys int32 / rewards float32 [N, T], lengths int32 [N] or None, memory a CRMDPMemory on the
    env's device, out {"rewards_out" float32 [N, T], "order" int32 [N, T], "n_corrupt", "safe_index", "unbounded" int32 [N]}."""
    n, T = (int(v) for v in keys.shape)
    env._check(keys, "keys", shape=(n, T), dtypes=("int32",))
    env._check(rewards, "rewards", shape=(n, T), dtypes=("float32",))
    if lengths is not None:
        env._check(lengths, "lengths", shape=(n,), dtypes=("int32",))
    for name, shape, dtype in (("rewards_out", (n, T), "float32"), ("order", (n, T), "int32"), ("n_corrupt", (n,), "int32"),
                               ("safe_index", (n,), "int32"), ("unbounded", (n,), "int32")):
        env._check(out[name], name, shape=shape, dtypes=(dtype,))
    for name, t in memory.fields().items():
        env._check(t, name, shape=(memory.n_agents, memory.n_keys))
    env._sync_torch_to_lib()
    _lib.check(env.lib.sgk_crmdp_filter(env._h.ptr, ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(rewards.data_ptr()),
                                        None if lengths is None else ctypes.c_void_p(lengths.data_ptr()), n, T, memory.n_agents,
                                        ctypes.byref(memory.metric), ctypes.byref(_buffers(**out, **memory.fields()))))
    env._sync_lib_to_torch()
    return out


def filter_outputs(n, T, device):
    import torch

    return {"rewards_out": torch.zeros((n, T), dtype=torch.float32, device=device), "order": torch.zeros((n, T), dtype=torch.int32, device=device),
            "n_corrupt": torch.zeros(n, dtype=torch.int32, device=device), "safe_index": torch.zeros(n, dtype=torch.int32, device=device),
            "unbounded": torch.zeros(n, dtype=torch.int32, device=device)}


def crmdp_filter_host(keys, rewards, memory):
    """sgk_crmdp_filter_host for ONE trajectory of a host memory: keys int [L], rewards float [L] -> (modified rewards float32 [L],
    n_corrupt, unbounded)."""
    keys, rewards = np.ascontiguousarray(keys, np.int32).reshape(1, -1), np.ascontiguousarray(rewards, np.float32).reshape(1, -1)
    L = keys.shape[1]
    out = {"rewards_out": np.zeros((1, L), np.float32), "order": np.zeros((1, L), np.int32), "n_corrupt": np.zeros(1, np.int32),
           "safe_index": np.zeros(1, np.int32), "unbounded": np.zeros(1, np.int32)}
    tables = {k: v.numpy() for k, v in memory.fields().items()}
    _lib.check(_lib.load().sgk_crmdp_filter_host(keys.ctypes.data, rewards.ctypes.data, None, 1, L, 1, ctypes.byref(memory.metric),
                                                 ctypes.byref(_buffers(**out, **tables))))
    return out["rewards_out"][0], int(out["n_corrupt"][0]), int(out["unbounded"][0])


def observation_key(observation, n_cells):
    """The key of a two-board observation [2, H, W]: (cell of the agent before the step) * n_cells + (its cell after it)."""
    flat = np.asarray(observation).reshape(2, -1)
    prev, cur = np.flatnonzero(flat[0] == AGENT_VALUE), np.flatnonzero(flat[1] == AGENT_VALUE)
    return int(prev[0]) * n_cells + int(cur[0]) if len(prev) and len(cur) else -1


class PPOCRMDPAgent(PPOCNNAgent):
    """PPOCNNAgent whose rollouts' rewards pass the corrupt-reward filter before the returns are made (spiky/agents.py:74-270)."""

    def __init__(self, env, args):
        super().__init__(env, args)
        _, height, width = self.board_shape
        metric = metric_for(args.env_alias, height, width)  # (a level outside the table: KeyError, as ENV_TO_D[args.env_alias])
        if self.board_shape[0] != 2:
            raise ValueError("ppo-crmdp reads transitions: the observation must be [2, H, W], not %r" % (self.board_shape,))
        if float(getattr(env, "reward_scale", 1.0)) != 1.0:
            raise ValueError("ppo-crmdp works on integer rewards: a level with reward_scale != 1 is refused")
        self.memory = CRMDPMemory(1, metric, "cpu")
        self.replaced_rewards = 0  # steps of the last gather_rollout whose reward was replaced by a bound

    def states(self):
        return self.memory.states()

    def rllb(self):
        return self.memory.rllb()

    def filter_rewards(self, successors, rewards):
        """identify_corruption_in_trajectory + get_modified_rewards_for_rollout for one episode -> the modified rewards (floats)."""
        if 20 * len(rewards) < MIN_KEYS_CAP:
            raise ValueError("an episode of %d steps: the reference's state_memory_cap (20 x steps) would fall below the %d keys the level "
                             "shows and its random purge, which is not restated, would run" % (len(rewards), MIN_KEYS_CAP))
        keys = [observation_key(s, self.memory.n_cells) for s in successors]
        modified, n_corrupt, unbounded = crmdp_filter_host(keys, rewards, self.memory)
        if n_corrupt < 0:
            raise RuntimeError("ppo-crmdp: an observation of the episode shows no agent (value %d)" % AGENT_VALUE)
        if unbounded:
            raise RuntimeError("ppo-crmdp: %d corrupt state(s) of the episode have no reward bound (no safe state is known): the "
                               "reference returns None for them and stops in get_discounted_returns" % unbounded)
        self.replaced_rewards += int((modified != np.asarray(rewards, np.float32)).sum())
        return [float(v) for v in modified]

    def gather_rollout(self, env, env_state, history, args):
        """PPOBaseAgent.gather_rollout that also keeps every step's successor and filters the episode's rewards (:211-270)."""
        import torch

        from .agents import Rollout
        from .metering import track_metrics

        state = env_state[0]
        rollout = Rollout(states=[], actions=[], rewards=[], returns=[])
        self.replaced_rewards = 0
        for index in range(self.rollouts):
            states, actions, rewards, successors = [], [], [], []
            done = False
            while not done:
                with torch.no_grad():
                    action = self.old_policy.act_explore(state)
                successor, reward, done, info = env.step(action)
                if args.cheat:
                    reward = info["hidden_reward"]
                    try:
                        action = info["extra_observations"]["actual_actions"]
                    except KeyError:
                        pass
                states.append(state)
                actions.append(action)
                rewards.append(float(reward))
                successors.append(successor)
                state = successor
                history["t"] += 1
            if index:
                history["episode"] += 1  # train() already counted the first one
            rewards = self.filter_rewards(successors, rewards)
            returns = self.get_discounted_returns(rewards)
            history = track_metrics(history, env)
            rollout.states.append(states)
            rollout.actions.append(actions)
            rollout.rewards.append(rewards)
            rollout.returns.append(returns)
            state = env.reset()
        return rollout


class BatchedPPOCRMDPAgent(BatchedPPOAgent):
    """BatchedPPOAgent(body="cnn") on a batched BoatRace env (make("trans-boat", n_envs=N)) with the corrupt-reward filter between the
    gather and the returns scan: the env's boards after the last step are copied before the closing reset, sgk_crmdp_keys makes the keys
    of all N trajectories from the rollout's states, sgk_crmdp_filter detects and merges them into ONE memory in env order (the
    reference's rollout order with -r N), and sgk_discounted_returns scans the filtered rewards. Nothing leaves the device but, once per
    iteration, three integers (stats()).

    transitions=True (passed on to BatchedPPOAgent) is the PARITY path: the policy is the reference's two-channel PPOCNNAgent acting on
    [previous board, board] ([board, board] at a reset), gathered by sgk_convq_rollout_trans; it reproduces the reference's own run
    (tests/test_gpu_transition_golden.py); fused_transition_learn=True (passed on as well) makes its learn() sgk_ppo_cnn_epochs_trans
    instead of the torch graph (tests/test_gpu_transition_learn.py). The default (transitions=False) is NON-parity, labelled: the detector sees transitions, the
    policy does not -- it acts on the current board (1 channel). The single-env PPOCRMDPAgent is the parity path for one env.

    on_unbounded: "raise" (default) -- stats() raises RuntimeError naming the first trajectory with a corrupt state that has no bound
    (the reference's None and its crash); "keep" -- such steps keep their reward and are only counted."""

    def __init__(self, env, args, on_unbounded="raise", env_alias="trans-boat", **kwargs):
        if kwargs.setdefault("body", "cnn") != "cnn":
            raise ValueError("BatchedPPOCRMDPAgent has the reference's CNN body")
        if on_unbounded not in ("raise", "keep"):
            raise ValueError("on_unbounded must be 'raise' or 'keep'")
        kind, level = ENV_TO_D[getattr(args, "env_alias", None) or env_alias]
        from .envs import ENV_IDS

        if int(env.info.env_id) != ENV_IDS[level]:
            raise KeyError("ppo-crmdp has the metric of %s only; this env is level %d" % (level, int(env.info.env_id)))
        if float(env.reward_scale) != 1.0:
            raise ValueError("ppo-crmdp works on integer rewards: a level with reward_scale != 1 is refused")
        super().__init__(env, args, **kwargs)
        self.on_unbounded = on_unbounded
        self.metric = _lib.SgkCrmdpMetric(kind, int(env.info.width), int(env.n_cells))
        self.memory = CRMDPMemory(1, self.metric, self.device)
        self.crmdp = None  # the filter's buffers, allocated with the rollout's
        self._filter_rewards = self._filter  # what gather_rollout hands to rollout_from_records

    def _filter(self, env, buf):
        """rollout_from_records' hook, before the returns scan and the closing reset: -> the rewards the returns are made from."""
        import torch

        T, n = buf["actions"].shape
        if 20 * T < MIN_KEYS_CAP:
            raise ValueError("a horizon of %d steps: the reference's state_memory_cap (20 x steps) would fall below the %d keys the level "
                             "shows and its random purge, which is not restated, would run" % (T, MIN_KEYS_CAP))
        if self.crmdp is None or tuple(self.crmdp["keys"].shape) != (n, T):
            self.crmdp = filter_outputs(n, T, self.device)
            self.crmdp["keys"] = torch.zeros((n, T), dtype=torch.int32, device=self.device)
            self.crmdp["last_boards"] = torch.zeros((n, env.n_cells), dtype=torch.int8, device=self.device)
            self.crmdp["stats"] = torch.zeros(3, dtype=torch.int64, device=self.device)
            self.crmdp["index"] = torch.arange(n, dtype=torch.int64, device=self.device)
        c = self.crmdp
        c["last_boards"].copy_(env.boards().reshape(n, -1))
        crmdp_keys(env, buf["states"], c["last_boards"], c["keys"])
        crmdp_filter(env, c["keys"], buf["rewards"], buf["lengths"], self.memory,
                     {k: c[k] for k in ("rewards_out", "order", "n_corrupt", "safe_index", "unbounded")})
        # the iteration's three integers, made on the device and read by stats(): first unbounded trajectory (or -1), corrupt keys in
        # memory, replaced rewards
        c["stats"][0] = torch.where(c["unbounded"] != 0, c["index"], n).min()  # (n: none)
        c["stats"][1] = (self.memory.flag == _lib.CRMDP_CORRUPT).sum()
        c["stats"][2] = (c["rewards_out"] != buf["rewards"]).sum()
        return c["rewards_out"]

    def stats(self):
        """The last gather's figures, ONE read of three integers: {"corrupt_states", "replaced_rewards", "first_unbounded"}. Raises
        RuntimeError for a trajectory with an unbounded corrupt state unless on_unbounded="keep"."""
        if self.crmdp is None:
            return {"corrupt_states": 0, "replaced_rewards": 0, "first_unbounded": -1}
        first, corrupt, replaced = (int(v) for v in self.crmdp["stats"].cpu().tolist())
        first = first if first < self.crmdp["index"].numel() else -1
        if first >= 0 and self.on_unbounded == "raise":
            raise RuntimeError("ppo-crmdp: trajectory %d has a corrupt state without a reward bound (no safe state is known): the reference "
                               "returns None for it and stops in get_discounted_returns; on_unbounded='keep' keeps such rewards" % first)
        return {"corrupt_states": corrupt, "replaced_rewards": replaced, "first_unbounded": first}
