"""A population of INDEPENDENT PPO-CNN agents on one GPU: M runs of the reference's `ppo-cnn -r E`, gathered and trained in lockstep.

  BatchedPPOCNNPopulation   M PPOCNNAgents over one BatchedGridworldEnv of N = M x E envs; member m owns the envs m * E .. (m + 1) * E - 1.
                            Each of the 14 parameters, Adam's moments and the old policy's ten tensors exists once per member, stacked
                            on a leading member axis in one contiguous tensor [M, ...]. gather_rollout() is ONE launch
                            (sgk_convq_rollout_members: a workgroup serves one member) + the returns scan, learn() is ONE call
                            (sgk_ppo_cnn_epochs_members: three launches per epoch, a member axis on the grid). The members differ in
                            their weights, their envs and their draws, as M runs of the reference with different seeds do -- and, with
                            member_hyper, in lr, clipping, critic_coeff, entropy_bonus and discount (sgk_ppo_cnn_epochs_members_hyper,
                            sgk_discounted_returns_members): a sweep in the same launches, the values read from device memory.

What member m computes is what a BatchedPPOAgent(body="cnn", fused_conv_learn=True) computes on a handle of E envs created at
env_index_base + m * E with the handle's seed, member m's weights, member_keys[m] as the key of its minibatch draws and member m's
hyper-parameters in its `args` -- bit for bit (tests/test_gpu_ppo_cnn_members.py, tests/test_gpu_member_hyper.py), and through that the reference's own run (tests/golden/batched_ppo_cnn_*.npz).

The members can also act as ONE agent on all N envs (ensemble.EnsembleMixin: ensemble_act(), evaluate_ensemble()): every member's greedy
action on every board in one launch (sgk_convq_act_members_all), then the plurality vote (sgk_members_vote).

There is no torch path for a population: a shape without a kernel is a ValueError in the constructor.
"""
import ctypes
import types

import torch

from . import _lib
from .ensemble import EnsembleMixin
from .metering import BatchMetrics
from .ppo import BatchedPPOAgent, PPOCNNAgent
from .ppo_population import _INT64_MIN, _MASK, PPOMemberHyper, _as_i64, default_member_seed

# PPOCNNAgent's own parameters (state_dict keys, registration order) and the short names of the stacked tensors; the old policy reads
# the first ten (trunk, bottleneck, actor path)
MEMBER_KEYS = BatchedPPOAgent.CNN_PARAMS
PARAMS = ("w1", "b1", "w2", "b2", "wb", "bb", "wa", "ba", "la", "lab", "wv", "bv", "lv", "lvb")
N_OLD = 10
FUSED_BOARDS = ((5, 5), (6, 5), (6, 6), (6, 8), (7, 7), (7, 8), (7, 9))  # the boards the conv kernels are instantiated for
FUSED_CHANNELS = (4, 5, 8)


def stack_state_dicts(state_dicts):
    """PPOCNNAgent state dicts (their own 14 parameters, MEMBER_KEYS; anything else, e.g. old_policy.*, is ignored) -> {short name:
    tensor [M, ...]} in PARAMS order, one contiguous tensor per parameter. Pure torch; the values are copied bit for bit."""
    if not state_dicts:
        raise ValueError("no members to stack")
    out = {}
    for key, name in zip(MEMBER_KEYS, PARAMS):
        parts = [torch.as_tensor(sd[key]).detach().to(torch.float32) for sd in state_dicts]
        if any(p.shape != parts[0].shape for p in parts):
            raise ValueError("members disagree on the shape of %s" % key)
        out[name] = torch.stack(parts).contiguous()
    return out


def unstack_state_dict(stacked, m):
    """Member m's own parameters out of stack_state_dicts' tensors, keyed like PPOCNNAgent.state_dict() (copies)."""
    return {key: stacked[name][m].detach().clone() for key, name in zip(MEMBER_KEYS, PARAMS)}


class BatchedPPOCNNPopulation(EnsembleMixin, PPOMemberHyper):
    """M independent PPOCNNAgents over env's N = M x E envs (see the module docstring). ensemble_act() / evaluate_ensemble()
    (ensemble.EnsembleMixin) let the M members act as one agent on all N envs: every member votes on every env.

    args: the ppo-cnn flags (lr, discount, batch_size, epochs, clipping, entropy_bonus, critic_coeff, n_layers, n_channels, seed).
    member_seeds: member m's initial weights are those of PPOCNNAgent(env, args) built under torch.manual_seed(member_seeds[m])
    (default: default_member_seed(args.seed, m)); member_keys: the Philox key of member m's minibatch draws (default: the seeds).
    The action draws are keyed by the env's seed and the GLOBAL env index, as everywhere. member_hyper: as for BatchedPPOPopulation
    (PPOMemberHyper)."""

    def __init__(self, env, args, n_members, member_seeds=None, member_keys=None, member_hyper=None):
        M = int(n_members)
        channels, layers, batch = int(getattr(args, "n_channels", 0) or 0), int(args.n_layers), int(args.batch_size)
        board = tuple(int(v) for v in env.observation_space.shape[-2:])
        if M < 1 or env.n_envs % M:
            raise ValueError("n_envs (%d) is not a multiple of n_members (%d): every member owns the same number of envs" % (env.n_envs, M))
        if layers != 2:
            raise ValueError("a PPO-CNN population needs n_layers = 2 (the fused kernels' topology), not %d" % layers)
        if channels not in FUSED_CHANNELS:
            raise ValueError("a PPO-CNN population needs n_channels 4, 5 or 8 (sgk_ppo_cnn_epochs_members), not %d" % channels)
        if not 2 <= batch <= 64:
            raise ValueError("a PPO-CNN population needs 2 <= batch_size <= 64 (sgk_ppo_cnn_epochs_members), not %d" % batch)
        if board not in FUSED_BOARDS or env.action_space.n != 4:
            raise ValueError("the fused conv kernels do not cover %s (a %dx%d board, %d actions)" % ((env.name,) + board + (env.action_space.n,)))
        self._resolve_member_hyper(args, member_hyper, M)
        self.env, self.n_members, self.member_envs = env, M, env.n_envs // M
        self.device = "cuda:%d" % env.device
        self.n_channels, self.batch_size, self.epochs = channels, batch, int(args.epochs)
        self.discount = float(args.discount)
        self.lr, self.betas, self.adam_eps = float(args.lr), (0.9, 0.999), 1e-8  # torch.optim.Adam's defaults, as the reference's
        self.clipping, self.critic_coeff, self.entropy_bonus = float(args.clipping), float(args.critic_coeff), float(args.entropy_bonus)
        seed = int(getattr(args, "seed", 0) or 0)
        self.member_seeds = [int(s) & _MASK for s in (member_seeds if member_seeds is not None
                                                      else [default_member_seed(seed, m) for m in range(M)])]
        keys = self.member_seeds if member_keys is None else [int(k) & _MASK for k in member_keys]
        if len(self.member_seeds) != M or len(keys) != M:
            raise ValueError("member_seeds / member_keys need one entry per member (%d)" % M)
        self.member_keys = torch.tensor(_as_i64(keys), dtype=torch.int64, device=self.device)
        self._alloc_member_hyper()
        self._cfg = types.SimpleNamespace(**vars(args))
        self._cfg.device = "cpu"
        dicts = []
        for s in self.member_seeds:  # (on the CPU: torch.nn.Conv2d / Linear draw their initial weights from the CPU generator)
            torch.manual_seed(s)
            dicts.append(PPOCNNAgent(env, self._cfg).state_dict())
        dev = self.device
        self.cur = {k: v.to(dev) for k, v in stack_state_dicts(dicts).items()}
        self.old = {k: torch.empty_like(self.cur[k]) for k in PARAMS[:N_OLD]}
        self.adam_m = [torch.zeros_like(self.cur[k]) for k in PARAMS]
        self.adam_v = [torch.zeros_like(self.cur[k]) for k in PARAMS]
        self.step = torch.zeros(M, dtype=torch.int64, device=dev)
        self._stats = torch.zeros((M, self.epochs, 3), dtype=torch.float32, device=dev)
        self._ws_bytes = env.ppo_cnn_members_workspace_bytes(channels, batch, M)
        self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=dev)
        self.member_metrics = torch.empty((M, _lib.METRICS_LEN), dtype=torch.int64, device=dev)
        self._metrics_init = torch.zeros(_lib.METRICS_LEN, dtype=torch.int64)
        self._metrics_init[_lib.M_MAX_RETURN:_lib.M_MAX_MARGIN_POS + 1] = _INT64_MIN
        self._metrics_init = self._metrics_init.to(dev)
        self.draws = 0  # lockstep act_explore calls so far == the RNG draw index
        self._buffers = None
        self.sync()
        self.reset_member_metrics()

    # -- state ---------------------------------------------------------------------------------------------------------------------
    def sync(self):
        """PPOBaseAgent.sync for every member: old <- current on the first ten stacked tensors."""
        for k in PARAMS[:N_OLD]:
            self.old[k].copy_(self.cur[k])

    def tensors(self):
        """Everything learn() reads and updates, by name: the current parameters, Adam's moments, the step counters. (For snapshots:
        copy_ into them; the kernels hold their addresses.)"""
        out = dict(self.cur)
        out.update({"m_" + k: t for k, t in zip(PARAMS, self.adam_m)})
        out.update({"v_" + k: t for k, t in zip(PARAMS, self.adam_v)})
        out["step"] = self.step
        return out

    def pbt_tensors(self):
        """Every per-member tensor the learner or the acting reads or updates: what a clone takes from its source (exploit_explore)."""
        return list(self.cur.values()) + self.adam_m + self.adam_v + list(self.old.values()) + [self.step]

    def load_member(self, m, state_dict, hyper=None):
        """Member m's current weights <- a PPOCNNAgent state dict (its own parameters; `old_policy.*` keys, when present, give the old
        policy, else the old policy is left alone until the next sync()). hyper: {name: value}, member m's hyper-parameters (a
        population with member_hyper only), or None: left alone."""
        m = self._member_index(m)
        self._load_member_hyper(m, hyper)
        for key, name in zip(MEMBER_KEYS, PARAMS):
            src = torch.as_tensor(state_dict[key]).to(device=self.device, dtype=torch.float32)
            if tuple(src.shape) != tuple(self.cur[name][m].shape):
                raise ValueError("%s has shape %s, expected %s" % (key, tuple(src.shape), tuple(self.cur[name][m].shape)))
            self.cur[name][m].copy_(src)
        if all("old_policy." + k in state_dict for k in MEMBER_KEYS[:N_OLD]):
            for key, name in zip(MEMBER_KEYS[:N_OLD], PARAMS):
                self.old[name][m].copy_(torch.as_tensor(state_dict["old_policy." + key]).to(device=self.device, dtype=torch.float32))

    def member(self, m):
        """A PPOCNNAgent on the env's device holding COPIES of member m's weights (current and old policy), built from args that
        carry member m's hyper-parameters."""
        m = self._member_index(m)
        agent = PPOCNNAgent(self.env, self._member_cfg(m))
        sd = unstack_state_dict(self.cur, m)
        sd.update({"old_policy." + key: self.old[name][m].clone() for key, name in zip(MEMBER_KEYS[:N_OLD], PARAMS)})
        agent.load_state_dict(sd, strict=False)  # (the old policy's critic is never read)
        return agent

    def _member_index(self, m):
        m = int(m)
        if not 0 <= m < self.n_members:
            raise IndexError("member %d of %d" % (m, self.n_members))
        return m

    @property
    def stats(self):
        """float32 [M, epochs, 3] on the device: policy loss, value loss, entropy of every member's epochs in the last learn()."""
        return self._stats

    # -- metrics -------------------------------------------------------------------------------------------------------------------
    def reset_member_metrics(self):
        self.member_metrics.copy_(self._metrics_init.unsqueeze(0).expand_as(self.member_metrics))

    def member_batch_metrics(self):
        """One BatchMetrics per member from the per-member vectors (one read-back)."""
        vecs = self.member_metrics.cpu().numpy()
        return [BatchMetrics(v, self.env.reward_scale) for v in vecs]

    # -- acting --------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _acting_weights(t):
        """The rollout kernel's ten tensors (trunk, bottleneck, actor_cnn as the head, actor_linear) out of stacked tensors."""
        return {"w1": t["w1"], "b1": t["b1"], "w2": t["w2"], "b2": t["b2"], "wb": t["wb"], "bb": t["bb"], "wh": t["wa"], "bh": t["ba"],
                "wl": t["la"], "bl": t["lab"]}

    def _ensemble_weights(self):
        """EnsembleMixin: the tensors evaluate() acts greedily with -- the population's own, their addresses stay."""
        return self._acting_weights(self.cur)

    def _ensemble_act_all(self, weights, out):
        """EnsembleMixin's acting launch for the conv bodies: sgk_convq_act_members_all."""
        self.env.convq_act_members_all(weights, self.n_members, self.n_channels, out=out)

    def gather_rollout(self, cheat=False, horizon=None):
        """PPOBaseAgent.gather_rollout (reference policy_base.py:133-177) of every member at once: one episode per env under its
        member's old policy in ONE launch, then the returns scan. Returns a BatchedRollout over all N envs (columns m * E .. are member
        m's); the episodes are booked in the env's metrics vector and in member_metrics[m]."""
        from .loops import rollout_buffers, rollout_from_records

        env = self.env
        if self._buffers is None or (horizon is not None and int(horizon) != self._buffers["actions"].shape[0]):
            self._buffers = rollout_buffers(env, horizon)
        buf = self._buffers
        T = buf["actions"].shape[0]
        env.reset()
        env.convq_rollout_members(self._acting_weights(self.old), self.n_members, T, self.n_channels, mode="sample", draw_index0=self.draws,
                                  auto_reset=False, states=buf["states"], actions=buf["actions"], recs=buf["recs"], mask_finished=True,
                                  member_metrics=self.member_metrics)
        self.draws += T
        return rollout_from_records(env, buf, self.discount, cheat=cheat, masked=True, gamma_pow=self._gamma_table(T))

    def evaluate(self, eval_timesteps):
        """batched_default_eval (reference eval.py:8-56) for every member's CURRENT policy, greedy: its two phases as two launches of
        the members rollout. Returns (per-member BatchMetrics, the aggregate BatchMetrics); both metrics are reset first."""
        env = self.env
        env.metrics_reset()
        self.reset_member_metrics()
        env.reset()
        w = self._acting_weights(self.cur)
        if int(eval_timesteps) > 1:
            env.convq_rollout_members(w, self.n_members, int(eval_timesteps) - 1, self.n_channels, mode="greedy", epsilon=0.0,
                                      auto_reset=True, member_metrics=self.member_metrics)
        env.convq_rollout_members(w, self.n_members, int(env.info.max_iterations), self.n_channels, mode="greedy", epsilon=0.0,
                                  auto_reset=False, member_metrics=self.member_metrics)
        return self.member_batch_metrics(), BatchMetrics(env.metrics(), env.reward_scale)

    # -- learning ------------------------------------------------------------------------------------------------------------------
    def learn(self, rollout, history=None, rows=None, rows_out=None):
        """PPOBaseAgent.learn (reference policy_base.py:64-131) for every member in ONE call (three launches per epoch): member m's
        `epochs` minibatches are drawn from its own E trajectories of `rollout` with the key member_keys[m]. rows: int64 [M, epochs,
        batch] on the device, flat rows t * N + env (global env index) replacing the draws; rows_out: the same shape, receives the
        rows used. With a history, the three scalars of each epoch, averaged over the members, are written under the reference's tags
        after one read-back. Nothing else synchronises: the call can be recorded in a graph."""
        env, M = self.env, self.n_members
        chk = env._check  # ValueError for a tensor of the wrong device / dtype / shape: the kernels take raw pointers
        T, n = rollout.actions.shape
        C, cells = self.n_channels, env.n_cells
        if n != env.n_envs:
            raise ValueError("the rollout holds %d trajectories, the population's env %d" % (n, env.n_envs))
        L = _lib.SgkPpoCnnLearner()
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        chk(rollout.states, "rollout.states", shape=(T, n, cells), dtypes=("int8",))
        chk(rollout.actions, "rollout.actions", shape=(T, n), dtypes=("uint8",))
        chk(rollout.returns, "rollout.returns", shape=(n, T), dtypes=("float32",))
        chk(rollout.lengths, "rollout.lengths", shape=(n,), dtypes=("int32",))
        L.states, L.actions, L.returns, L.lengths = ptr(rollout.states), ptr(rollout.actions), ptr(rollout.returns), ptr(rollout.lengths)
        L.horizon, L.n_channels, L.batch, L.n_epochs, L.n_trajectories = T, C, self.batch_size, self.epochs, n
        shapes = ((M, C, 1, 3, 3), (M, C), (M, C, C, 3, 3), (M, C), (M, C, 1, 1, 1), (M, C), (M, C, C, 3, 3), (M, C), (M, 4, C * cells),
                  (M, 4), (M, C, C, 3, 3), (M, C), (M, 1, C * cells), (M, 1))
        for i, k in enumerate(PARAMS):
            chk(self.cur[k], "parameter " + k, shape=shapes[i], dtypes=("float32",))
            chk(self.adam_m[i], "Adam exp_avg of " + k, shape=shapes[i], dtypes=("float32",))
            chk(self.adam_v[i], "Adam exp_avg_sq of " + k, shape=shapes[i], dtypes=("float32",))
            L.params[i], L.m[i], L.v[i] = self.cur[k].data_ptr(), self.adam_m[i].data_ptr(), self.adam_v[i].data_ptr()
        for i, k in enumerate(PARAMS[:N_OLD]):
            chk(self.old[k], "old policy " + k, shape=shapes[i], dtypes=("float32",))
            L.old_params[i] = self.old[k].data_ptr()
        chk(self.step, "step", shape=(M,), dtypes=("int64",))
        chk(self._stats, "stats", shape=(M, self.epochs, 3), dtypes=("float32",))
        chk(self._ws, "workspace", numel=self._ws_bytes, dtypes=("uint8",))
        L.step, L.stats_out, L.workspace = ptr(self.step), ptr(self._stats), ptr(self._ws)
        if rows is not None:
            L.rows = ptr(chk(rows, "rows", shape=(M, self.epochs, self.batch_size), dtypes=("int64",)))
        if rows_out is not None:
            L.rows_out = ptr(chk(rows_out, "rows_out", shape=(M, self.epochs, self.batch_size), dtypes=("int64",)))
        L.lr, (L.beta1, L.beta2), L.eps = self.lr, self.betas, self.adam_eps
        L.clipping, L.critic_coeff, L.entropy_bonus = self.clipping, self.critic_coeff, self.entropy_bonus
        env.ppo_cnn_epochs_members(L, M, self.member_keys, member_hyper=None if self.hyper is None else self.hyper["learner"])
        if history is not None:
            self._log_stats(history)
        return history

    def _log_stats(self, history):
        stats = self._stats.mean(0).cpu().numpy()
        writer = history["writer"]
        for epoch in range(self.epochs):  # the reference's three scalars per epoch (policy_base.py:108-119), the members' mean
            writer.add_scalar("Train/policy_loss", float(stats[epoch, 0]), history["t_learn"])
            writer.add_scalar("Train/value_loss", float(stats[epoch, 1]), history["t_learn"])
            writer.add_scalar("Train/policy_entropy", float(stats[epoch, 2]), history["t_learn"])
            history["t_learn"] += 1
