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
import torch

from . import _lib
from .population import stack_state_dicts as _stack, unstack_state_dict as _unstack
from .ppo import BatchedPPOAgent, PPOCNNAgent
from .ppo_population import PPOMemberHyper

# PPOCNNAgent's own parameters (state_dict keys, registration order) and the short names of the stacked tensors; the old policy reads
# the first ten (trunk, bottleneck, actor path)
MEMBER_KEYS = BatchedPPOAgent.CNN_PARAMS
PARAMS = ("w1", "b1", "w2", "b2", "wb", "bb", "wa", "ba", "la", "lab", "wv", "bv", "lv", "lvb")
N_OLD = 10
FUSED_BOARDS = ((5, 5), (6, 5), (6, 6), (6, 8), (7, 7), (7, 8), (7, 9))  # the boards the conv kernels are instantiated for
FUSED_CHANNELS = (4, 5, 8)


def stack_state_dicts(state_dicts):
    """population.stack_state_dicts for PPOCNNAgent state dicts: their own 14 parameters (MEMBER_KEYS) under the names PARAMS."""
    return _stack(state_dicts, MEMBER_KEYS, PARAMS)


def unstack_state_dict(stacked, m):
    """Member m's own parameters out of stack_state_dicts' tensors, keyed like PPOCNNAgent.state_dict() (copies)."""
    return _unstack(stacked, m, MEMBER_KEYS, PARAMS)


class BatchedPPOCNNPopulation(PPOMemberHyper):
    """M independent PPOCNNAgents over env's N = M x E envs (see the module docstring). ensemble_act() / evaluate_ensemble()
    (ensemble.EnsembleMixin) let the M members act as one agent on all N envs: every member votes on every env.

    args: the ppo-cnn flags (lr, discount, batch_size, epochs, clipping, entropy_bonus, critic_coeff, n_layers, n_channels, seed).
    member_seeds: member m's initial weights are those of PPOCNNAgent(env, args) built under torch.manual_seed(member_seeds[m])
    (default: default_member_seed(args.seed, m)); member_keys: the Philox key of member m's minibatch draws (default: the seeds).
    The action draws are keyed by the env's seed and the GLOBAL env index, as everywhere. member_hyper: as for BatchedPPOPopulation
    (PPOMemberHyper)."""

    def __init__(self, env, args, n_members, member_seeds=None, member_keys=None, member_hyper=None):
        M = self._member_count(env, n_members)
        channels, layers, batch = int(getattr(args, "n_channels", 0) or 0), int(args.n_layers), int(args.batch_size)
        board = tuple(int(v) for v in env.observation_space.shape[-2:])
        if layers != 2:
            raise ValueError("a PPO-CNN population needs n_layers = 2 (the fused kernels' topology), not %d" % layers)
        if channels not in FUSED_CHANNELS:
            raise ValueError("a PPO-CNN population needs n_channels 4, 5 or 8 (sgk_ppo_cnn_epochs_members), not %d" % channels)
        if not 2 <= batch <= 64:
            raise ValueError("a PPO-CNN population needs 2 <= batch_size <= 64 (sgk_ppo_cnn_epochs_members), not %d" % batch)
        if board not in FUSED_BOARDS or env.action_space.n != 4:
            raise ValueError("the fused conv kernels do not cover %s (a %dx%d board, %d actions)" % ((env.name,) + board + (env.action_space.n,)))
        self.n_channels = channels
        dicts = self._init_ppo(env, args, M, batch, PPOCNNAgent, member_seeds, member_keys, member_hyper)
        self.cur = {k: v.to(self.device) for k, v in stack_state_dicts(dicts).items()}
        self.old = {k: torch.empty_like(self.cur[k]) for k in PARAMS[:N_OLD]}
        self._alloc_learner_state(PARAMS)
        self._ws_bytes = env.ppo_cnn_members_workspace_bytes(channels, batch, M)
        self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)
        self._alloc_member_metrics()
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

    # -- acting --------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _acting_weights(t):
        """The rollout kernel's ten tensors (trunk, bottleneck, actor_cnn as the head, actor_linear) out of stacked tensors."""
        return {"w1": t["w1"], "b1": t["b1"], "w2": t["w2"], "b2": t["b2"], "wb": t["wb"], "bb": t["bb"], "wh": t["wa"], "bh": t["ba"],
                "wl": t["la"], "bl": t["lab"]}

    def _rollout_members(self, weights, n_steps, **kw):
        self.env.convq_rollout_members(weights, self.n_members, n_steps, self.n_channels, **kw)

    def _old_weights(self):
        return self._acting_weights(self.old)

    def _greedy_weights(self):
        return self._acting_weights(self.cur)

    _ensemble_weights = _greedy_weights  # (EnsembleMixin: the tensors evaluate() acts with -- the population's own, their addresses stay)

    def _ensemble_act_all(self, weights, out):
        """EnsembleMixin's acting launch for the conv bodies: sgk_convq_act_members_all."""
        self.env.convq_act_members_all(weights, self.n_members, self.n_channels, out=out)

    # -- learning ------------------------------------------------------------------------------------------------------------------
    def learn(self, rollout, history=None, rows=None, rows_out=None):
        """PPOBaseAgent.learn (reference policy_base.py:64-131) for every member in ONE call (three launches per epoch): member m's
        `epochs` minibatches are drawn from its own E trajectories of `rollout` with the key member_keys[m]. rows: int64 [M, epochs,
        batch] on the device, flat rows t * N + env (global env index) replacing the draws; rows_out: the same shape, receives the
        rows used. With a history, the three scalars of each epoch, averaged over the members, are written under the reference's tags
        after one read-back. Nothing else synchronises: the call can be recorded in a graph."""
        env, M = self.env, self.n_members
        chk = env._check  # ValueError for a tensor of the wrong device / dtype / shape: the kernels take raw pointers
        C, cells = self.n_channels, env.n_cells
        L = _lib.SgkPpoCnnLearner()
        self._fill_learner(L, rollout, rows, rows_out)
        L.n_channels = C
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
        L.workspace = chk(self._ws, "workspace", numel=self._ws_bytes, dtypes=("uint8",)).data_ptr()
        env.ppo_cnn_epochs_members(L, M, self.member_keys, member_hyper=None if self.hyper is None else self.hyper["learner"])
        if history is not None:
            self._log_stats(history)
        return history
