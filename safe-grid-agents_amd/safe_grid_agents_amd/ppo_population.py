"""A population of INDEPENDENT PPO-MLP agents on one GPU: M runs of the reference's `ppo-mlp -r E`, gathered and trained in lockstep.

  BatchedPPOPopulation   M PPOMLPAgents over one BatchedGridworldEnv of N = M x E envs; member m owns the envs m * E .. (m + 1) * E - 1.
                         Every parameter, Adam tensor and old-policy tensor exists once per member, stacked on a leading member axis in
                         one contiguous tensor [M, ...]. gather_rollout() is ONE launch (sgk_policy_rollout_members: a workgroup serves
                         one member) + the returns scan, learn() is ONE launch (sgk_ppo_epochs_members: workgroup m = member m). The
                         members differ in their weights, their envs and their draws, as M runs of the reference with different seeds
                         do -- and, with member_hyper, in lr, clipping, critic_coeff, entropy_bonus and discount: a sweep in the same two
                         launches (sgk_ppo_epochs_members_hyper, sgk_discounted_returns_members), the values read from device memory.

What member m computes is what a BatchedPPOAgent computes on a handle of E envs created at env_index_base + m * E with the handle's
seed, member m's weights, member_keys[m] as the key of its minibatch draws and member m's hyper-parameters in its `args` -- bit for
bit (tests/test_gpu_ppo_members.py, tests/test_gpu_member_hyper.py), and through that the reference's own run
(tests/golden/batched_ppo_*.npz).

There is no torch path for a population: a shape without a kernel is a ValueError in the constructor.
"""
import types

import torch

from . import _lib
from .member_hyper import PPO_NAMES
from .population import Population, default_member_seed  # noqa: F401 (default_member_seed: the name's first home, still imported from here)
from .population import stack_state_dicts as _stack, unstack_state_dict as _unstack
from .ppo import PPOMLPAgent

# PPOMLPAgent's own parameters (state_dict keys, registration order) and the short names of the stacked tensors
MEMBER_KEYS = ("network.0.0.weight", "network.0.0.bias", "network.1.0.0.weight", "network.1.0.0.bias", "actor.weight", "actor.bias",
               "critic.weight", "critic.bias")
PARAMS = ("w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc")
FUSED_CELLS = (25, 30, 36, 48, 49, 56, 63)  # the boards the fused policy kernel is instantiated for


def stack_state_dicts(state_dicts):
    """population.stack_state_dicts for PPOMLPAgent state dicts: their own parameters (MEMBER_KEYS) under the names PARAMS."""
    return _stack(state_dicts, MEMBER_KEYS, PARAMS)


def unstack_state_dict(stacked, m):
    """Member m's own parameters out of stack_state_dicts' tensors, keyed like PPOMLPAgent.state_dict() (copies)."""
    return _unstack(stacked, m, MEMBER_KEYS, PARAMS)


class PPOMemberHyper(Population):
    """What the two PPO populations (BatchedPPOPopulation, BatchedPPOCNNPopulation) share beyond population.Population: their
    per-member hyper-parameters, the constructors' common part, gather_rollout() and the learner struct's common fields.

    member_hyper=None: `hyper` is None and the population calls the shared-hyper entry points, exactly as without this class.
    Else `member_values` holds {name: [M floats]} for all of PPO_NAMES on the host and `hyper` the device tensors the kernels read:
      hyper["learner"]    float64 [M, 4], rows of sgk_ppo_member_hyper (lr, clipping, critic_coeff, entropy_bonus)
      hyper["discount"]   float64 [M], the members' discounts: no kernel reads it; it travels with a clone (exploit_explore), since the
                          float32 power table cannot be re-derived on the device bit for bit, and feeds pull_member_hyper
      hyper["gamma_pow"]  float32 [M, T], row m = float32(discount_m ** t): the table of sgk_discounted_returns_members, made at the
                          first gather_rollout for its horizon T (absent before)
    set_member_hyper copies into them, so the kernels and any recorded graph keep their addresses and see the new values.

    exploit_explore (PBTMixin) perturbs the learner row's four columns; the discount -- its value and its row of every cached power
    table -- is cloned only.

    A subclass supplies _rollout_members() and _greedy_weights() (population.Population) and _old_weights(), the old policy in the same
    layout."""

    HYPER_NAMES = PPO_NAMES
    PBT_COLUMNS = PPO_NAMES[:4]

    def _pbt_hyper_tensors(self):
        return [self.hyper["discount"]] + [self._gamma[T] for T in sorted(self._gamma)]

    def _pbt_pull_extra(self):
        return self.hyper["discount"]

    def _pbt_after_pull(self, rows, extra):
        for k, name in enumerate(PPO_NAMES[:4]):
            self.member_values[name] = [row[k] for row in rows]
        self.member_values["discount"] = list(extra)

    # -- construction --------------------------------------------------------------------------------------------------------------
    def _init_ppo(self, env, args, M, batch, agent_class, member_seeds, member_keys, member_hyper):
        """The constructors' common part after their refusals: the members' bookkeeping, args' shared values, and the members'
        initial state dicts -- agent_class(env, args) built on the CPU under torch.manual_seed(member_seeds[m]) -- which it returns."""
        self._init_members(env, args, M, member_seeds, member_keys, member_hyper)
        self.batch_size, self.epochs = batch, int(args.epochs)
        self.discount = float(args.discount)
        self.lr, self.betas, self.adam_eps = float(args.lr), (0.9, 0.999), 1e-8  # torch.optim.Adam's defaults, as the reference's
        self.clipping, self.critic_coeff, self.entropy_bonus = float(args.clipping), float(args.critic_coeff), float(args.entropy_bonus)
        self.draws = 0  # lockstep act_explore calls so far == the RNG draw index
        self._buffers = None
        self._cfg = types.SimpleNamespace(**vars(args))
        self._cfg.device = "cpu"
        dicts = []
        for s in self.member_seeds:  # (on the CPU: torch.nn layers draw their initial weights from the CPU generator)
            torch.manual_seed(s)
            dicts.append(agent_class(env, self._cfg).state_dict())
        return dicts

    def _alloc_learner_state(self, names):
        """Adam's moments of the stacked parameters `names` of self.cur, the step counters and the stats."""
        M, dev = self.n_members, self.device
        self.adam_m = [torch.zeros_like(self.cur[k]) for k in names]
        self.adam_v = [torch.zeros_like(self.cur[k]) for k in names]
        self.step = torch.zeros(M, dtype=torch.int64, device=dev)
        self._stats = torch.zeros((M, self.epochs, 3), dtype=torch.float32, device=dev)

    # -- per-member hyper-parameters -----------------------------------------------------------------------------------------------
    def _alloc_member_hyper(self):
        v, self._gamma = self.member_values, {}
        rows = [[v[k][m] for k in PPO_NAMES[:4]] for m in range(self.n_members)]
        self.hyper = {"learner": torch.tensor(rows, dtype=torch.float64, device=self.device),
                      "discount": torch.tensor(v["discount"], dtype=torch.float64, device=self.device)}

    def _store_member_hyper(self, name, vals):
        if name == "discount":
            self.hyper["discount"].copy_(torch.tensor(vals, dtype=torch.float64))
            for T, table in self._gamma.items():
                table.copy_(self._gamma_host(T))
        else:
            self.hyper["learner"][:, PPO_NAMES.index(name)].copy_(torch.tensor(vals, dtype=torch.float64))

    def _shared_hyper(self):
        return {"lr": self.lr, "clipping": self.clipping, "critic_coeff": self.critic_coeff, "entropy_bonus": self.entropy_bonus,
                "discount": self.discount}

    def _member_cfg(self, m):
        """self._cfg with member m's hyper-parameters, on the env's device: the `args` of the single agent member m equals."""
        cfg = types.SimpleNamespace(**vars(self._cfg))
        cfg.device = self.device
        vars(cfg).update(self.member_hyper_of(m))
        return cfg

    def _gamma_host(self, T):
        import numpy as np

        return torch.from_numpy(np.stack([_lib.discount_powers(d, T) for d in self.member_values["discount"]]))

    def _gamma_table(self, T):
        """hyper["gamma_pow"] for a horizon of T steps (None without member_hyper): made once per T, refreshed in place."""
        if self.hyper is None:
            return None
        T = int(T)
        if T not in self._gamma:
            self._pull_if_dirty()  # (the new table's rows come from the host mirror)
            self._gamma[T] = self._gamma_host(T).to(self.device)
        self.hyper["gamma_pow"] = self._gamma[T]
        return self._gamma[T]

    # -- acting and learning -------------------------------------------------------------------------------------------------------
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
        self._rollout_members(self._old_weights(), T, mode="sample", draw_index0=self.draws, auto_reset=False, states=buf["states"],
                              actions=buf["actions"], recs=buf["recs"], mask_finished=True, member_metrics=self.member_metrics)
        self.draws += T
        return rollout_from_records(env, buf, self.discount, cheat=cheat, masked=True, gamma_pow=self._gamma_table(T))

    def _fill_learner(self, L, rollout, rows, rows_out):
        """The fields sgk_ppo_learner and sgk_ppo_cnn_learner have in common, checked (ValueError for a tensor of the wrong device /
        dtype / shape: the kernels take raw pointers): the rollout, the sizes but the body's width, the step counters, the stats,
        rows / rows_out and the seven shared scalars."""
        env, M = self.env, self.n_members
        chk = env._check
        T, n = rollout.actions.shape
        if n != env.n_envs:
            raise ValueError("the rollout holds %d trajectories, the population's env %d" % (n, env.n_envs))
        chk(rollout.states, "rollout.states", shape=(T, n, env.n_cells), dtypes=("int8",))
        chk(rollout.actions, "rollout.actions", shape=(T, n), dtypes=("uint8",))
        chk(rollout.returns, "rollout.returns", shape=(n, T), dtypes=("float32",))
        chk(rollout.lengths, "rollout.lengths", shape=(n,), dtypes=("int32",))
        L.states, L.actions, L.returns, L.lengths = (rollout.states.data_ptr(), rollout.actions.data_ptr(), rollout.returns.data_ptr(),
                                                     rollout.lengths.data_ptr())
        L.horizon, L.batch, L.n_epochs, L.n_trajectories = T, self.batch_size, self.epochs, n
        chk(self.step, "step", shape=(M,), dtypes=("int64",))
        chk(self._stats, "stats", shape=(M, self.epochs, 3), dtypes=("float32",))
        L.step, L.stats_out = self.step.data_ptr(), self._stats.data_ptr()
        if rows is not None:
            L.rows = chk(rows, "rows", shape=(M, self.epochs, self.batch_size), dtypes=("int64",)).data_ptr()
        if rows_out is not None:
            L.rows_out = chk(rows_out, "rows_out", shape=(M, self.epochs, self.batch_size), dtypes=("int64",)).data_ptr()
        L.lr, (L.beta1, L.beta2), L.eps = self.lr, self.betas, self.adam_eps
        L.clipping, L.critic_coeff, L.entropy_bonus = self.clipping, self.critic_coeff, self.entropy_bonus

    @property
    def stats(self):
        """float32 [M, epochs, 3] on the device: policy loss, value loss, entropy of every member's epochs in the last learn()."""
        return self._stats

    def _log_stats(self, history):
        stats = self._stats.mean(0).cpu().numpy()
        writer = history["writer"]
        for epoch in range(self.epochs):  # the reference's three scalars per epoch (policy_base.py:108-119), the members' mean
            writer.add_scalar("Train/policy_loss", float(stats[epoch, 0]), history["t_learn"])
            writer.add_scalar("Train/value_loss", float(stats[epoch, 1]), history["t_learn"])
            writer.add_scalar("Train/policy_entropy", float(stats[epoch, 2]), history["t_learn"])
            history["t_learn"] += 1


class BatchedPPOPopulation(PPOMemberHyper):
    """M independent PPOMLPAgents over env's N = M x E envs (see the module docstring). ensemble_act() / evaluate_ensemble()
    (ensemble.EnsembleMixin) let the M members act as one agent on all N envs: every member votes on every env.

    args: the ppo-mlp flags (lr, discount, batch_size, epochs, clipping, entropy_bonus, critic_coeff, n_layers, n_hidden, seed).
    member_seeds: member m's initial weights are those of PPOMLPAgent(env, args) built under torch.manual_seed(member_seeds[m])
    (default: default_member_seed(args.seed, m)); member_keys: the Philox key of member m's minibatch draws (default: the seeds).
    The action draws are keyed by the env's seed and the GLOBAL env index, as everywhere. member_hyper: None (every member runs with
    args' values, the shared-hyper entry points), or {name: M floats} for names of lr, clipping, critic_coeff, entropy_bonus, discount
    (the others keep args' value for every member): see PPOMemberHyper."""

    def __init__(self, env, args, n_members, member_seeds=None, member_keys=None, member_hyper=None):
        M = self._member_count(env, n_members)
        hidden, layers, batch = int(getattr(args, "n_hidden", 0) or 0), int(args.n_layers), int(args.batch_size)
        if layers != 2:
            raise ValueError("a PPO population needs n_layers = 2 (the fused kernels' topology), not %d" % layers)
        if hidden not in (64, 100):
            raise ValueError("a PPO population needs n_hidden 64 or 100 (sgk_ppo_epochs_members), not %d" % hidden)
        if not 2 <= batch <= 64:
            raise ValueError("a PPO population needs 2 <= batch_size <= 64 (sgk_ppo_epochs_members), not %d" % batch)
        if env.n_cells not in FUSED_CELLS or env.action_space.n != 4:
            raise ValueError("the fused policy kernel does not cover %s (%d cells, %d actions)" % (env.name, env.n_cells, env.action_space.n))
        self.n_hidden = hidden
        dicts = self._init_ppo(env, args, M, batch, PPOMLPAgent, member_seeds, member_keys, member_hyper)
        K0, H, dev = env.n_cells, hidden, self.device
        self.cur = {k: v.to(dev) for k, v in stack_state_dicts(dicts).items()}
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        # transposed copies the kernels read: the learner keeps w1t / w2t current; sync() and load_member() refresh the others
        self.cur_t = {"w1t": f32(M, K0, H), "w2t": f32(M, H, H)}
        self.old = {"w1t": f32(M, K0, H), "b1": f32(M, H), "w2": f32(M, H, H), "w2t": f32(M, H, H), "b2": f32(M, H), "wa": f32(M, 4, H),
                    "w3t": f32(M, H, 4), "ba": f32(M, 4)}
        self._alloc_learner_state(PARAMS)
        self._alloc_member_metrics()
        self._ens_w3t = None
        self._refresh_transposes()
        self.sync()
        self.reset_member_metrics()

    # -- state ---------------------------------------------------------------------------------------------------------------------
    def _refresh_transposes(self):
        self.cur_t["w1t"].copy_(self.cur["w1"].transpose(1, 2))
        self.cur_t["w2t"].copy_(self.cur["w2"].transpose(1, 2))

    def sync(self):
        """PPOBaseAgent.sync for every member: old <- current on the stacked tensors, transposed copies included."""
        cur, old = self.cur, self.old
        old["w1t"].copy_(cur["w1"].transpose(1, 2))
        old["b1"].copy_(cur["b1"])
        old["w2"].copy_(cur["w2"])
        old["w2t"].copy_(cur["w2"].transpose(1, 2))
        old["b2"].copy_(cur["b2"])
        old["wa"].copy_(cur["wa"])
        old["w3t"].copy_(cur["wa"].transpose(1, 2))
        old["ba"].copy_(cur["ba"])

    def tensors(self):
        """Everything learn() reads and updates, by name: the current parameters and their transposed copies, Adam's moments, the step
        counters. (For snapshots: copy_ into them; the kernels hold their addresses.)"""
        out = dict(self.cur)
        out.update(self.cur_t)
        out.update({"m_" + k: t for k, t in zip(PARAMS, self.adam_m)})
        out.update({"v_" + k: t for k, t in zip(PARAMS, self.adam_v)})
        out["step"] = self.step
        return out

    def pbt_tensors(self):
        """Every per-member tensor the learner or the acting reads or updates: what a clone takes from its source (exploit_explore)."""
        return list(self.cur.values()) + list(self.cur_t.values()) + self.adam_m + self.adam_v + [self.step] + list(self.old.values())

    def load_member(self, m, state_dict, hyper=None):
        """Member m's current weights <- a PPOMLPAgent state dict (its own parameters; `old_policy.*` keys, when present, give the old
        policy, else the old policy is left alone until the next sync()). hyper: {name: value}, member m's hyper-parameters (a
        population with member_hyper only), or None: left alone."""
        m = self._member_index(m)
        self._load_member_hyper(m, hyper)
        for key, name in zip(MEMBER_KEYS, PARAMS):
            src = torch.as_tensor(state_dict[key]).to(device=self.device, dtype=torch.float32)
            if tuple(src.shape) != tuple(self.cur[name][m].shape):
                raise ValueError("%s has shape %s, expected %s" % (key, tuple(src.shape), tuple(self.cur[name][m].shape)))
            self.cur[name][m].copy_(src)
        self.cur_t["w1t"][m].copy_(self.cur["w1"][m].t())
        self.cur_t["w2t"][m].copy_(self.cur["w2"][m].t())
        if all("old_policy." + k in state_dict for k in MEMBER_KEYS[:6]):
            o = [torch.as_tensor(state_dict["old_policy." + k]).to(device=self.device, dtype=torch.float32) for k in MEMBER_KEYS[:6]]
            old = self.old
            old["w1t"][m].copy_(o[0].t()); old["b1"][m].copy_(o[1]); old["w2"][m].copy_(o[2]); old["w2t"][m].copy_(o[2].t())
            old["b2"][m].copy_(o[3]); old["wa"][m].copy_(o[4]); old["w3t"][m].copy_(o[4].t()); old["ba"][m].copy_(o[5])

    def member(self, m):
        """A PPOMLPAgent on the env's device holding COPIES of member m's weights (current and old policy), built from args that
        carry member m's hyper-parameters."""
        m = self._member_index(m)
        agent = PPOMLPAgent(self.env, self._member_cfg(m))
        own = unstack_state_dict(self.cur, m)
        old = self.old
        olds = {"network.0.0.weight": old["w1t"][m].t(), "network.0.0.bias": old["b1"][m], "network.1.0.0.weight": old["w2"][m],
                "network.1.0.0.bias": old["b2"][m], "actor.weight": old["wa"][m], "actor.bias": old["ba"][m]}
        sd = dict(own)
        sd.update({"old_policy." + k: v.clone() for k, v in olds.items()})
        agent.load_state_dict(sd, strict=False)  # (the old policy's critic is never read)
        return agent

    # -- acting --------------------------------------------------------------------------------------------------------------------
    def _rollout_members(self, weights, n_steps, **kw):
        self.env.policy_rollout_members(weights, self.n_members, n_steps, **kw)

    def _old_weights(self):
        o = self.old
        return {"w1t": o["w1t"], "b1": o["b1"], "w2": o["w2"], "b2": o["b2"], "w3t": o["w3t"], "b3": o["ba"]}

    def _greedy_weights(self):
        c = self.cur
        return {"w1t": self.cur_t["w1t"], "b1": c["b1"], "w2": c["w2"], "b2": c["b2"], "w3t": c["wa"].transpose(1, 2).contiguous(),
                "b3": c["ba"]}

    def _ensemble_weights(self):
        """_greedy_weights() at addresses that stay (EnsembleMixin records launches): the actor head's transpose is copied into one
        buffer, made at the first call."""
        c = self.cur
        if self._ens_w3t is None:
            self._ens_w3t = torch.empty_like(self.old["w3t"])
        self._ens_w3t.copy_(c["wa"].transpose(1, 2))
        return {"w1t": self.cur_t["w1t"], "b1": c["b1"], "w2": c["w2"], "b2": c["b2"], "w3t": self._ens_w3t, "b3": c["ba"]}

    # -- learning ------------------------------------------------------------------------------------------------------------------
    def learn(self, rollout, history=None, rows=None, rows_out=None):
        """PPOBaseAgent.learn (reference policy_base.py:64-131) for every member in ONE launch: member m's `epochs` minibatches are drawn
        from its own E trajectories of `rollout` with the key member_keys[m]. rows: int64 [M, epochs, batch] on the device, flat rows
        t * N + env (global env index) replacing the draws; rows_out: the same shape, receives the rows used. With a history, the
        three scalars of each epoch, averaged over the members, are written under the reference's tags after one read-back. Nothing
        else synchronises: the call can be recorded in a graph."""
        env, M = self.env, self.n_members
        chk = env._check  # ValueError for a tensor of the wrong device / dtype / shape: the kernel takes raw pointers
        K0, H = env.n_cells, self.n_hidden
        L = _lib.SgkPpoLearner()
        self._fill_learner(L, rollout, rows, rows_out)
        L.n_hidden = H
        shapes ={"w1": (M, H, K0), "b1": (M, H), "w2": (M, H, H), "b2": (M, H), "wa": (M, 4, H), "ba": (M, 4), "wc": (M, 1, H), "bc": (M, 1)}
        for i, k in enumerate(PARAMS):
            chk(self.cur[k], "parameter " + k, shape=shapes[k], dtypes=("float32",))
            chk(self.adam_m[i], "Adam exp_avg of " + k, shape=shapes[k], dtypes=("float32",))
            chk(self.adam_v[i], "Adam exp_avg_sq of " + k, shape=shapes[k], dtypes=("float32",))
            setattr(L, k, self.cur[k].data_ptr())
            L.m[i], L.v[i] = self.adam_m[i].data_ptr(), self.adam_v[i].data_ptr()
        old = self.old
        for t, name, shape in ((self.cur_t["w1t"], "w1t", (M, K0, H)), (self.cur_t["w2t"], "w2t", (M, H, H)), (old["w1t"], "old w1t", (M, K0, H)),
                               (old["b1"], "old b1", (M, H)), (old["w2t"], "old w2t", (M, H, H)), (old["b2"], "old b2", (M, H)),
                               (old["wa"], "old actor weight", (M, 4, H)), (old["ba"], "old actor bias", (M, 4))):
            chk(t, name, shape=shape, dtypes=("float32",))
        L.w1t, L.w2t = self.cur_t["w1t"].data_ptr(), self.cur_t["w2t"].data_ptr()
        L.ow1t, L.ob1, L.ow2t, L.ob2, L.owa, L.oba = (old[k].data_ptr() for k in ("w1t", "b1", "w2t", "b2", "wa", "ba"))
        env.ppo_epochs_members(L, M, self.member_keys, member_hyper=None if self.hyper is None else self.hyper["learner"])
        if history is not None:
            self._log_stats(history)
        return history
