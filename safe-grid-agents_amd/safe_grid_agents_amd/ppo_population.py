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
import ctypes
import types

import torch

from . import _lib
from .ensemble import EnsembleMixin
from .member_hyper import PPO_NAMES, resolve, validate_values
from .metering import BatchMetrics
from .pbt import PBTMixin
from .ppo import PPOMLPAgent

# PPOMLPAgent's own parameters (state_dict keys, registration order) and the short names of the stacked tensors
MEMBER_KEYS = ("network.0.0.weight", "network.0.0.bias", "network.1.0.0.weight", "network.1.0.0.bias", "actor.weight", "actor.bias",
               "critic.weight", "critic.bias")
PARAMS = ("w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc")
FUSED_CELLS = (25, 30, 36, 48, 49, 56, 63)  # the boards the fused policy kernel is instantiated for
_MASK = 2 ** 64 - 1
_INT64_MIN = -(2 ** 63)


def default_member_seed(seed, m):
    """Member m's default seed (initial weights: torch.manual_seed; minibatch draws: Philox key) from the run's seed: the splitmix64
    output function applied to seed + (m + 1) * 0x9E3779B97F4A7C15 (mod 2^64),

        z = (seed + (m + 1) * 0x9E3779B97F4A7C15) mod 2^64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) mod 2^64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) mod 2^64
        return z ^ (z >> 31)

    Both steps are bijections of the 64-bit integers (an odd multiplier; xor-shifts and odd multipliers), so the seeds of one run are
    distinct for distinct m < 2^64."""
    z = (int(seed) + (int(m) + 1) * 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def stack_state_dicts(state_dicts):
    """PPOMLPAgent state dicts (their own parameters, MEMBER_KEYS; anything else, e.g. old_policy.*, is ignored) -> {short name:
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
    """Member m's own parameters out of stack_state_dicts' tensors, keyed like PPOMLPAgent.state_dict() (copies)."""
    return {key: stacked[name][m].detach().clone() for key, name in zip(MEMBER_KEYS, PARAMS)}


def _as_i64(values):
    """uint64 values as the int64 bit patterns a torch tensor can hold."""
    return [v - 2 ** 64 if v >= 2 ** 63 else v for v in (int(x) & _MASK for x in values)]


class PPOMemberHyper(PBTMixin):
    """The per-member hyper-parameters of the two PPO populations (BatchedPPOPopulation, BatchedPPOCNNPopulation).

    member_hyper=None: `hyper` is None and the population calls the shared-hyper entry points, exactly as without this class.
    Else `member_values` holds {name: [M floats]} for all of PPO_NAMES on the host and `hyper` the device tensors the kernels read:
      hyper["learner"]    float64 [M, 4], rows of sgk_ppo_member_hyper (lr, clipping, critic_coeff, entropy_bonus)
      hyper["discount"]   float64 [M], the members' discounts: no kernel reads it; it travels with a clone (exploit_explore), since the
                          float32 power table cannot be re-derived on the device bit for bit, and feeds pull_member_hyper
      hyper["gamma_pow"]  float32 [M, T], row m = float32(discount_m ** t): the table of sgk_discounted_returns_members, made at the
                          first gather_rollout for its horizon T (absent before)
    set_member_hyper copies into them, so the kernels and any recorded graph keep their addresses and see the new values.

    exploit_explore (PBTMixin) perturbs the learner row's four columns; the discount -- its value and its row of every cached power
    table -- is cloned only."""

    hyper = None
    member_values = None
    PBT_COLUMNS = PPO_NAMES[:4]

    def _pbt_hyper_tensors(self):
        return [self.hyper["discount"]] + [self._gamma[T] for T in sorted(self._gamma)]

    def _pbt_pull_extra(self):
        return self.hyper["discount"]

    def _pbt_after_pull(self, rows, extra):
        for k, name in enumerate(PPO_NAMES[:4]):
            self.member_values[name] = [row[k] for row in rows]
        self.member_values["discount"] = list(extra)

    def _resolve_member_hyper(self, args, member_hyper, n_members):
        """Validation only (no device): ValueError for an unknown name, a wrong length, an invalid value."""
        if member_hyper is not None:
            defaults = {k: float(getattr(args, k)) for k in PPO_NAMES}
            self.member_values = resolve(member_hyper, PPO_NAMES, defaults, n_members)

    def _alloc_member_hyper(self):
        if self.member_values is not None:
            v, self._gamma = self.member_values, {}
            rows = [[v[k][m] for k in PPO_NAMES[:4]] for m in range(self.n_members)]
            self.hyper = {"learner": torch.tensor(rows, dtype=torch.float64, device=self.device),
                          "discount": torch.tensor(v["discount"], dtype=torch.float64, device=self.device)}

    def set_member_hyper(self, name, values):
        """Member m's `name` <- values[m] (validated: ValueError), copied INTO the device tensors (no new allocation): the next
        learn() / gather_rollout() -- a replay of a recorded one included -- runs with the new values. A population built without
        member_hyper has no per-member tensors: ValueError."""
        if self.hyper is None:
            raise ValueError("this population was built without member_hyper: its hyper-parameters are shared")
        if name not in PPO_NAMES:
            raise ValueError("member_hyper has no %r here: the names are %s" % (name, ", ".join(PPO_NAMES)))
        vals = validate_values(name, values, self.n_members)
        self.member_values[name] = vals
        if name == "discount":
            self.hyper["discount"].copy_(torch.tensor(vals, dtype=torch.float64))
            for T, table in self._gamma.items():
                table.copy_(self._gamma_host(T))
        else:
            self.hyper["learner"][:, PPO_NAMES.index(name)].copy_(torch.tensor(vals, dtype=torch.float64))

    def member_hyper_of(self, m):
        """{name: member m's value} for all of PPO_NAMES (the shared values without member_hyper): what the `args` of the single agent
        that member m equals carry."""
        m = self._member_index(m)
        self._pull_if_dirty()
        if self.member_values is None:
            return {"lr": self.lr, "clipping": self.clipping, "critic_coeff": self.critic_coeff, "entropy_bonus": self.entropy_bonus,
                    "discount": self.discount}
        return {k: self.member_values[k][m] for k in PPO_NAMES}

    def _member_cfg(self, m):
        """self._cfg with member m's hyper-parameters, on the env's device: the `args` of the single agent member m equals."""
        cfg = types.SimpleNamespace(**vars(self._cfg))
        cfg.device = self.device
        vars(cfg).update(self.member_hyper_of(m))
        return cfg

    def _load_member_hyper(self, m, hyper):
        """load_member's `hyper`: {name: value} for member m alone."""
        if hyper is None:
            return
        if self.hyper is None:
            raise ValueError("this population was built without member_hyper: its hyper-parameters are shared")
        self._pull_if_dirty()
        for name, value in dict(hyper).items():
            if name not in PPO_NAMES:
                raise ValueError("member_hyper has no %r here: the names are %s" % (name, ", ".join(PPO_NAMES)))
            vals = list(self.member_values[name])
            vals[m] = value
            self.set_member_hyper(name, vals)

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


class BatchedPPOPopulation(EnsembleMixin, PPOMemberHyper):
    """M independent PPOMLPAgents over env's N = M x E envs (see the module docstring). ensemble_act() / evaluate_ensemble()
    (ensemble.EnsembleMixin) let the M members act as one agent on all N envs: every member votes on every env.

    args: the ppo-mlp flags (lr, discount, batch_size, epochs, clipping, entropy_bonus, critic_coeff, n_layers, n_hidden, seed).
    member_seeds: member m's initial weights are those of PPOMLPAgent(env, args) built under torch.manual_seed(member_seeds[m])
    (default: default_member_seed(args.seed, m)); member_keys: the Philox key of member m's minibatch draws (default: the seeds).
    The action draws are keyed by the env's seed and the GLOBAL env index, as everywhere. member_hyper: None (every member runs with
    args' values, the shared-hyper entry points), or {name: M floats} for names of lr, clipping, critic_coeff, entropy_bonus, discount
    (the others keep args' value for every member): see PPOMemberHyper."""

    def __init__(self, env, args, n_members, member_seeds=None, member_keys=None, member_hyper=None):
        M = int(n_members)
        hidden, layers, batch = int(getattr(args, "n_hidden", 0) or 0), int(args.n_layers), int(args.batch_size)
        if M < 1 or env.n_envs % M:
            raise ValueError("n_envs (%d) is not a multiple of n_members (%d): every member owns the same number of envs" % (env.n_envs, M))
        if layers != 2:
            raise ValueError("a PPO population needs n_layers = 2 (the fused kernels' topology), not %d" % layers)
        if hidden not in (64, 100):
            raise ValueError("a PPO population needs n_hidden 64 or 100 (sgk_ppo_epochs_members), not %d" % hidden)
        if not 2 <= batch <= 64:
            raise ValueError("a PPO population needs 2 <= batch_size <= 64 (sgk_ppo_epochs_members), not %d" % batch)
        if env.n_cells not in FUSED_CELLS or env.action_space.n != 4:
            raise ValueError("the fused policy kernel does not cover %s (%d cells, %d actions)" % (env.name, env.n_cells, env.action_space.n))
        self._resolve_member_hyper(args, member_hyper, M)
        self.env, self.n_members, self.member_envs = env, M, env.n_envs // M
        self.device = "cuda:%d" % env.device
        self.n_hidden, self.batch_size, self.epochs = hidden, batch, int(args.epochs)
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
        for s in self.member_seeds:  # (on the CPU: torch.nn.Linear draws its initial weights from the CPU generator)
            torch.manual_seed(s)
            dicts.append(PPOMLPAgent(env, self._cfg).state_dict())
        K0, H, dev = env.n_cells, hidden, self.device
        self.cur = {k: v.to(dev) for k, v in stack_state_dicts(dicts).items()}
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        # transposed copies the kernels read: the learner keeps w1t / w2t current; sync() and load_member() refresh the others
        self.cur_t = {"w1t": f32(M, K0, H), "w2t": f32(M, H, H)}
        self.old = {"w1t": f32(M, K0, H), "b1": f32(M, H), "w2": f32(M, H, H), "w2t": f32(M, H, H), "b2": f32(M, H), "wa": f32(M, 4, H),
                    "w3t": f32(M, H, 4), "ba": f32(M, 4)}
        self.adam_m = [torch.zeros_like(self.cur[k]) for k in PARAMS]
        self.adam_v = [torch.zeros_like(self.cur[k]) for k in PARAMS]
        self.step = torch.zeros(M, dtype=torch.int64, device=dev)
        self._stats = torch.zeros((M, self.epochs, 3), dtype=torch.float32, device=dev)
        self.member_metrics = torch.empty((M, _lib.METRICS_LEN), dtype=torch.int64, device=dev)
        self._metrics_init = torch.zeros(_lib.METRICS_LEN, dtype=torch.int64)
        self._metrics_init[_lib.M_MAX_RETURN:_lib.M_MAX_MARGIN_POS + 1] = _INT64_MIN
        self._metrics_init = self._metrics_init.to(dev)
        self.draws = 0  # lockstep act_explore calls so far == the RNG draw index
        self._buffers = None
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
        env.policy_rollout_members(self._old_weights(), self.n_members, T, mode="sample", draw_index0=self.draws, auto_reset=False,
                                   states=buf["states"], actions=buf["actions"], recs=buf["recs"], mask_finished=True,
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
        w = self._greedy_weights()
        if int(eval_timesteps) > 1:
            env.policy_rollout_members(w, self.n_members, int(eval_timesteps) - 1, mode="greedy", epsilon=0.0, auto_reset=True,
                                       member_metrics=self.member_metrics)
        env.policy_rollout_members(w, self.n_members, int(env.info.max_iterations), mode="greedy", epsilon=0.0, auto_reset=False,
                                   member_metrics=self.member_metrics)
        return self.member_batch_metrics(), BatchMetrics(env.metrics(), env.reward_scale)

    # -- learning ------------------------------------------------------------------------------------------------------------------
    def learn(self, rollout, history=None, rows=None, rows_out=None):
        """PPOBaseAgent.learn (reference policy_base.py:64-131) for every member in ONE launch: member m's `epochs` minibatches are drawn
        from its own E trajectories of `rollout` with the key member_keys[m]. rows: int64 [M, epochs, batch] on the device, flat rows
        t * N + env (global env index) replacing the draws; rows_out: the same shape, receives the rows used. With a history, the
        three scalars of each epoch, averaged over the members, are written under the reference's tags after one read-back. Nothing
        else synchronises: the call can be recorded in a graph."""
        env, M = self.env, self.n_members
        chk = env._check  # ValueError for a tensor of the wrong device / dtype / shape: the kernel takes raw pointers
        T, n = rollout.actions.shape
        K0, H = env.n_cells, self.n_hidden
        if n != env.n_envs:
            raise ValueError("the rollout holds %d trajectories, the population's env %d" % (n, env.n_envs))
        L = _lib.SgkPpoLearner()
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        chk(rollout.states, "rollout.states", shape=(T, n, K0), dtypes=("int8",))
        chk(rollout.actions, "rollout.actions", shape=(T, n), dtypes=("uint8",))
        chk(rollout.returns, "rollout.returns", shape=(n, T), dtypes=("float32",))
        chk(rollout.lengths, "rollout.lengths", shape=(n,), dtypes=("int32",))
        L.states, L.actions, L.returns, L.lengths = ptr(rollout.states), ptr(rollout.actions), ptr(rollout.returns), ptr(rollout.lengths)
        L.horizon, L.n_hidden, L.batch, L.n_epochs, L.n_trajectories = T, H, self.batch_size, self.epochs, n
        shapes = {"w1": (M, H, K0), "b1": (M, H), "w2": (M, H, H), "b2": (M, H), "wa": (M, 4, H), "ba": (M, 4), "wc": (M, 1, H), "bc": (M, 1)}
        for i, k in enumerate(PARAMS):
            chk(self.cur[k], "parameter " + k, shape=shapes[k], dtypes=("float32",))
            chk(self.adam_m[i], "Adam exp_avg of " + k, shape=shapes[k], dtypes=("float32",))
            chk(self.adam_v[i], "Adam exp_avg_sq of " + k, shape=shapes[k], dtypes=("float32",))
            setattr(L, k, ptr(self.cur[k]))
            L.m[i], L.v[i] = self.adam_m[i].data_ptr(), self.adam_v[i].data_ptr()
        old = self.old
        for t, name, shape in ((self.cur_t["w1t"], "w1t", (M, K0, H)), (self.cur_t["w2t"], "w2t", (M, H, H)), (old["w1t"], "old w1t", (M, K0, H)),
                               (old["b1"], "old b1", (M, H)), (old["w2t"], "old w2t", (M, H, H)), (old["b2"], "old b2", (M, H)),
                               (old["wa"], "old actor weight", (M, 4, H)), (old["ba"], "old actor bias", (M, 4))):
            chk(t, name, shape=shape, dtypes=("float32",))
        L.w1t, L.w2t = ptr(self.cur_t["w1t"]), ptr(self.cur_t["w2t"])
        L.ow1t, L.ob1, L.ow2t, L.ob2, L.owa, L.oba = (ptr(old["w1t"]), ptr(old["b1"]), ptr(old["w2t"]), ptr(old["b2"]), ptr(old["wa"]),
                                                      ptr(old["ba"]))
        chk(self.step, "step", shape=(M,), dtypes=("int64",))
        chk(self._stats, "stats", shape=(M, self.epochs, 3), dtypes=("float32",))
        L.step, L.stats_out = ptr(self.step), ptr(self._stats)
        if rows is not None:
            L.rows = ptr(chk(rows, "rows", shape=(M, self.epochs, self.batch_size), dtypes=("int64",)))
        if rows_out is not None:
            L.rows_out = ptr(chk(rows_out, "rows_out", shape=(M, self.epochs, self.batch_size), dtypes=("int64",)))
        L.lr, (L.beta1, L.beta2), L.eps = self.lr, self.betas, self.adam_eps
        L.clipping, L.critic_coeff, L.entropy_bonus = self.clipping, self.critic_coeff, self.entropy_bonus
        env.ppo_epochs_members(L, M, self.member_keys, member_hyper=None if self.hyper is None else self.hyper["learner"])
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
