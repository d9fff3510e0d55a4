"""A population of INDEPENDENT Deep-Q agents on one GPU: M runs of the reference's `deep-q`, acting and learning in lockstep.

  BatchedDeepQPopulation   M DeepQAgents over one BatchedGridworldEnv of N = M x E envs; member m owns the envs m * E .. (m + 1) * E - 1.
                           Every parameter, transposed copy, Adam tensor and target tensor exists once per member, stacked on a leading
                           member axis in one contiguous tensor [M, ...]; the replay ring is ONE DeviceReplay over all N envs, member m's
                           transitions its own columns. step() acts for every member in one launch (sgk_policy_rollout_members, one
                           step) and learns in two (sgk_dqn_sgd_step_members: the SGD kernel with one workgroup per member, then Adam
                           over n_members x ceil(P / 256) workgroups). The members differ in their weights, their envs and their
                           draws, as M runs of the reference with different seeds do -- and, with member_hyper, in lr, discount and the
                           starting epsilon (sgk_dqn_sgd_step_members_hyper, sgk_policy_rollout_members_eps): a sweep in the same
                           launches, the values read from device memory. epsilon_anneal and the schedule's shape stay shared.

What member m computes is what a BatchedDeepQAgent(sgd_steps=1, fused_learn=True) computes on a handle of E envs created at
env_index_base + m * E with the handle's seed, member m's weights, member_keys[m] as the key of its minibatch draws and member m's
lr, discount and epsilon in its `args` -- bit for bit (tests/test_gpu_dqn_members.py, tests/test_gpu_member_hyper.py), and through that the reference's own run (tests/golden/batched_dqn_*.npz).

There is no torch path for a population: a shape without a kernel is a ValueError in the constructor.
"""
import ctypes

import torch

from . import _lib
from .deepq_batched import BatchedDeepQAgent, DeviceReplay
from .member_hyper import DQN_NAMES
from .population import Population, default_member_seed  # noqa: F401 (default_member_seed: importable from here as before)
from .population import stack_state_dicts as _stack, unstack_state_dict as _unstack
from .ppo_population import FUSED_CELLS

# BatchedDeepQAgent.Q's parameters (state_dict keys, registration order) and the short names of the stacked tensors
MEMBER_KEYS = ("0.0.weight", "0.0.bias", "1.0.0.weight", "1.0.0.bias", "2.weight", "2.bias")
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")


def stack_state_dicts(state_dicts):
    """population.stack_state_dicts for Q-network state dicts: MEMBER_KEYS under the names PARAMS."""
    return _stack(state_dicts, MEMBER_KEYS, PARAMS)


def unstack_state_dict(stacked, m):
    """Member m's parameters out of stack_state_dicts' tensors, keyed like BatchedDeepQAgent.Q.state_dict() (copies)."""
    return _unstack(stacked, m, MEMBER_KEYS, PARAMS)


class BatchedDeepQPopulation(Population):
    """M independent DeepQAgents over env's N = M x E envs (see the module docstring). ensemble_act() / evaluate_ensemble()
    (ensemble.EnsembleMixin) let the M Q-networks act as one agent on all N envs: every member votes on every env.

    args: the deep-q flags (lr, discount, batch_size, sync_every, epsilon, epsilon_anneal, n_layers, n_hidden, seed). member_seeds:
    member m's initial weights are what BatchedDeepQAgent.build_Q gives on the CPU under torch.manual_seed(member_seeds[m]), Q first,
    then the target, initialised independently as value.py:82-84 does (default: default_member_seed(args.seed, m)); member_keys: the
    Philox key of member m's minibatch draws (default: the seeds). The action draws are keyed by the env's seed and the GLOBAL env
    index, as everywhere. sgd_steps learner calls per lockstep step; reference_loss_broadcast as for BatchedDeepQAgent.

    member_hyper: None (every member runs with args' values, the shared-hyper entry points), or {name: M floats} for names of lr,
    discount, epsilon (the schedule's starting value); the others keep args' value for every member. `member_values` then holds
    {name: [M floats]} on the host and `hyper` the device tensors the kernels read:
      hyper["learner"]   float64 [M, 2], rows of sgk_dqn_member_hyper (lr, discount)
      hyper["epsilon0"]  float64 [M], the starting values;  hyper["epsilon"]  float64 [M], the annealed values of the current step
    The annealed values are computed ON THE DEVICE, once per step(): three elementwise float64 kernels evaluate update_epsilon's
    expression 1.0 - (1 - eps0) * t / anneal for every member in its own order of operations (IEEE double: the host's bits), so
    step() makes no host synchronisation and no host-to-device copy. set_member_hyper copies into these tensors: the kernels and
    any recorded graph keep their addresses.

    exploit_explore (PBTMixin) perturbs lr and discount (the learner row's columns); the three epsilon tensors are cloned only."""

    HYPER_NAMES = DQN_NAMES
    PBT_COLUMNS = DQN_NAMES[:2]
    torch = torch # (the two BatchedDeepQAgent methods borrowed below read self.torch)
    build_Q = BatchedDeepQAgent.build_Q

    def __init__(self, env, args, n_members, member_seeds=None, member_keys=None, replay_slices=8, sgd_steps=1,
                 reference_loss_broadcast=True, member_hyper=None):
        M = self._member_count(env, n_members)
        hidden, layers, batch = int(getattr(args, "n_hidden", 0) or 0), int(args.n_layers), int(args.batch_size)
        if layers != 2:
            raise ValueError("a Deep-Q population needs n_layers = 2 (the fused kernels' topology), not %d" % layers)
        if hidden not in (64, 100):
            raise ValueError("a Deep-Q population needs n_hidden 64 or 100 (sgk_dqn_sgd_step_members), not %d" % hidden)
        if not 1 <= batch <= 64:
            raise ValueError("a Deep-Q population needs 1 <= batch_size <= 64 (sgk_dqn_sgd_step_members), not %d" % batch)
        if env.n_cells not in FUSED_CELLS or env.action_space.n != 4:
            raise ValueError("the fused policy kernel does not cover %s (%d cells, %d actions)" % (env.name, env.n_cells, env.action_space.n))
        self._init_members(env, args, M, member_seeds, member_keys, member_hyper)
        self.n_hidden, self.batch_size, self.sgd_steps = hidden, batch, int(sgd_steps)
        self.discount, self.lr = float(args.discount), float(args.lr)
        self.sync_every = int(args.sync_every)
        self.eps0, self.anneal = float(args.epsilon), int(args.epsilon_anneal)
        self.reference_loss_broadcast = bool(reference_loss_broadcast)
        self.t = 0  # lockstep steps taken == update_epsilon() calls == the RNG draw index
        K0, H, dev = env.n_cells, hidden, self.device
        self.q_body, self.action_n = "mlp", env.action_space.n  # (what build_Q reads)
        q_dicts, t_dicts = [], []
        for s in self.member_seeds:  # (on the CPU: torch.nn.Linear draws its initial weights from the CPU generator)
            torch.manual_seed(s)
            q_dicts.append(self.build_Q(K0, layers, H).state_dict())
            t_dicts.append(self.build_Q(K0, layers, H).state_dict())
        self.cur = {k: v.to(dev) for k, v in stack_state_dicts(q_dicts).items()}
        self.target = {k: v.to(dev) for k, v in stack_state_dicts(t_dicts).items()}
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        # transposed copies: the learner keeps the current network's three current; sync_target_Q / load_member refresh the target's
        self.cur_t = {"w1t": f32(M, K0, H), "w2t": f32(M, H, H), "w3t": f32(M, H, 4)}
        self.target_t = {"w1t": f32(M, K0, H), "w2t": f32(M, H, H)}
        self.adam_m = [torch.zeros_like(self.cur[k]) for k in PARAMS]
        self.adam_v = [torch.zeros_like(self.cur[k]) for k in PARAMS]
        self.adam_vmax = [torch.zeros_like(self.cur[k]) for k in PARAMS]
        self.step_count = torch.zeros(M, dtype=torch.int64, device=dev)
        self.loss = torch.zeros(M, dtype=torch.float32, device=dev)
        self.last_loss = None
        self._L = None  # the learner struct (see _learner)
        self.workspace = torch.zeros(env.dqn_members_workspace_bytes(H, M), dtype=torch.uint8, device=dev)
        self.replay = DeviceReplay(env.n_envs, K0, int(replay_slices), dev)
        self._actions = torch.empty((1, env.n_envs), dtype=torch.uint8, device=dev)
        self._alloc_member_metrics()
        self._refresh_transposes()
        self._refresh_target_transposes()
        self.reset_member_metrics()

    # -- state ---------------------------------------------------------------------------------------------------------------------
    def _refresh_transposes(self):
        self.cur_t["w1t"].copy_(self.cur["w1"].transpose(1, 2))
        self.cur_t["w2t"].copy_(self.cur["w2"].transpose(1, 2))
        self.cur_t["w3t"].copy_(self.cur["w3"].transpose(1, 2))

    def _refresh_target_transposes(self):
        self.target_t["w1t"].copy_(self.target["w1"].transpose(1, 2))
        self.target_t["w2t"].copy_(self.target["w2"].transpose(1, 2))

    def sync_target_Q(self):
        """DeepQAgent.sync_target_Q for every member: target <- Q on the stacked tensors, transposed copies included."""
        for k in PARAMS:
            self.target[k].copy_(self.cur[k])
        self._refresh_target_transposes()

    def tensors(self):
        """Everything the learner reads and updates, by name: the parameters and their transposed copies, Adam's three moments, the
        target network and its transposes, the step counters and the losses. (For snapshots: copy_ into them; the kernels hold their
        addresses.)"""
        out = dict(self.cur)
        out.update(self.cur_t)
        out.update({"m_" + k: t for k, t in zip(PARAMS, self.adam_m)})
        out.update({"v_" + k: t for k, t in zip(PARAMS, self.adam_v)})
        out.update({"vmax_" + k: t for k, t in zip(PARAMS, self.adam_vmax)})
        out.update({"target_" + k: t for k, t in self.target.items()})
        out.update({"target_" + k: t for k, t in self.target_t.items()})
        out["step"] = self.step_count
        out["loss"] = self.loss
        return out

    def pbt_tensors(self):
        """Every per-member tensor the learner or the acting reads or updates: what a clone takes from its source (exploit_explore).
        The epsilon tensors exist with member_hyper only."""
        out = (list(self.cur.values()) + list(self.cur_t.values()) + list(self.target.values()) + list(self.target_t.values())
               + self.adam_m + self.adam_v + self.adam_vmax + [self.step_count])
        if self.hyper is not None:
            out += [self.hyper["epsilon0"], self._one_minus_eps0, self.hyper["epsilon"]]
        return out

    def _pbt_pull_extra(self):
        return self.hyper["epsilon0"]

    def _pbt_after_pull(self, rows, extra):
        self.member_values["lr"], self.member_values["discount"] = [r[0] for r in rows], [r[1] for r in rows]
        self.member_values["epsilon"] = list(extra)
        self._eps_t = None  # (derived from the epsilon tensors: evaluated again at the next step)

    def _alloc_member_hyper(self):
        v, f64 = self.member_values, dict(dtype=torch.float64, device=self.device)
        self.hyper = {"learner": torch.tensor([[v["lr"][m], v["discount"][m]] for m in range(self.n_members)], **f64),
                      "epsilon0": torch.tensor(v["epsilon"], **f64), "epsilon": torch.empty(self.n_members, **f64)}
        self._one_minus_eps0 = torch.tensor([1 - e for e in v["epsilon"]], **f64)  # (the host's own 1 - eps0)
        self._zero_eps = torch.zeros(self.n_members, **f64)
        self._eps_t = None  # the step hyper["epsilon"] holds the values of

    def _store_member_hyper(self, name, vals):
        if name == "epsilon":  # (the schedule's starting value)
            self.hyper["epsilon0"].copy_(torch.tensor(vals, dtype=torch.float64))
            self._one_minus_eps0.copy_(torch.tensor([1 - e for e in vals], dtype=torch.float64))
            self._eps_t = None
        else:
            self.hyper["learner"][:, DQN_NAMES.index(name)].copy_(torch.tensor(vals, dtype=torch.float64))

    def _shared_hyper(self):
        return {"lr": self.lr, "discount": self.discount, "epsilon": self.eps0}

    def member_state(self, m):
        """{"Q": state_dict, "target_Q": state_dict, "hyper": {lr, discount, epsilon}} of member m: the networks under
        BatchedDeepQAgent's key names (copies) and the hyper-parameters of the single agent member m equals."""
        m = self._member_index(m)
        return {"Q": unstack_state_dict(self.cur, m), "target_Q": unstack_state_dict(self.target, m), "hyper": self.member_hyper_of(m)}

    def load_member(self, m, q_state, target_state=None, hyper=None):
        """Member m's Q-network <- a BatchedDeepQAgent.Q state dict; its target network <- target_state, or left alone; its
        hyper-parameters <- hyper ({name: value}; a population with member_hyper only), or left alone."""
        m = self._member_index(m)
        self._load_member_hyper(m, hyper)
        for dst, state in ((self.cur, q_state), (self.target, target_state)):
            if state is None:
                continue
            for key, name in zip(MEMBER_KEYS, PARAMS):
                src = torch.as_tensor(state[key]).to(device=self.device, dtype=torch.float32)
                if tuple(src.shape) != tuple(dst[name][m].shape):
                    raise ValueError("%s has shape %s, expected %s" % (key, tuple(src.shape), tuple(dst[name][m].shape)))
                dst[name][m].copy_(src)
        for k, t in self.cur_t.items():
            t[m].copy_(self.cur[k[:-1]][m].t())
        for k, t in self.target_t.items():
            t[m].copy_(self.target[k[:-1]][m].t())

    # epsilon schedule of DeepQAgent (value.py:70-76,142-146): the members are in lockstep and its shape depends on t alone; shared,
    # or -- with member_hyper -- one starting value per member
    @property
    def epsilon(self):
        """The current epsilon: a float, or with member_hyper the float64 [M] device tensor hyper["epsilon"] (see the class
        docstring: computed on the device, no synchronisation)."""
        t = min(self.t, self.anneal - 1)
        if self.hyper is None:
            return 1.0 - (1 - self.eps0) * t / self.anneal
        eps = self.hyper["epsilon"]
        if self._eps_t != t:  # 1.0 - ((1 - eps0) * t) / anneal, update_epsilon's order of operations, in float64
            torch.mul(self._one_minus_eps0, float(t), out=eps)
            eps.div_(float(self.anneal))
            eps.neg_().add_(1.0)  # (1.0 - x == -x + 1.0 in IEEE arithmetic)
            self._eps_t = t
        return eps

    def update_epsilon(self):
        self.t += 1
        return self.epsilon

    # -- acting --------------------------------------------------------------------------------------------------------------------
    def greedy_weights(self):
        """The stacked Q-networks in the members rollout's layout (the kernels keep w1t / w3t current)."""
        c = self.cur
        return {"w1t": self.cur_t["w1t"], "b1": c["b1"], "w2": c["w2"], "b2": c["b2"], "w3t": self.cur_t["w3t"], "b3": c["b3"]}

    _greedy_weights = _ensemble_weights = greedy_weights  # (evaluate() and EnsembleMixin: the population's own tensors, their addresses stay)

    def _rollout_members(self, weights, n_steps, **kw):
        self.env.policy_rollout_members(weights, self.n_members, n_steps, **kw)

    def warmup(self, n_steps, reference_state=True):
        """dqn_warmup (warmup.py:8-23) for every env of every member: the env-level streamed random rollout, as
        BatchedDeepQAgent.warmup runs it (the ring's columns are the envs, whoever owns them)."""
        return BatchedDeepQAgent.warmup(self, n_steps, reference_state)

    # -- learning ------------------------------------------------------------------------------------------------------------------
    def _learner(self):
        """The filled sgk_dqn_learner addressing member 0 of the stacked tensors, checked and built ONCE (learn_batch runs every lockstep
        step: ~40 tensor checks per call were a tenth of it). It keeps the tensors it points at alive: assigning another tensor to one
        of the attributes does not reach the kernels -- copy_ into them, as tensors() says."""
        if self._L is not None:
            return self._L[0]
        env, M, rp = self.env, self.n_members, self.replay
        chk = env._check  # ValueError for a tensor of the wrong device / dtype / shape: the kernel takes raw pointers
        K0, H, S, n = env.n_cells, self.n_hidden, rp.slices, env.n_envs
        keep = []

        def ptr(t):
            keep.append(t)
            return ctypes.c_void_p(t.data_ptr())

        L = _lib.SgkDqnLearner()
        L.states = ptr(chk(rp.states, "replay states", shape=(S, n, K0), dtypes=("int8",)))
        L.successors = ptr(chk(rp.successors, "replay successors", shape=(S, n, K0), dtypes=("int8",)))
        L.actions = ptr(chk(rp.actions, "replay actions", shape=(S, n), dtypes=("uint8",)))
        L.rewards = ptr(chk(rp.rewards, "replay rewards", shape=(S, n), dtypes=("int8",)))
        L.terminals = ptr(chk(rp.terminals, "replay terminals", shape=(S, n), dtypes=("bool", "uint8")))
        L.n_hidden, L.batch = H, self.batch_size
        L.loss_mode = _lib.DQN_LOSS_REFERENCE if self.reference_loss_broadcast else _lib.DQN_LOSS_PER_SAMPLE
        shapes = {"w1": (M, H, K0), "b1": (M, H), "w2": (M, H, H), "b2": (M, H), "w3": (M, 4, H), "b3": (M, 4)}
        for i, k in enumerate(PARAMS):
            setattr(L, k, ptr(chk(self.cur[k], "parameter " + k, shape=shapes[k], dtypes=("float32",))))
            chk(self.target[k], "target " + k, shape=shapes[k], dtypes=("float32",))
            L.m[i] = ptr(chk(self.adam_m[i], "Adam exp_avg of " + k, shape=shapes[k], dtypes=("float32",))).value
            L.v[i] = ptr(chk(self.adam_v[i], "Adam exp_avg_sq of " + k, shape=shapes[k], dtypes=("float32",))).value
            L.vmax[i] = ptr(chk(self.adam_vmax[i], "Adam max_exp_avg_sq of " + k, shape=shapes[k], dtypes=("float32",))).value
        tshapes = {"w1t": (M, K0, H), "w2t": (M, H, H), "w3t": (M, H, 4)}
        for k, t in self.cur_t.items():
            setattr(L, k, ptr(chk(t, k, shape=tshapes[k], dtypes=("float32",))))
        for k, t in self.target_t.items():
            chk(t, "target " + k, shape=tshapes[k], dtypes=("float32",))
        tg = self.target
        L.tw1t, L.tb1, L.tw2t, L.tb2, L.tw3, L.tb3 = (ptr(self.target_t["w1t"]), ptr(tg["b1"]), ptr(self.target_t["w2t"]), ptr(tg["b2"]),
                                                      ptr(tg["w3"]), ptr(tg["b3"]))
        L.step = ptr(chk(self.step_count, "step", shape=(M,), dtypes=("int64",)))
        L.loss_out = ptr(chk(self.loss, "loss", shape=(M,), dtypes=("float32",)))
        L.lr, L.beta1, L.beta2, L.eps = self.lr, 0.9, 0.999, 1e-8
        L.discount, L.max_grad_norm = self.discount, 10.0
        self._L = (L, keep)
        return L

    def learn_batch(self, rows=None, rows_out=None):
        """DeepQAgent.learn's SGD step (reference value.py:116-134) for every member in one call of sgk_dqn_sgd_step_members: member m's
        minibatch is drawn from its own E columns of the ring with the key member_keys[m]. rows: int64 [M, batch] on the device, global
        transition indices slice * N + env replacing the draws; rows_out: the same shape, receives the indices used. Returns the
        losses, float32 [M] on the device. Nothing allocates or synchronises: the call can be recorded in a graph."""
        L, shape = self._learner(), (self.n_members, self.batch_size)
        L.slices_filled = int(self.replay.filled)
        L.rows = None if rows is None else self.env._check(rows, "rows", shape=shape, dtypes=("int64",)).data_ptr()
        L.rows_out = None if rows_out is None else self.env._check(rows_out, "rows_out", shape=shape, dtypes=("int64",)).data_ptr()
        self.env.dqn_sgd_step_members(L, self.n_members, self.member_keys, self.workspace,
                                      member_hyper=None if self.hyper is None else self.hyper["learner"])
        self.last_loss = self.loss
        return self.loss

    def step(self, learn=True, cheat=False, explore=True):
        """One lockstep iteration of dqn_learn for every member: act_explore -> env.step -> replay.add -> learn -> update_epsilon ->
        (sync target) -> reset finished envs (the episode loop of train.py:62-70). Returns the actions, uint8 [N]."""
        env, rp = self.env, self.replay
        if learn and not rp.states_ready(env):
            rp.store(env, 0)  # the boards the agents act on are the transitions' states (already there when the previous step left them)
        # one step of the members rollout = sgk_policy_act + sgk_step for every member's envs, each with its own Q-network
        if self.hyper is None:
            eps, member_eps = (self.epsilon if explore else 0.0), None
        else:
            eps, member_eps = 0.0, (self.epsilon if explore else self._zero_eps)
        env.policy_rollout_members(self.greedy_weights(), self.n_members, 1, mode="greedy", epsilon=eps,
                                   draw_index0=self.t, auto_reset=not learn, actions=self._actions,
                                   member_metrics=self.member_metrics, member_epsilon=member_eps)
        actions = self._actions[0]
        if learn:
            rp.store(env, 1, actions=actions, cheat=cheat)  # the rest of the add: successor boards, action, reward, terminal
            for _ in range(self.sgd_steps):
                self.learn_batch()
        t = self.t
        self.update_epsilon()
        if learn and t % self.sync_every == self.sync_every - 1:
            self.sync_target_Q()
        if learn:
            rp.reset_store(env)  # reset_done + the NEXT transition's states in one launch
        return actions
