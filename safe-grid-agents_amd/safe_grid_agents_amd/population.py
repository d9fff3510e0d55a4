"""What the three populations (BatchedPPOPopulation, BatchedPPOCNNPopulation, BatchedDeepQPopulation) share: the members' seeds and
keys, stacking state dicts on a leading member axis, the per-member metrics, the greedy evaluation and the host side of the per-member
hyper-parameters. A population module adds its tensors, its kernels' calls and where a hyper-parameter lands on the device.
"""
import torch

from . import _lib
from .ensemble import EnsembleMixin
from .member_hyper import resolve, validate_values
from .metering import BatchMetrics
from .pbt import PBTMixin

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


def stack_state_dicts(state_dicts, keys, names):
    """State dicts (their entries `keys`; anything else, e.g. old_policy.*, is ignored) -> {short name: tensor [M, ...]} in the order
    of `names`, one contiguous tensor per parameter. Pure torch; the values are copied bit for bit."""
    if not state_dicts:
        raise ValueError("no members to stack")
    out = {}
    for key, name in zip(keys, names):
        parts = [torch.as_tensor(sd[key]).detach().to(torch.float32) for sd in state_dicts]
        if any(p.shape != parts[0].shape for p in parts):
            raise ValueError("members disagree on the shape of %s" % key)
        out[name] = torch.stack(parts).contiguous()
    return out


def unstack_state_dict(stacked, m, keys, names):
    """Member m's parameters out of stack_state_dicts' tensors, keyed by `keys` like the member's own state_dict() (copies)."""
    return {key: stacked[name][m].detach().clone() for key, name in zip(keys, names)}


def _as_i64(values):
    """uint64 values as the int64 bit patterns a torch tensor can hold."""
    return [v - 2 ** 64 if v >= 2 ** 63 else v for v in (int(x) & _MASK for x in values)]


class Population(EnsembleMixin, PBTMixin):
    """The base of the three populations: M members over env's N = M x E envs, member m owning the envs m * E .. (m + 1) * E - 1.

    A subclass's constructor calls _member_count() (the first refusal), makes its own shape refusals, then _init_members() -- the last
    step that needs no device and the first that does -- and _alloc_member_metrics() where its allocations have their place. It supplies
      _rollout_members(weights, n_steps, **kw)   its members-rollout call (the env's policy_ / convq_rollout_members)
      _greedy_weights()                          the members' current weights in that call's layout
    and, for the per-member hyper-parameters (HYPER_NAMES; `member_values` {name: [M floats]} on the host, `hyper` the device tensors
    the kernels read -- both None for a population built without member_hyper, which calls the shared-hyper entry points),
      _alloc_member_hyper()                      `hyper` from `member_values`
      _store_member_hyper(name, vals)            where a value lands on the device: copied INTO the tensors
      _shared_hyper()                            {name: the shared value} of a population without member_hyper."""

    HYPER_NAMES = ()
    hyper = None
    member_values = None

    # -- construction --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _member_count(env, n_members):
        M = int(n_members)
        if M < 1 or env.n_envs % M:
            raise ValueError("n_envs (%d) is not a multiple of n_members (%d): every member owns the same number of envs" % (env.n_envs, M))
        return M

    def _init_members(self, env, args, M, member_seeds, member_keys, member_hyper):
        """member_hyper's validation (no device: ValueError for an unknown name, a wrong length, an invalid value), then the members'
        bookkeeping: env, n_members, member_envs, device, member_seeds, the member_keys tensor and the hyper tensors."""
        if member_hyper is not None:
            self.member_values = resolve(member_hyper, self.HYPER_NAMES, {k: float(getattr(args, k)) for k in self.HYPER_NAMES}, M)
        self.env, self.n_members, self.member_envs = env, M, env.n_envs // M
        self.device = "cuda:%d" % env.device
        seed = int(getattr(args, "seed", 0) or 0)
        self.member_seeds = [int(s) & _MASK for s in (member_seeds if member_seeds is not None
                                                      else [default_member_seed(seed, m) for m in range(M)])]
        keys = self.member_seeds if member_keys is None else [int(k) & _MASK for k in member_keys]
        if len(self.member_seeds) != M or len(keys) != M:
            raise ValueError("member_seeds / member_keys need one entry per member (%d)" % M)
        self.member_keys = torch.tensor(_as_i64(keys), dtype=torch.int64, device=self.device)
        if self.member_values is not None:
            self._alloc_member_hyper()

    def _alloc_member_metrics(self):
        self.member_metrics = torch.empty((self.n_members, _lib.METRICS_LEN), dtype=torch.int64, device=self.device)
        self._metrics_init = torch.zeros(_lib.METRICS_LEN, dtype=torch.int64)
        self._metrics_init[_lib.M_MAX_RETURN:_lib.M_MAX_MARGIN_POS + 1] = _INT64_MIN
        self._metrics_init = self._metrics_init.to(self.device)

    def _member_index(self, m):
        m = int(m)
        if not 0 <= m < self.n_members:
            raise IndexError("member %d of %d" % (m, self.n_members))
        return m

    # -- metrics -------------------------------------------------------------------------------------------------------------------
    def reset_member_metrics(self):
        self.member_metrics.copy_(self._metrics_init.unsqueeze(0).expand_as(self.member_metrics))

    def member_batch_metrics(self):
        """One BatchMetrics per member from the per-member vectors (one read-back)."""
        vecs = self.member_metrics.cpu().numpy()
        return [BatchMetrics(v, self.env.reward_scale) for v in vecs]

    def evaluate(self, eval_timesteps):
        """batched_default_eval (reference eval.py:8-56) for every member's CURRENT network, greedy: its two phases as two launches of
        the members rollout. Returns (per-member BatchMetrics, the aggregate BatchMetrics); both metrics are reset first."""
        env = self.env
        env.metrics_reset()
        self.reset_member_metrics()
        env.reset()
        w = self._greedy_weights()
        if int(eval_timesteps) > 1:
            self._rollout_members(w, int(eval_timesteps) - 1, mode="greedy", epsilon=0.0, auto_reset=True, member_metrics=self.member_metrics)
        self._rollout_members(w, int(env.info.max_iterations), mode="greedy", epsilon=0.0, auto_reset=False, member_metrics=self.member_metrics)
        return self.member_batch_metrics(), BatchMetrics(env.metrics(), env.reward_scale)

    # -- per-member hyper-parameters -----------------------------------------------------------------------------------------------
    def _need_member_hyper(self, name=None):
        if self.hyper is None:
            raise ValueError("this population was built without member_hyper: its hyper-parameters are shared")
        if name is not None and name not in self.HYPER_NAMES:
            raise ValueError("member_hyper has no %r here: the names are %s" % (name, ", ".join(self.HYPER_NAMES)))

    def set_member_hyper(self, name, values):
        """Member m's `name` <- values[m] (validated: ValueError), copied INTO the device tensors (no new allocation): the next launch
        that reads them -- a replay of a recorded one included -- runs with the new values. A population built without member_hyper has
        no per-member tensors: ValueError."""
        self._need_member_hyper(name)
        vals = validate_values(name, values, self.n_members)
        self.member_values[name] = vals
        self._store_member_hyper(name, vals)

    def member_hyper_of(self, m):
        """{name: member m's value} for all of HYPER_NAMES (the shared values without member_hyper): what the `args` of the single agent
        that member m equals carry."""
        m = self._member_index(m)
        self._pull_if_dirty()
        if self.member_values is None:
            return self._shared_hyper()
        return {k: self.member_values[k][m] for k in self.HYPER_NAMES}

    def _load_member_hyper(self, m, hyper):
        """load_member's `hyper`: {name: value} for member m alone, or None: left alone."""
        if hyper is None:
            return
        self._need_member_hyper()
        self._pull_if_dirty()
        for name, value in dict(hyper).items():
            self._need_member_hyper(name)
            vals = list(self.member_values[name])
            vals[m] = value
            self.set_member_hyper(name, vals)
