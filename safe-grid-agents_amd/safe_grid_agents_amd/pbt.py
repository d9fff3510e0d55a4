"""Population-based training on the device: the exploit / explore step of the three populations.

Every K iterations the worst members of a population become copies of the best ones, with their hyper-parameters nudged (Jaderberg et
al. 2017, "Population Based Training of Neural Networks"). A population here already keeps every member's weights, Adam state and
old / target policy stacked on a leading member axis and its hyper-parameters in device tensors the kernels read when they run, so the
step is two kinds of launch (include/sgk.h):

  sgk_members_select   one workgroup ranks the members by their scores, names every member's source (src[d] = s for the replaced, src[m]
                       = m for the rest) and writes the replaced members' hyper rows: the source's, the perturbed columns multiplied by
                       factor_down or factor_up on a Philox coin and clamped to their bounds
  sgk_members_clone    one launch per 64 stacked tensors copies the sources' slabs over the replaced members'

PBTMixin.exploit_explore() is that step; a population supplies pbt_tensors(), the list of its per-member tensors. Nothing synchronises
and nothing is read back: the host mirror `member_values` goes stale and is pulled (pull_member_hyper, one read-back) when it is next
asked for. A clone keeps its own member_keys / member_seeds and its own envs, so it diverges from its parent; metrics, stats, losses,
workspaces and the replay ring are not cloned.

This module also holds the command line's side: the --pbt-* flags' grammar (parse_pbt: SystemExit with a plain message).
"""
from . import _lib

DEFAULT_FACTORS = (0.8, 1.2)
_BIG = 1e6  # the "no upper bound" of the default bounds: large and finite
# the default bounds keep a perturbed value valid under member_hyper.validate_values
DEFAULT_BOUNDS = {"lr": (1e-8, 1e3), "discount": (1e-8, 1.0), "clipping": (0.0, _BIG), "critic_coeff": (0.0, _BIG),
                  "entropy_bonus": (0.0, _BIG)}
# command-line agent alias -> the names --pbt-perturb accepts: the columns of the learner's device rows
PERTURB_NAMES = {"ppo-mlp": _lib.PPO_MEMBER_HYPER_FIELDS, "ppo-cnn": _lib.PPO_MEMBER_HYPER_FIELDS, "deep-q": _lib.DQN_MEMBER_HYPER_FIELDS}


def tensor_descs(tensors, n_members):
    """A ctypes array of sgk_members_tensor for tensors stacked [n_members, ...] (contiguous; a slab of a multiple of 4 bytes).
    ValueError for a tensor that is not. The array does not keep the tensors alive: the caller does."""
    descs = (_lib.SgkMembersTensor * len(tensors))()
    for i, t in enumerate(tensors):
        if t.dim() < 1 or int(t.shape[0]) != int(n_members) or not t.is_contiguous():
            raise ValueError("a per-member tensor must be contiguous with the members on its first axis (%d), not %s" % (n_members, tuple(t.shape)))
        nbytes = (t.numel() // int(n_members)) * t.element_size()
        if nbytes % 4 or t.data_ptr() % 4:
            raise ValueError("a member's slab must be 4-byte aligned and a multiple of 4 bytes (shape %s, %s)" % (tuple(t.shape), t.dtype))
        descs[i].base, descs[i].bytes_per_member = t.data_ptr(), nbytes
    return descs


class PBTMixin:
    """exploit_explore() / pull_member_hyper() for a population with `hyper["learner"]` (float64 [M, C] rows of PBT_COLUMNS),
    `member_values`, `member_metrics`, `env`, `n_members`, `device`, `member_seeds` and a pbt_tensors() method.

      pbt_src         int32 [M] on the device: after a call, the member each member has become (itself, unless it was replaced)
      pbt_status      int32 [1] on the device: non-zero when a clone was refused (pull_member_hyper raises)
      pbt_generation  int64 [1] on the device: the explore step's draw counter, advanced by the kernel (a replayed graph draws anew)
      pbt_key         the Philox key of the explore step's coins (default: member 0's seed)"""

    PBT_COLUMNS = ()  # the names of hyper["learner"]'s columns: the values exploit_explore can perturb
    pbt_src = pbt_status = pbt_generation = pbt_key = None
    _hyper_dirty = False
    _pbt_descs = None

    def pbt_tensors(self):
        raise NotImplementedError

    def _pbt_hyper_tensors(self):
        """The hyper tensors beside the learner rows that a clone takes from its source unchanged."""
        return []

    def _pbt_after_pull(self, rows, extra):
        """member_values <- what pull_member_hyper read: rows [M][C] of the learner tensor, extra: _pbt_pull_extra()'s values."""

    def _pbt_pull_extra(self):
        """A float64 [M] tensor read back with the learner rows (the cloned-only value), or None."""
        return None

    def _pbt_state(self):
        import torch

        if self.pbt_src is None:
            self.pbt_src = torch.arange(self.n_members, dtype=torch.int32, device=self.device)
            self.pbt_status = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.pbt_generation = torch.zeros(1, dtype=torch.int64, device=self.device)
            if self.pbt_key is None:
                self.pbt_key = int(self.member_seeds[0])

    def default_scores(self):
        """The members' mean return of member_metrics, float64 [M] on the device: sum_return / episodes, -inf for a member that
        finished no episode. Torch ops on the device; no read-back."""
        import torch

        mm = self.member_metrics
        episodes = mm[:, _lib.M_EPISODES]
        mean = mm[:, _lib.M_SUM_RETURN].to(torch.float64) / episodes.to(torch.float64)
        return torch.where(episodes > 0, mean, torch.full_like(mean, float("-inf")))

    def exploit_explore(self, scores=None, fraction=0.25, perturb=("lr",), factors=DEFAULT_FACTORS, bounds=None):
        """One exploit / explore step: the int(fraction * M) worst members by `scores` (float64 [M] on the device, higher is better;
        default: default_scores()) become copies of the best ones -- every tensor of pbt_tensors() and the hyper tensors -- and the
        columns named in `perturb` (of PBT_COLUMNS) of their hyper rows are the source's times factors[0] or factors[1] (a Philox coin per
        member and column), clamped to bounds[name] = (lo, hi) (default: DEFAULT_BOUNDS). One sgk_members_select call and one
        sgk_members_clone call per 64 tensors; nothing allocates (given scores), synchronises or is read back, so the call can be
        recorded in a graph. Needs a population built with member_hyper (ValueError)."""
        if self.hyper is None:
            raise ValueError("this population was built without member_hyper: its hyper-parameters are shared")
        M, cols = self.n_members, self.PBT_COLUMNS
        fraction = float(fraction)
        if not 0.0 <= fraction <= 0.5:
            raise ValueError("fraction must be in [0, 0.5] (the replaced members and their sources are disjoint), not %r" % (fraction,))
        perturb = (perturb,) if isinstance(perturb, str) else tuple(perturb)
        unknown = [p for p in perturb if p not in cols]
        if unknown:
            raise ValueError("exploit_explore cannot perturb %s here: the names are %s" % (", ".join(repr(p) for p in unknown), ", ".join(cols)))
        try:
            down, up = (float(f) for f in factors)
        except (TypeError, ValueError):
            raise ValueError("factors must be two positive floats (down, up), not %r" % (factors,)) from None
        limits = dict(DEFAULT_BOUNDS)
        for name, pair in dict(bounds or {}).items():
            if name not in cols:
                raise ValueError("bounds names %r; the names are %s" % (name, ", ".join(cols)))
            limits[name] = (float(pair[0]), float(pair[1]))
        self._pbt_state()
        if scores is None:
            scores = self.default_scores()
        ex = _lib.SgkMembersExplore()
        ex.hyper_dev, ex.n_columns = self.hyper["learner"].data_ptr(), len(cols)
        ex.perturb_mask = sum(1 << cols.index(p) for p in set(perturb))
        ex.factor_down, ex.factor_up = down, up
        for k, name in enumerate(cols):
            ex.lo[k], ex.hi[k] = limits[name]
        ex.key, ex.generation_dev = int(self.pbt_key) & (2 ** 64 - 1), self.pbt_generation.data_ptr()
        tensors = list(self.pbt_tensors()) + list(self._pbt_hyper_tensors())
        addresses = tuple(t.data_ptr() for t in tensors)
        if self._pbt_descs is None or self._pbt_descs[0] != addresses:
            self._pbt_descs = (addresses, tensor_descs(tensors, M), tensors)
        self._hyper_dirty = True
        self.env.members_select(scores, int(fraction * M), self.pbt_src, explore=ex)  # (SgkError for what the library refuses)
        self.env.members_clone(self.pbt_src, self._pbt_descs[1], self.pbt_status)

    def pull_member_hyper(self):
        """member_values <- the device's hyper tensors, in ONE read-back (after exploit_explore the host mirror is stale;
        member_hyper_of, member, member_state call this first when it is). RuntimeError when pbt_status says a clone was refused."""
        import torch

        if self.hyper is None:
            raise ValueError("this population was built without member_hyper: its hyper-parameters are shared")
        self._pbt_state()
        M, C = self.n_members, len(self.PBT_COLUMNS)
        parts = [self.hyper["learner"].reshape(-1), self.pbt_status.to(torch.float64)]
        extra = self._pbt_pull_extra()
        if extra is not None:
            parts.append(extra.reshape(-1))
        host = torch.cat(parts).cpu().tolist()
        if host[M * C] != 0.0:
            raise RuntimeError("sgk_members_clone refused a source (pbt_status = %d): pbt_src is no fixed-point map of the members"
                               % int(host[M * C]))
        rows = [host[m * C:(m + 1) * C] for m in range(M)]
        self._pbt_after_pull(rows, host[M * C + 1:] if extra is not None else None)
        self._hyper_dirty = False

    def _pull_if_dirty(self):
        if self._hyper_dirty:
            self.pull_member_hyper()


# -- the command line ---------------------------------------------------------------------------------------------------------------
def parse_pbt(args):
    """The --pbt-* flags of `args` -> {"every", "fraction", "factors", "perturb"} or None without --pbt-every. SystemExit with a plain
    message for --pbt-every without --members, an agent without a population, a fraction outside [0, 0.5], factors that are not two
    positive floats and a name the agent's learner row does not have."""
    every = int(getattr(args, "pbt_every", 0) or 0)
    if not every:
        return None
    if every < 0:
        raise SystemExit("--pbt-every must be >= 1")
    valid = PERTURB_NAMES.get(args.agent_alias)
    if valid is None:
        raise SystemExit("--pbt-every runs on a population of ppo-mlp, ppo-cnn or deep-q agents, not %r" % (args.agent_alias,))
    if not int(getattr(args, "members", 0) or 0):
        raise SystemExit("--pbt-every needs --members M: population-based training replaces the worst members by the best")
    fraction = getattr(args, "pbt_fraction", None)
    fraction = 0.25 if fraction is None else float(fraction)
    if not 0.0 <= fraction <= 0.5:
        raise SystemExit("--pbt-fraction must be in [0, 0.5], not %r" % (fraction,))
    spec = getattr(args, "pbt_factors", None)
    factors = DEFAULT_FACTORS
    if spec is not None:
        try:
            factors = tuple(float(v) for v in str(spec).split(","))
        except ValueError:
            factors = ()
        if len(factors) != 2 or not all(0.0 < f < float("inf") for f in factors):
            raise SystemExit("--pbt-factors %s: expected two positive floats down,up (default 0.8,1.2)" % (spec,))
    spec = getattr(args, "pbt_perturb", None)
    perturb = ("lr",)
    if spec is not None:
        perturb = tuple(v.strip().replace("-", "_") for v in str(spec).split(","))
        for name in perturb:
            if name not in valid:
                raise SystemExit("--pbt-perturb %s: the names %s can perturb are %s" % (spec, args.agent_alias, ", ".join(valid)))
    return {"every": every, "fraction": fraction, "factors": factors, "perturb": perturb}
