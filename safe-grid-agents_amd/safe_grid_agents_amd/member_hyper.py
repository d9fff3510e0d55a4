"""Per-member hyper-parameters of the populations: a sweep in one launch.

Member m of a BatchedPPOPopulation / BatchedPPOCNNPopulation / BatchedDeepQPopulation can learn and act with its own lr, clipping,
critic_coeff, entropy_bonus, discount (PPO) or lr, discount, epsilon (Deep-Q). The values live in device memory in the layouts of
include/sgk.h (sgk_ppo_member_hyper, sgk_dqn_member_hyper, one double per member for epsilon, one float32 row of discount powers per
member for the PPO returns); the kernels read them when they run, so nothing is re-recorded or re-launched per value.

This module is the host side that needs no device: the names, the validation (ValueError), and the `--sweep NAME=v1,v2,...` grammar of
the command line (SystemExit with the valid names).
"""
import itertools
import math

# the names a population takes, in the order of the device struct's fields (then the ones that live elsewhere)
PPO_NAMES = ("lr", "clipping", "critic_coeff", "entropy_bonus", "discount")
DQN_NAMES = ("lr", "discount", "epsilon")
# command-line agent alias -> the names --sweep accepts (the flag spelling uses '-', the name '_'; both are taken)
SWEEP_NAMES = {"ppo-mlp": PPO_NAMES, "ppo-cnn": PPO_NAMES, "deep-q": DQN_NAMES}


def validate_values(name, values, n_members):
    """`values` as a list of n_members floats that `name` may take: finite; lr > 0; 0 <= epsilon <= 1; 0 < discount <= 1.
    ValueError otherwise (the library does not look into device memory: this is the check)."""
    try:
        vals = [float(v) for v in values]
    except (TypeError, ValueError):
        raise ValueError("member_hyper[%r] must be a sequence of %d floats" % (name, n_members)) from None
    if len(vals) != n_members:
        raise ValueError("member_hyper[%r] has %d values, the population %d members" % (name, len(vals), n_members))
    for m, v in enumerate(vals):
        if not math.isfinite(v):
            raise ValueError("member_hyper[%r][%d] = %r is not finite" % (name, m, v))
        if name == "lr" and not v > 0.0:
            raise ValueError("member_hyper['lr'][%d] = %r: lr must be > 0" % (m, v))
        if name == "epsilon" and not 0.0 <= v <= 1.0:
            raise ValueError("member_hyper['epsilon'][%d] = %r: epsilon must be in [0, 1]" % (m, v))
        if name == "discount" and not 0.0 < v <= 1.0:
            raise ValueError("member_hyper['discount'][%d] = %r: discount must be in (0, 1]" % (m, v))
    return vals


def resolve(member_hyper, names, defaults, n_members):
    """{name: [n_members floats]} for every name of `names`: the validated entry of member_hyper, or the shared default for the names
    it does not give. ValueError for a name outside `names`, a wrong length or an invalid value."""
    try:
        given = dict(member_hyper)
    except (TypeError, ValueError):
        raise ValueError("member_hyper must map a name of %s to a sequence of %d floats" % (list(names), n_members)) from None
    unknown = [k for k in given if k not in names]
    if unknown:
        raise ValueError("member_hyper has no %s here: the names are %s" % (", ".join(repr(k) for k in unknown), ", ".join(names)))
    return {k: validate_values(k, given[k], n_members) if k in given else [float(defaults[k])] * n_members for k in names}


def annealed_epsilon(eps0, t, anneal):
    """DeepQAgent's schedule (value.py:70-76,142-146) for one starting value, the expression of update_epsilon."""
    t = min(int(t), int(anneal) - 1)
    return 1.0 - (1 - eps0) * t / anneal


# -- the command line ---------------------------------------------------------------------------------------------------------------
def parse_sweep(specs, agent_alias, members):
    """`--sweep NAME=v1,v2,...` flags (in the order given) -> (names, grid): grid is the Cartesian product, first flag slowest, a list
    of G tuples. SystemExit with the valid names for a sweep without --members, an agent without sweepable names, a name the agent
    does not have, a name given twice, a missing '=', an empty list or a value that is no float; SystemExit naming G when `members` is
    no multiple of G."""
    valid = SWEEP_NAMES.get(agent_alias)
    if valid is None:
        raise SystemExit("--sweep runs on a population of ppo-mlp, ppo-cnn or deep-q agents, not %r" % (agent_alias,))
    listing = "the names %s can sweep are %s" % (agent_alias, ", ".join(valid))
    if not int(members or 0):
        raise SystemExit("--sweep needs --members M (M a multiple of the number of grid points); " + listing)
    names, axes = [], []
    for spec in specs:
        name, eq, rest = str(spec).partition("=")
        name = name.strip().replace("-", "_")
        if not eq or name not in valid:
            raise SystemExit("--sweep %s: expected NAME=v1,v2,...; %s" % (spec, listing))
        if name in names:
            raise SystemExit("--sweep %s: %s is swept twice; %s" % (spec, name, listing))
        items = [v.strip() for v in rest.split(",")]
        if not rest.strip() or any(not v for v in items):
            raise SystemExit("--sweep %s: an empty list of values; %s" % (spec, listing))
        try:
            values = [float(v) for v in items]
        except ValueError:
            raise SystemExit("--sweep %s: the values must be floats; %s" % (spec, listing)) from None
        names.append(name)
        axes.append(values)
    grid = list(itertools.product(*axes))
    if int(members) % len(grid):
        raise SystemExit("--sweep spans G = %d grid points; --members %d is no multiple of G = %d" % (len(grid), int(members), len(grid)))
    return names, grid


def sweep_member_hyper(names, grid, members):
    """The populations' member_hyper for a grid: member m runs point m % G and is replica m // G of it."""
    G = len(grid)
    return {name: [grid[m % G][i] for m in range(int(members))] for i, name in enumerate(names)}


def point_label(names, point):
    return " ".join("%s=%g" % (n, v) for n, v in zip(names, point))


def sweep_table(names, grid, per_member_returns, per_member_safeties):
    """The lines of the end-of-run table: one per grid point, mean +- std (population std) of the replicas' return and safety."""
    import numpy as np

    G, lines = len(grid), []
    for g, point in enumerate(grid):
        r = np.asarray(per_member_returns[g::G], dtype=np.float64)
        s = np.asarray(per_member_safeties[g::G], dtype=np.float64)
        lines.append("%-40s return %10.4f +- %-10.4f safety %10.4f +- %-10.4f (%d replica%s)" % (
            point_label(names, point), r.mean(), r.std(), s.mean(), s.std(), len(r), "" if len(r) == 1 else "s"))
    return lines
