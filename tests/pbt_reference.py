"""The numpy reference of the exploit / explore step (include/sgk.h: sgk_members_select), written from the header's contract and from
nothing else: a stable sort for the order, the oracle's own Philox for the coins. tests/test_pbt_abi.py checks it against hand-written
cases; the library's host and device code is then compared with it, exactly."""
import numpy as np

from oracle import oracle as O

STREAM_EXPLORE = 7


def order(scores):
    """The members from best to worst: NaN counts as -inf; by score, descending; equal scores (-0.0 == 0.0 among them) by index."""
    s = np.asarray(scores, dtype=np.float64).copy()
    s[np.isnan(s)] = -np.inf
    return sorted(range(len(s)), key=lambda m: (-s[m], m))  # (tuples compare with ==: -0.0 and 0.0 tie, and the index decides)


def select(scores, n_replace):
    """src int32 [M]: src[order[M - 1 - i]] = order[i] for i < n_replace, src[m] = m for every other member."""
    o = order(scores)
    M = len(o)
    src = np.arange(M, dtype=np.int32)
    for i in range(int(n_replace)):
        src[o[M - 1 - i]] = o[i]
    return src


def explore_pick(key, generation, member, column):
    """x[0] & 1 of philox4x32_10(ctr = {member, column, (uint32)generation, 7}, key = {key_lo, key_hi})."""
    key, generation = int(key) & (2 ** 64 - 1), int(generation) & (2 ** 64 - 1)
    x = O.philox4x32_10([int(member), int(column), generation & 0xFFFFFFFF, STREAM_EXPLORE], [key & 0xFFFFFFFF, key >> 32])
    return int(x[0]) & 1


def explore(hyper, src, mask, factors, lo, hi, key, generation):
    """The hyper tensor [M, C] after the explore step (a float64 copy): rows of the replaced members only."""
    out = np.array(hyper, dtype=np.float64, copy=True)
    M, C = out.shape
    for d in range(M):
        s = int(src[d])
        if s == d:
            continue
        for k in range(C):
            v = np.float64(hyper[s][k])
            if (int(mask) >> k) & 1:
                f = np.float64(factors[1] if explore_pick(key, generation, d, k) else factors[0])
                v = v * f  # one IEEE double multiply
                v = np.float64(lo[k]) if v < lo[k] else v
                v = np.float64(hi[k]) if v > hi[k] else v
            out[d][k] = v
    return out


SCORE_SETS = {}


def score_sets():
    """name -> float64 scores, the cases of both test files: seeded random, all-equal, NaN / inf / signed zeros, and the sizes 1, 2, 5
    (odd: the middle member is untouched), 1025 and 4096 (a lane of the kernel ranks more than one member)."""
    if not SCORE_SETS:
        rng = np.random.default_rng(20261019)
        SCORE_SETS["random_37"] = rng.normal(size=37)
        SCORE_SETS["equal_12"] = np.full(12, 3.5)
        SCORE_SETS["special_11"] = np.array([0.0, np.nan, -0.0, np.inf, -np.inf, 1.0, np.nan, 0.0, -1.0, np.inf, -0.0])
        SCORE_SETS["one"] = np.array([2.0])
        SCORE_SETS["two"] = np.array([1.0, 2.0])
        SCORE_SETS["five"] = np.array([0.5, -1.0, 4.0, 4.0, 0.25])
        SCORE_SETS["random_1025"] = np.round(rng.normal(size=1025), 1)  # (rounded: plenty of ties)
        SCORE_SETS["random_4096"] = np.round(rng.normal(size=4096), 2)
    return SCORE_SETS
