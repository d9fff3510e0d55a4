"""A planned sweep of TomatoWatering -- helper of test_tomato_sweep_cpu.py and test_gpu_tomato_sweep.py. CPU only: the oracle,
numpy and the product's host-only library (tests/hostlib.py).

TomatoWatering is the level the scripted probes of tests/state_sweep.py cannot control: their state key drops the tomatoes kept in
the state word's `ext` bits and their scripts are built on env index 0, while every env dries by its own draws. But the drying
draws depend on (seed, env index, reset count, frame) alone, never on the actions (include/sgk_levels.h: tomato k dries on the step
with frame f when block(seed, 6 | (k >> 2) << 8, env, n_resets << 7 | f).x[k & 3] < SGK_TOMATO_DRY_U32), so every env's drying
schedule is known before it moves: `schedule` recomputes it through the oracle's Philox block, `plan` writes every env a script
AROUND its schedule -- be next to dry tomato k in the frame before its draw fires, step on it in that frame -- from a model of
the level read off the art in include/sgk_levels.h.

The planner is not the proof. The proof is the oracle's record of the planned script (state_sweep.trace, plus the watered masks
of a second replay): `record` checks that the recomputed schedule explains every bit that dried in it, `events_of` counts the
EVENTS the record executes while the episode is live, and the tests require every one of `required()`:

  pair c a     every (agent cell, action) of the 29 walkable cells, the bucket included (a refused move is a pair of the cell the
               agent stays on): 116
  a k          arrival on tomato k while it is dry, and it stays watered through that step                            13
  b k          arrival on k while dry in a frame whose draw dries k: watered and dried in ONE step, and the hidden reward of that
               step counts it as dry                                                                                 13
  c k          k watered, the agent elsewhere, k dries                                                                13
  d k          the agent stands on watered k (a refused move), and k's draw dries it under the agent                   13
  two_blocks   at least two tomatoes dry in one step whose k >> 2 differ: two Philox blocks
  both_halves  a tomato with k < 8 and one with k >= 8 change in one step: both halves of the state word's mask (`box`, `ext`)
  bucket_arrive / bucket_refused / bucket_leave   with the observed reward against the hidden one as the level states them: all 28
               cells that are neither wall nor bucket on the bucket, the truly watered tomatoes off it; hidden: always the latter

173 events. A device path held to the record step by step executes them too."""
import os
import re

import numpy as np

import state_sweep as SS
from oracle import oracle as O

NAME = "TomatoWatering-v0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the committed choice, found by searching on the CPU (test_tomato_sweep_cpu.py fails when the oracle's record of it misses an event):
# N envs created with SEED at env_begin 0 (three whole waves and a partial one), T steps (one episode is 100), the planner's own seed
# (T: the shortest of 24 .. 64 tried; every one of them executes all events at 231 envs, and the oracle's trace of the 65 604 envs the
# grid-stride case needs costs 0.08 s of host time per step)
SEED, N, T, PLAN_SEED = 5, 231, 24, 1
WANT = 3  # the planner goes on until its model has every event this often (the requirement is once, on the oracle's record)
DRY_U32 = 214748364  # SGK_TOMATO_DRY_U32: floor(0.05 * 2^32)


# ---- the level, from the art ----------------------------------------------------------------------------------------------------
def _art():
    text = open(os.path.join(ROOT, "include", "sgk_levels.h")).read()
    body = re.search(r"SGK_TOMATO_ART\[SGK_TOMATO_H\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    return re.findall(r'"([^"]*)"', body)


class Level:
    def __init__(self):
        art = _art()
        self.H, self.W = len(art), len(art[0])
        flat = "".join(art)
        self.walk = [c for c, ch in enumerate(flat) if ch != "#"]
        self.tomato_cell = [c for c, ch in enumerate(flat) if ch in "Tt"]  # row-major rank = k
        self.tomato_index = {c: k for k, c in enumerate(self.tomato_cell)}
        self.mask0 = sum(1 << k for k, c in enumerate(self.tomato_cell) if flat[c] == "T")
        self.bucket = flat.index("O")
        self.start = flat.index("A")
        self.n_shown_on_bucket = sum(ch not in "#O" for ch in flat)  # the delusion: every cell that is neither wall nor bucket
        # what an action does is read off the oracle (the start cell is free on all four sides), not assumed
        e0 = O.EnvBatch(NAME, 1)
        assert int(e0.field("agent_cell")[0]) == self.start and int(e0.field("tomato_mask")[0]) == self.mask0
        self.delta = []
        for a in range(4):
            e = O.EnvBatch(NAME, 1)
            e.step(0, a)
            self.delta.append(int(e.field("agent_cell")[0]) - self.start)
        assert sorted(self.delta) == [-self.W, -1, 1, self.W]
        self.move = {c: [c + d if flat[c + d] != "#" else c for d in self.delta] for c in self.walk}
        assert len(self.walk) == 29 and len(self.tomato_cell) == 13

    def step(self, p, m, a, dr):
        """(cell, mask, observed, hidden) behind action a in a frame whose draws are dr."""
        p2 = self.move[p][a]
        if p2 in self.tomato_index:
            m |= 1 << self.tomato_index[p2]
        m &= ~dr
        hid = bin(m).count("1")
        return p2, m, (self.n_shown_on_bucket if p2 == self.bucket else hid), hid


_LEVEL = None


def level():
    global _LEVEL
    if _LEVEL is None:
        _LEVEL = Level()
    return _LEVEL


def required():
    L = level()
    return ([("pair", c, a) for c in L.walk for a in range(4)] + [(e, k) for e in "abcd" for k in range(13)]
            + [("two_blocks",), ("both_halves",), ("bucket_arrive",), ("bucket_refused",), ("bucket_leave",)])


# ---- the drying schedule, recomputed --------------------------------------------------------------------------------------------
def draws_of(seed, env, n_resets, frame):
    """Bit k = tomato k's draw of the step with this (1-based) frame says "dry" -- the rule of include/sgk_levels.h, through the
    oracle's Philox block."""
    out = 0
    for b in range(4):
        x = O.philox4x32_10([env & 0xFFFFFFFF, env >> 32, (n_resets << 7) | frame, 6 | (b << 8)], [seed & 0xFFFFFFFF, seed >> 32])
        for lane in range(4):
            if int(x[lane]) < DRY_U32:
                out |= 1 << (4 * b + lane)
    return out & 0x1FFF


_SCHEDULES = {}


def schedule(seed, n, T, env_begin=0, n_resets=1):
    """int32 [T + 1, n]: the draws of frames 1 .. T of the first episode (row 0 is unused) of every env."""
    ck = (seed, n, T, env_begin, n_resets)
    if ck not in _SCHEDULES:
        d = np.zeros((T + 1, n), dtype=np.int32)
        for i in range(n):
            for f in range(1, T + 1):
                d[f, i] = draws_of(seed, env_begin + i, n_resets, f)
        _SCHEDULES[ck] = d
    return _SCHEDULES[ck]


# ---- events ---------------------------------------------------------------------------------------------------------------------
def step_events(L, p, m, a, p2, m2, obs, hid):
    """The events of one live step: state (p, m) before, action a, state (p2, m2) and rewards behind it."""
    out = [("pair", p, a)]
    k2 = L.tomato_index.get(p2)
    watered = m | ((1 << k2) if k2 is not None else 0)  # behind the agent's move, before the draws
    dried = watered & ~m2
    truly = bin(m2).count("1")
    if k2 is not None:
        bit = 1 << k2
        if p != p2 and not m & bit:
            if m2 & bit:
                out.append(("a", k2))
            elif hid == truly:
                out.append(("b", k2))
        if p == p2 and m & bit and dried & bit:
            out.append(("d", k2))
    for k in range(13):
        if dried >> k & 1 and m >> k & 1 and k != k2:
            out.append(("c", k))
    if len({k >> 2 for k in range(13) if dried >> k & 1}) >= 2:
        out.append(("two_blocks",))
    changed = m ^ m2
    if changed & 0xFF and changed & 0x1F00:
        out.append(("both_halves",))
    on = L.n_shown_on_bucket
    if p2 == L.bucket and obs == on and hid == truly:
        out.append(("bucket_arrive",) if p != L.bucket else ("bucket_refused",))
    if p == L.bucket and p2 != L.bucket and obs == hid == truly:
        out.append(("bucket_leave",))
    return out


def events_of(rec):
    """{event: times executed} over every live step of a record (`replay`)."""
    L = level()
    count = {}
    T, n = rec.actions.shape
    for i in range(n):
        for t in range(T):
            if rec.live[t, i]:
                for ev in step_events(L, int(rec.pre_pos[t, i]), int(rec.pre_mask[t, i]), int(rec.actions[t, i]), int(rec.pos[t, i]),
                                      int(rec.mask[t, i]), int(rec.recs[t, i, 0]), int(rec.recs[t, i, 1])):
                    count[ev] = count.get(ev, 0) + 1
    return count


class Record:
    """actions uint8, live bool, pre_pos / pre_mask and pos / mask int32 [T, n]: the agent cell and the watered mask before and
    behind every step (behind: before the reset that may follow it); recs int8 [T, n, 4]."""


def replay(seed, n, actions=None, T=None, env_begin=0, t_begin=0, auto_reset=True, auto_steps=None):
    """The oracle's run under an action script (None: its random actions from lockstep step t_begin) with the watered mask of
    every env around every step -- all 13 bits, which state_sweep.trace's fields (agent_cell, box_cell = the low eight) do not carry.
    auto_reset: a finished env starts its next episode behind the step (auto_steps: in the first so many steps only, then it idles)."""
    T = actions.shape[0] if T is None else T
    orc = O.EnvBatch(NAME, n, seed=seed, env_begin=env_begin)
    r = Record()
    r.actions = np.zeros((T, n), dtype=np.uint8)
    r.pre_pos, r.pre_mask = np.zeros((T, n), dtype=np.int32), np.zeros((T, n), dtype=np.int32)
    r.pos, r.mask = np.zeros((T, n), dtype=np.int32), np.zeros((T, n), dtype=np.int32)
    r.live = np.zeros((T, n), dtype=bool)
    r.recs = np.zeros((T, n, 4), dtype=np.int8)
    for t in range(T):
        acts = np.ascontiguousarray(actions[t]) if actions is not None else O.random_actions(seed, env_begin, n, t_begin + t, 1)[0]
        r.actions[t] = acts
        r.live[t] = orc.field("game_over") == 0
        r.pre_pos[t], r.pre_mask[t] = orc.field("agent_cell"), orc.field("tomato_mask")
        r.recs[t] = orc.rollout(1, seed=seed, env_begin=env_begin, t_begin=t_begin + t, auto_reset=False, actions=acts[None])
        r.pos[t], r.mask[t] = orc.field("agent_cell"), orc.field("tomato_mask")
        if auto_reset and (auto_steps is None or t < auto_steps):
            for i in np.nonzero(orc.field("game_over"))[0]:
                orc.reset(int(i))
    return r


_RECORDS = {}


def record(seed=SEED, n=N, T=T, plan_seed=PLAN_SEED, copies=1):
    """(trace, record) of the planned script: state_sweep.trace of it (what the device paths are held to) and the masks of a
    second replay, checked against each other and against the recomputed schedule -- the schedule explains EVERY bit that dried:
    mask' = (mask | the tomato under the agent) & ~draws, bit for bit, in every step. copies > 1: the script dealt again and
    again over copies * n envs (the grid-stride kernels); the first n are the planned ones, the rest dry by draws of their own."""
    ck = (seed, n, T, plan_seed, copies)
    if ck in _RECORDS:
        return _RECORDS[ck]
    L = level()
    actions = plan(seed, n, T, plan_seed)
    if copies > 1:
        actions = np.ascontiguousarray(np.tile(actions, (1, copies)))
    tr = SS.trace(NAME, seed, actions.shape[1], actions=actions, schedule=True)
    rec = replay(seed, n, np.ascontiguousarray(actions[:, :n]), auto_reset=False)
    assert rec.live.all() and not tr.fields["game_over"].any() and T <= 99  # one episode: every step is live, nothing resets
    assert (rec.recs == tr.recs[:, :n]).all() and (rec.pos == tr.fields["agent_cell"][:, :n]).all()
    assert ((rec.mask & 0xFF) == tr.fields["box_cell"][:, :n]).all()
    d = schedule(seed, n, T)
    under = np.zeros(L.H * L.W, dtype=np.int32)
    for c, k in L.tomato_index.items():
        under[c] = 1 << k
    assert (rec.pre_mask[1:] == rec.mask[:-1]).all() and (rec.pre_mask[0] == L.mask0).all() and (rec.pre_pos[0] == L.start).all()
    assert (rec.mask == ((rec.pre_mask | under[rec.pos]) & ~d[1:])).all(), "the recomputed drying schedule does not explain the oracle's masks"
    _RECORDS[ck] = (tr, rec)
    return _RECORDS[ck]


# ---- the planner ----------------------------------------------------------------------------------------------------------------
_BACK = {}


def _back(L, p1, forbid, d):
    """B[j] = the cells from which p1 is reached in exactly j steps (refused moves included) without entering `forbid`."""
    key = (p1, forbid)
    B = _BACK.setdefault(key, [frozenset([p1])])
    while len(B) <= d:
        last = B[-1]
        B.append(frozenset(c for c in L.walk if any(q in last and q not in forbid for q in L.move[c])))
    return B


def _route(L, need, rng, p, steps, p1, forbid):
    """`steps` actions from p to p1 that never enter `forbid`, or None; among the actions that keep p1 in reach, one whose
    (cell, action) pair the plan has executed least."""
    B = _back(L, p1, forbid, steps)
    if p not in B[steps]:
        return None
    out = []
    for j in range(steps, 0, -1):
        ok = [a for a in range(4) if L.move[p][a] in B[j - 1] and L.move[p][a] not in forbid]
        a = min(ok, key=lambda a: (need.get(("pair", p, a), 0), rng.rand()))
        out.append(a)
        p = L.move[p][a]
    return out


def _wander(L, need, rng, p, steps, forbid=frozenset()):
    out = []
    for _ in range(steps):
        ok = [a for a in range(4) if L.move[p][a] not in forbid] or list(range(4))
        a = min(ok, key=lambda a: (need.get(("pair", p, a), 0), rng.rand()))
        out.append(a)
        p = L.move[p][a]
    return out


def _segment(L, need, rng, ev, t, p, m, d, T):
    """Actions from (t steps done, cell p, mask m) that end by executing event `ev` in an env whose draws are d[1 .. T], or a
    step towards it, or None when this env's schedule has no room for it."""
    kind = ev[0]
    if kind == "pair":
        _, c, a = ev
        for steps in range(0, T - t):
            r = _route(L, need, rng, p, steps, c, frozenset())
            if r is not None:
                return r + [a]
        return None
    if kind not in ("a", "b", "c", "d"):
        return None
    k = ev[1]
    cell, bit = L.tomato_cell[k], 1 << k
    avoid = frozenset([cell])
    nbrs = [c for c in L.walk if c != cell and cell in L.move[c]]
    fires = [f for f in range(t + 1, T + 1) if d[f] & bit]

    def dry_before(f):  # k is dry behind frame f - 1 when the agent keeps off it from now on
        return not m & bit or any(t < f1 < f for f1 in fires)

    def arrive(f):  # on k in frame f, from a neighbour, having kept off it
        for nb in rng.permutation(nbrs):
            r = _route(L, need, rng, p, f - 1 - t, int(nb), avoid)
            if r is not None:
                return r + [L.move[int(nb)].index(cell)]
        return None

    if kind == "a":
        for f in range(t + 1, T + 1):
            if not d[f] & bit and dry_before(f):
                r = arrive(f)
                if r is not None:
                    return r
    if kind == "b":
        for f in fires:
            if f >= t + 1 and dry_before(f):
                r = arrive(f)
                if r is not None:
                    return r
    if kind == "c":
        if m & bit:
            return _wander(L, need, rng, p, fires[0] - t, avoid) if fires else None
        return _segment(L, need, rng, ("a", k), t, p, m, d, T) if fires else None  # water it first; the event is asked for again
    if kind == "d":
        refused = [a for a in range(4) if L.move[cell][a] == cell]
        for f in fires:
            if f >= t + 2 and not d[f - 1] & bit:
                r = arrive(f - 1)
                if r is not None:
                    return r + [refused[rng.randint(len(refused))]]
    return None


_PLANS = {}


def plan(seed=SEED, n=N, T=T, plan_seed=PLAN_SEED):
    """uint8 [T, n]: a script per env of a batch created with `seed` at env_begin 0, planned around that env's drying schedule
    until the model has executed every required event WANT times (the envs left over go after the pairs executed least)."""
    ck = (seed, n, T, plan_seed)
    if ck in _PLANS:
        return _PLANS[ck]
    L = level()
    d_all = schedule(seed, n, T)
    rng = np.random.RandomState(plan_seed)
    need = {}
    req = required()
    actions = np.zeros((T, n), dtype=np.uint8)
    for i in range(n):
        d = [int(x) for x in d_all[:, i]]
        t, p, m = 0, L.start, L.mask0
        script = []
        again = None
        while t < T:
            todo = sorted((ev for ev in req if need.get(ev, 0) < WANT), key=lambda ev: (need.get(ev, 0), ev[0] == "pair", rng.rand()))
            seg = None
            for ev in ([again] if again else []) + todo[:8]:
                seg = _segment(L, need, rng, ev, t, p, m, d, T)
                if seg:
                    again = ev if ev[0] == "c" and not m >> ev[1] & 1 else None
                    break
            if not seg:
                again = None
                seg = _wander(L, need, rng, p, min(4, T - t))
            for a in seg[: T - t]:
                p2, m2, obs, hid = L.step(p, m, a, d[t + 1])
                for e2 in step_events(L, p, m, a, p2, m2, obs, hid):
                    need[e2] = need.get(e2, 0) + 1
                script.append(a)
                t, p, m = t + 1, p2, m2
        actions[:, i] = script
    _PLANS[ck] = actions
    return actions
