"""A planned sweep of FriendFoe -- helper of test_draw_sweeps_cpu.py and test_gpu_draw_sweeps.py. CPU only: the oracle, numpy and the
product's host-only library (tests/hostlib.py).

FriendFoe keeps six float64 estimates per env that outlive episodes and launches, and they decide the next episode's level. Its own
draws -- the bandit type of an episode and the neutral bandit's level -- depend on (seed, env index, reset count) alone
(include/sgk_levels.h: block(seed, 6, env, n_resets << 7).x[0] * 3 >> 32 and x[1] <= SGK_FOE_NEUTRAL_BOX0_U32), never on the actions,
so every env's types are known before it moves: `draws` recomputes them through the oracle's Philox block, and the planners write
every env a script (or a list of memoryless policies, rewritten between launches) AROUND its types, from a model of the level read off
the art in include/sgk_levels.h and a float64 model of the estimator.

The planner is not the proof. The proof is the oracle's record of the plan (state_sweep.trace_phases: step records, boards, every
state field and the six estimates of every env as bit patterns behind EVERY step): `explain` checks that the recomputed draws and the
model estimator explain every episode's type, every level and every estimate bit in it -- type and level inferred from the floor value
and the reward --, `events_of` counts the EVENTS the record executes, and the tests require every one of `required(form)`:

  pair ty c a        every (room type, agent cell, action) of the 10 cells that are not a box                                  120
  open ty lv ch      a box opened: type, level (the box that pays) and choice; +49 or -51 on both channels                    12
  friend_level1 / adversary_level1      an estimate has moved the reward to box 1
  flip_back ty       level 1 in one opened episode of that type (friend, adversary) and level 0 in a later one of the same env    2
  first_of_type ty   the tie at 0.5 / 0.5 resolves to level 0 (friend, adversary)                                              2
  all_three          an env whose three estimates all differ from 0.5
  same_type_twice / type_change      in consecutive episodes of one env
  depth 6            an env with at least 6 updates of one estimate (DEPTH: what the committed plans reach)
  quiet_launch       (policy form) a phase in which an env whose estimates have moved opens no box: the fused kernels' register copy
                     is not dirty in that launch, nothing is stored and nothing may change

The time-limit plan (`timeout_plan`, TL_N envs x TL_T = 104 steps) has its own: `timeout` (an episode ends at max_iterations without
a box: done = 1 in the step record, which is also what the replay ring's terminal flag holds -- include/sgk.h does not tell a time
limit from a terminal state, so the oracle's behaviour is what is pinned), `timeout_moved` (in an env whose estimates had moved: they
keep their bits across it) and `open_after_timeout` (the next episode, typed by reset count + 1, is played to a box)."""
import os
import re

import numpy as np

import state_sweep as SS
from oracle import oracle as O

NAME = "FriendFoe-v0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the committed choice, found by searching on the CPU (test_draw_sweeps_cpu.py fails when the oracle's record of either form misses an
# event): N envs created with SEED at env_begin 0, T steps of action script, the policy form's phases, the planner's own seed
SEED, N, T, PLAN_SEED = 5, 130, 48, 1
PHASES = (16, 16, 16, 16)
WANT = 3  # the planners go on until their model has every event this often (the requirement is once, on the oracle's record)
DEPTH = {"actions": 8, "policy": 9}  # the deepest estimate of the committed plans on the oracle's record (asserted equal, and >= 6)
TL_N, TL_T = 66, 104
NEUTRAL_BOX0_U32 = 2576980377  # SGK_FOE_NEUTRAL_BOX0_U32: floor(0.6 * 2^32)
MAX_ITERATIONS = 100
FRIEND, NEUTRAL, ADVERSARY = 0, 1, 2


# ---- the level, from the art ----------------------------------------------------------------------------------------------------
def _art():
    text = open(os.path.join(ROOT, "include", "sgk_levels.h")).read()
    body = re.search(r"SGK_FOE_ART\[SGK_FOE_H\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    return re.findall(r'"([^"]*)"', body)


class Level:
    def __init__(self):
        art = _art()
        self.H, self.W = len(art), len(art[0])
        flat = "".join(art)
        self.walk = [c for c, ch in enumerate(flat) if ch != "#"]
        self.boxes = sorted(c for c, ch in enumerate(flat) if ch in "10")  # box 0 = the left one
        self.start = flat.index("A")
        self.cells = [c for c in self.walk if c not in self.boxes]
        e0 = O.EnvBatch(NAME, 1)
        assert int(e0.field("agent_cell")[0]) == self.start
        self.delta = []
        for a in range(4):  # what an action does is read off the oracle (the start cell is free on three sides; the fourth is refused)
            e = O.EnvBatch(NAME, 1)
            e.step(0, a)
            self.delta.append(int(e.field("agent_cell")[0]) - self.start)
        self.refused_at_start = self.delta.index(0)
        self.delta[self.refused_at_start] = -sum(self.delta)  # up + down + left + right = 0
        assert sorted(self.delta) == [-self.W, -1, 1, self.W]
        self.move = {c: [c + d if flat[c + d] != "#" else c for d in self.delta] for c in self.walk}
        assert len(self.cells) == 10 and len(self.boxes) == 2 and self.boxes[0] // self.W == self.boxes[1] // self.W
        self.toward = [self._tree(b) for b in self.boxes]

    def _tree(self, goal):
        """{cell: first action of a shortest way to the box `goal` over cells that are not a box}."""
        out, frontier = {}, [goal]
        while frontier:
            nxt = []
            for q in frontier:
                for c in self.cells:
                    if c not in out:
                        for a in range(4):
                            if self.move[c][a] == q:
                                out[c] = a
                                nxt.append(c)
                                break
            frontier = nxt
        return out

    def path(self, src, dst):
        """Actions of a shortest way from src to dst over cells that are not a box."""
        seen, frontier = {src: []}, [src]
        while frontier and dst not in seen:
            nxt = []
            for q in frontier:
                for a in range(4):
                    c = self.move[q][a]
                    if c not in seen and c in self.cells:
                        seen[c] = seen[q] + [a]
                        nxt.append(c)
            frontier = nxt
        return seen[dst]


_LEVEL = None


def level():
    global _LEVEL
    if _LEVEL is None:
        _LEVEL = Level()
    return _LEVEL


def required(form="actions"):
    L = level()
    out = ([("pair", ty, c, a) for ty in range(3) for c in L.cells for a in range(4)]
           + [("open", ty, lv, ch) for ty in range(3) for lv in range(2) for ch in range(2)]
           + [("friend_level1",), ("adversary_level1",), ("flip_back", FRIEND), ("flip_back", ADVERSARY), ("first_of_type", FRIEND),
              ("first_of_type", ADVERSARY), ("all_three",), ("same_type_twice",), ("type_change",), ("depth", 6)])
    return out + ([("quiet_launch",)] if form == "policy" else [])


def required_timeout():
    return [("timeout",), ("timeout_moved",), ("open_after_timeout",)]


# ---- the draws, recomputed ------------------------------------------------------------------------------------------------------
def draw_of(seed, env, n_resets):
    """(bandit type, the neutral bandit's level) of the episode that reset number n_resets starts -- the rule of
    include/sgk_levels.h, through the oracle's Philox block."""
    x = O.philox4x32_10([env & 0xFFFFFFFF, env >> 32, n_resets << 7, 6], [seed & 0xFFFFFFFF, seed >> 32])
    return (int(x[0]) * 3) >> 32, 0 if int(x[1]) <= NEUTRAL_BOX0_U32 else 1


_DRAWS = {}


def draws(seed, n, resets, env_begin=0):
    """int8 [resets + 1, n, 2]: (type, neutral level) of reset counts 1 .. resets (row 0 is unused) of every env."""
    ck = (seed, n, resets, env_begin)
    if ck not in _DRAWS:
        d = np.zeros((resets + 1, n, 2), dtype=np.int8)
        for i in range(n):
            for r in range(1, resets + 1):
                d[r, i] = draw_of(seed, env_begin + i, r)
        _DRAWS[ck] = d
    return _DRAWS[ck]


class Estimator:
    """PolicyEstimator of the level's text, in Python's float64: the same two products and one sum, in the same order."""

    def __init__(self):
        self.p = [[0.5, 0.5] for _ in range(3)]
        self.count = [0, 0, 0]

    def update(self, ty, choice):
        self.p[ty][0] *= 0.75
        self.p[ty][1] *= 0.75
        self.p[ty][choice] += 0.25
        self.count[ty] += 1

    def level(self, ty, neutral_level):
        p0, p1 = self.p[ty]
        if ty == FRIEND:
            return 1 if p1 > p0 else 0  # the first maximum
        if ty == NEUTRAL:
            return int(neutral_level)
        return 1 if p1 < p0 else 0  # the first minimum

    def bits(self):
        return np.array([x for pair in self.p for x in pair], dtype=np.float64).view(np.uint64)


# ---- events ---------------------------------------------------------------------------------------------------------------------
class _EnvLog:
    """What one env has done so far, and the events that follow from it: shared by the planners' model and by events_of."""

    def __init__(self):
        self.count = [0, 0, 0]
        self.seen1 = [False, False, False]
        self.last_type = None
        self.after_timeout = False
        self.opened_in_phase = False

    def begin(self, ty):
        out = []
        if self.last_type is not None:
            out.append(("same_type_twice",) if ty == self.last_type else ("type_change",))
        self.last_type = ty
        return out

    def opened(self, ty, lv, ch):
        out = [("open", ty, lv, ch)]
        if ty != NEUTRAL:
            if lv == 1:
                out.append(("friend_level1",) if ty == FRIEND else ("adversary_level1",))
            if self.count[ty] == 0 and lv == 0:
                out.append(("first_of_type", ty))
            if self.seen1[ty] and lv == 0:
                out.append(("flip_back", ty))
            self.seen1[ty] = self.seen1[ty] or lv == 1
        self.count[ty] += 1
        if min(self.count) > 0:
            out.append(("all_three",))
        if max(self.count) >= 6:
            out.append(("depth", 6))
        if self.after_timeout:
            out.append(("open_after_timeout",))
        self.after_timeout = False
        self.opened_in_phase = True
        return out

    def timed_out(self):
        self.after_timeout = True
        return [("timeout",)] + ([("timeout_moved",)] if max(self.count) > 0 else [])

    def phase_begins(self):
        self.moved_before_phase = max(self.count) > 0
        self.opened_in_phase = False

    def phase_ends(self):
        return [("quiet_launch",)] if self.moved_before_phase and not self.opened_in_phase else []


def _walk(tr):
    """Every live step of a record, env by env: (i, t, type by the floor, reset count, cell, action, how it ended, choice, level by
    the reward) -- how it ended: None, "open" or "timeout"."""
    L = level()
    box0, box1 = L.boxes
    for i in range(tr.n):
        for t in range(tr.T):
            f = {k: v[t] for k, v in tr.before.items()}
            if f["game_over"][i]:
                continue
            board = tr.boards_before[t, i]
            ty = int(board.max()) - 5  # the floor value of the room: 5 / 6 / 7 (the boxes show 4, the agent 2)
            assert 0 <= ty <= 2, (i, t, board)
            end = ch = lv = None
            if tr.pre["game_over"][t, i]:
                cell = int(tr.pre["agent_cell"][t, i])
                if cell in (box0, box1):
                    end, ch = "open", int(cell == box1)
                    r = int(tr.recs[t, i, 0])
                    assert r in (49, -51) and r == int(tr.recs[t, i, 1]), (i, t, r)  # -1 and +50 / -50, on both channels
                    lv = ch if r > 0 else 1 - ch
                else:
                    end = "timeout"
                    assert int(tr.pre["frame"][t, i]) == MAX_ITERATIONS and tuple(tr.recs[t, i, :3]) == (-1, -1, 1), (i, t)
            yield i, t, ty, int(f["n_resets"][i]), int(f["agent_cell"][i]), int(tr.actions[t, i]), end, ch, lv


def events_of(tr):
    """({event: times executed} over a record of state_sweep.trace_phases, the deepest estimate: updates of one estimate of one env)."""
    count, depth = {}, 0

    def add(evs):
        for ev in evs:
            count[ev] = count.get(ev, 0) + 1

    starts = {0} | {e + 1 for e in tr.phase_end[:-1]}
    ends = set(tr.phase_end)
    steps = {}
    for rec in _walk(tr):
        steps.setdefault(rec[0], {})[rec[1]] = rec
    for i in range(tr.n):
        log, new_episode = _EnvLog(), True
        for t in range(tr.T):
            if t in starts:
                log.phase_begins()
            rec = steps.get(i, {}).get(t)
            if rec is not None:
                _, _, ty, _, cell, a, end, ch, lv = rec
                if new_episode:
                    add(log.begin(ty))
                    new_episode = False
                add([("pair", ty, cell, a)])
                if end == "open":
                    add(log.opened(ty, lv, ch))
                elif end == "timeout":
                    add(log.timed_out())
                new_episode = end is not None
            if t in ends and len(tr.phase_end) > 1:
                add(log.phase_ends())
        depth = max(depth, max(log.count))
    return count, depth


def explain(tr, seed, env_begin=0):
    """The recomputed draws and the model estimator explain the record: every episode's type (by the floor), every neutral level and
    every friend's / adversary's level (by the reward of the opened box), and every bit of the six estimates behind every step --
    across every episode boundary, a time limit included, which leaves them alone and still advances the reset count."""
    resets = int(tr.before["n_resets"].max()) + 1
    d = draws(seed, tr.n, resets, env_begin)
    est = [Estimator() for _ in range(tr.n)]
    want = np.zeros_like(tr.aux)
    by_t = {}
    for rec in _walk(tr):
        by_t.setdefault(rec[1], []).append(rec)
    assert (tr.aux0 == Estimator().bits()[None, :]).all()
    for t in range(tr.T):
        for i, _, ty, nr, _, _, end, ch, lv in by_t.get(t, []):
            assert ty == d[nr, i, 0], "env %d reset %d: the floor shows type %d, the draw says %d" % (i, nr, ty, d[nr, i, 0])
            if end == "open":
                assert lv == est[i].level(ty, d[nr, i, 1]), "env %d reset %d type %d: level %d by the reward" % (i, nr, ty, lv)
                est[i].update(ty, ch)
        for i in range(tr.n):
            want[t, i] = est[i].bits()
    assert (tr.aux == want).all(), "the model estimator does not explain the oracle's estimates"
    return True


# ---- the planners ---------------------------------------------------------------------------------------------------------------
class _Sim:
    """One env of the planners' model: the level, the recomputed draws, the estimator."""

    def __init__(self, L, d, need):
        self.L, self.d, self.need = L, d, need
        self.est, self.log = Estimator(), _EnvLog()
        self.nr, self.cell, self.frame = 1, L.start, 0
        self._begin()

    def _begin(self):
        self.ty = int(self.d[self.nr][0])
        self.lv = self.est.level(self.ty, int(self.d[self.nr][1]))
        self._count(self.log.begin(self.ty))

    def _count(self, evs):
        for ev in evs:
            self.need[ev] = self.need.get(ev, 0) + 1

    def step(self, a):
        L = self.L
        self._count([("pair", self.ty, self.cell, a)])
        self.cell = L.move[self.cell][a]
        self.frame += 1
        ended = True
        if self.cell in L.boxes:
            ch = L.boxes.index(self.cell)
            self._count(self.log.opened(self.ty, self.lv, ch))
            self.est.update(self.ty, ch)
        elif self.frame >= MAX_ITERATIONS:
            self._count(self.log.timed_out())
        else:
            ended = False
        if ended:
            self.nr, self.cell, self.frame = self.nr + 1, L.start, 0
            self._begin()
        return ended

    def choice(self, rng, ty=None):
        """The box to open in an episode of type ty: the opening the plan has least of, and a level that flips after it."""
        ty = self.ty if ty is None else ty
        lv = self.lv if ty == self.ty else self.est.level(ty, 0)
        best = None
        for ch in range(2):
            score = self.need.get(("open", ty, lv, ch), 0) + 0.3 * rng.rand()
            if ty != NEUTRAL:
                e2 = Estimator()
                e2.p[ty] = list(self.est.p[ty])
                e2.update(ty, ch)
                nxt = e2.level(ty, 0)
                wish = (("friend_level1",) if ty == FRIEND else ("adversary_level1",)) if nxt == 1 else ("flip_back", ty)
                if nxt != lv:
                    score += 0.5 * min(self.need.get(wish, 0), WANT) - 1.0
            if best is None or score < best[0]:
                best = (score, ch)
        return best[1]

    def probe(self, rng, ty=None):
        """The (cell, action) of this room type the plan has executed least, or None when it has them all WANT times."""
        ty = self.ty if ty is None else ty
        todo = [(self.need.get(("pair", ty, c, a), 0), rng.rand(), c, a) for c in self.L.cells for a in range(4)]
        n, _, c, a = min(todo)
        return (c, a) if n < WANT else None


_PLANS = {}


def plan(seed=SEED, n=N, T=T, plan_seed=PLAN_SEED):
    """uint8 [T, n]: a script per env of a batch created with `seed` at env_begin 0, across episodes with auto-reset: two envs of
    three take a detour over the (type, cell, action) the plan has least of before they open a box, the third plays shortest
    episodes (the deepest estimates); which box: _Sim.choice."""
    ck = ("actions", seed, n, T, plan_seed)
    if ck in _PLANS:
        return _PLANS[ck]
    L = level()
    d = draws(seed, n, T + 2)
    rng = np.random.RandomState(plan_seed)
    need = {}
    actions = np.zeros((T, n), dtype=np.uint8)
    for i in range(n):
        sim = _Sim(L, d[:, i], need)
        script = []
        while len(script) < T:
            seg, cell = [], sim.cell
            pr = sim.probe(rng) if i % 3 else None
            if pr is not None:
                seg = L.path(cell, pr[0]) + [pr[1]]
                cell = L.move[pr[0]][pr[1]]
            tree = L.toward[sim.choice(rng)]
            while cell not in L.boxes:
                seg.append(tree[cell])
                cell = L.move[cell][seg[-1]]
            for a in seg[: T - len(script)]:
                script.append(a)
                sim.step(a)
        actions[:, i] = script
    _PLANS[ck] = actions
    return actions


def plan_policies(seed=SEED, n=N, phases=PHASES, plan_seed=PLAN_SEED):
    """[(n_steps, policy int8 [n, n_states])]: memoryless policies over the product's state index (room type * n_cells + cell), every
    env's rewritten between the launches. Per room type: the shortest way to the chosen box from every cell, overridden along the
    shortest way from the start to the probed cell and by the probed action there (a refused probe, or one that leads back onto the
    way, loops until the phase ends: that env opens nothing more in the phase). One env of five whose estimates have moved walks
    into the wall below the start for a whole phase: the quiet launch."""
    ck = ("policy", seed, n, tuple(phases), plan_seed)
    if ck in _PLANS:
        return _PLANS[ck]
    L = level()
    nc = L.H * L.W
    ns = SS.n_states(NAME)
    assert ns == 3 * nc
    d = draws(seed, n, sum(phases) + 2)
    rng = np.random.RandomState(plan_seed)
    need = {}
    sims = [_Sim(L, d[:, i], need) for i in range(n)]
    out = []
    for p, steps in enumerate(phases):
        policy = np.zeros((n, ns), dtype=np.int8)
        for i, sim in enumerate(sims):
            sim.log.phase_begins()
            if p > 0 and (i + p) % 5 == 2 and max(sim.log.count) > 0:
                policy[i, :] = L.refused_at_start
            else:
                for ty in range(3):
                    tree = L.toward[sim.choice(rng, ty)]
                    for c in L.cells:
                        policy[i, ty * nc + c] = tree[c]
                    pr = sim.probe(rng, ty) if i % 3 else None
                    if pr is not None:
                        c = L.start
                        for a in L.path(L.start, pr[0]):
                            policy[i, ty * nc + c] = a
                            c = L.move[c][a]
                        policy[i, ty * nc + pr[0]] = pr[1]
            for _ in range(steps):
                sim.step(int(policy[i, sim.ty * nc + sim.cell]))
            for ev in sim.log.phase_ends():
                need[ev] = need.get(ev, 0) + 1
        out.append((steps, policy))
    _PLANS[ck] = out
    return out


def timeout_plan(seed=SEED, n=TL_N, T=TL_T):
    """(actions uint8 [T, n], policy int8 [n, n_states]) of the time-limit plan. Script: the even envs play one shortest episode and
    then walk into the wall below the start for 100 steps (the time limit falls on the last step); the odd ones do so from the start
    and open a box in the four steps behind the time limit. One policy: a memoryless policy cannot tell the first episode from the
    second but by the room type, so the even envs open a box in rooms of their first episode's type and walk into the wall in the
    others, the odd ones the other way round; an env whose first two episodes have the same type plays on as its types say."""
    L = level()
    nc = L.H * L.W
    d = draws(seed, n, 32)
    actions = np.full((T, n), L.refused_at_start, dtype=np.uint8)
    policy = np.zeros((n, SS.n_states(NAME)), dtype=np.int8)
    for i in range(n):
        ch = (i >> 1) & 1
        episode = []
        c = L.start
        while c not in L.boxes:
            episode.append(L.toward[ch][c])
            c = L.move[c][episode[-1]]
        at = 0 if i % 2 == 0 else MAX_ITERATIONS
        actions[at:at + len(episode), i] = episode[: T - at]
        first = int(d[1, i, 0])
        for ty in range(3):
            opens = (ty == first) == (i % 2 == 0)
            for c in L.cells:
                policy[i, ty * nc + c] = L.toward[ch][c] if opens else L.refused_at_start
    return actions, policy


# ---- the records ----------------------------------------------------------------------------------------------------------------
_RECORDS = {}


def record(form="actions", schedule="auto", copies=1, n=None):
    """The oracle's record of the committed plan in either form (cached: the tests share one per form and schedule kind), explained by
    the recomputed draws. schedule: "auto", "reset", or "idle" (reset_done() behind every 5th step). copies / n: the script dealt again
    and again over n envs (the grid-stride kernel); the first N are the planned ones, the others play the same scripts in rooms of
    their own; without the states before each reset, which only the events need."""
    ck = (form, schedule, copies, n)
    if ck in _RECORDS:
        return _RECORDS[ck]

    def kinds(T):
        return ["reset" if t % 5 == 4 else "none" for t in range(T)] if schedule == "idle" else [schedule] * T

    if form == "actions":
        actions = plan()
        if copies > 1:
            actions = np.ascontiguousarray(np.tile(actions, (1, copies))[:, :n])
        tr = SS.trace_phases(NAME, SEED, actions.shape[1], [(actions, kinds(T))], pre=copies == 1)
    else:
        tr = SS.trace_phases(NAME, SEED, N, [(pol, kinds(steps)) for steps, pol in plan_policies()])
    if copies == 1:
        explain(tr, SEED)
    _RECORDS[ck] = tr
    return tr


def timeout_record(form="actions", schedule="auto"):
    ck = ("timeout", form, schedule)
    if ck not in _RECORDS:
        actions, policy = timeout_plan()
        tr = SS.trace_phases(NAME, SEED, TL_N, [(actions if form == "actions" else policy, [schedule] * TL_T)])
        explain(tr, SEED)
        _RECORDS[ck] = tr
    return _RECORDS[ck]
