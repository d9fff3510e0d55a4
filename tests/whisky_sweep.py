"""A planned sweep of WhiskyGold -- helper of test_draw_sweeps_cpu.py and test_gpu_draw_sweeps.py. CPU only: the oracle, numpy and the
product's host-only library (tests/hostlib.py).

From the step after drinking the whisky, the level replaces the agent's action with probability 0.9 by a random one. The draws depend
on (seed, env index, reset count, frame) alone, never on the actions (include/sgk_levels.h: block(seed, 6, env, n_resets << 7 | frame),
replaced when x[0] < SGK_WHISKY_EXPLORATION_U32, by x[1] & 3), so every env's replacements are known before it moves: `draw_of`
recomputes them through the oracle's Philox block, and the planners write every env a script (or a list of memoryless policies over
(drunk, cell), rewritten between launches) AROUND them, from a model of the level read off the art in include/sgk_levels.h.

The planner is not the proof. The proof is the oracle's record of the plan (state_sweep.trace_phases): `explain` checks that the
recomputed draws explain every executed action in it, `events_of` counts the EVENTS the record executes while the episode is live, and
the tests require every one of `required()`:

  pair c d a                 every (agent cell, drunk bit, EXECUTED action): 16 sober cells, 17 drunk ones (the whisky's included)  132
  kept a / replaced a        drunk, the draw says keep and the chosen action a is executed / the draw replaces it by a              8
  replaced_same              the replacement equals the chosen action
  drink c                    sober arrival on the whisky from each of its three neighbours: observed -1 + 5, hidden -1              3
  first_drunk_step_replaced  the step right behind the drink is replaced
  rearrive c                 drunk arrival on the empty whisky cell from each neighbour: observed -1                               3
  refused_on_whisky_cell     a drunk agent standing on it walks into the wall: observed -1
  goal_sober / goal_drunk_kept / goal_drunk_replaced
  second_episode_drink       the whisky is back behind a reset and is drunk again (the draws keyed by the new reset count)

The time-limit plan (`timeout_plan`, TL_N envs x TL_T = 104 steps) has `timeout_sober` and `timeout_drunk`: the episode ends at
max_iterations off the goal: done = 1 in the step record, which is also what the replay ring's terminal flag holds -- include/sgk.h
does not tell a time limit from a terminal state, so the oracle's behaviour is what is pinned. (An ordinary episode takes six steps
here, so an env cannot play one and then run into the time limit within 104 steps: the envs run into it in their FIRST episode, and
the sober ones drink in the four steps behind it, by the draws of reset count 2.)"""
import os
import re

import numpy as np

import state_sweep as SS
from oracle import oracle as O

NAME = "WhiskyGold-v0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the committed choice, found by searching on the CPU (test_draw_sweeps_cpu.py fails when the oracle's record of either form misses an
# event): N envs created with SEED at env_begin 0, T steps of action script, the policy form's phases, the planner's own seed
SEED, N, T, PLAN_SEED = 5, 290, 40, 1
PHASES = (16, 16, 16, 16)
WANT = 3
TL_N, TL_T = 70, 104
EXPLORATION_U32 = 3865470566  # SGK_WHISKY_EXPLORATION_U32: floor(0.9 * 2^32)
MAX_ITERATIONS = 100


def _art():
    text = open(os.path.join(ROOT, "include", "sgk_levels.h")).read()
    body = re.search(r"SGK_WHISKY_ART\[SGK_WHISKY_H\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    return re.findall(r'"([^"]*)"', body)


class Level:
    def __init__(self):
        art = _art()
        self.H, self.W = len(art), len(art[0])
        flat = "".join(art)
        self.walk = [c for c, ch in enumerate(flat) if ch != "#"]
        self.start, self.whisky, self.goal = flat.index("A"), flat.index("W"), flat.index("G")
        self.sober_cells = [c for c in self.walk if c not in (self.whisky, self.goal)]
        self.drunk_cells = [c for c in self.walk if c != self.goal]
        e0 = O.EnvBatch(NAME, 1)
        assert int(e0.field("agent_cell")[0]) == self.start and int(e0.field("box_cell")[0]) == self.whisky
        self.delta = []
        for a in range(4):  # what an action does is read off the oracle (the start cell has a wall above: that move is refused)
            e = O.EnvBatch(NAME, 1)
            e.step(0, a)
            self.delta.append(int(e.field("agent_cell")[0]) - self.start)
        self.refused_at_start = self.delta.index(0)
        self.delta[self.refused_at_start] = -sum(self.delta)
        assert sorted(self.delta) == [-self.W, -1, 1, self.W]
        self.move = {c: [c + d if flat[c + d] != "#" else c for d in self.delta] for c in self.walk}
        self.whisky_nbrs = [c for c in self.sober_cells if self.whisky in self.move[c]]
        self.goal_nbrs = [c for c in self.sober_cells if self.goal in self.move[c]]
        assert len(self.sober_cells) == 16 and len(self.drunk_cells) == 17 and len(self.whisky_nbrs) == 3

    def tree(self, goal, forbid):
        """{cell: first action of a shortest way to `goal` that keeps off `forbid`}."""
        out, frontier = {}, [goal]
        while frontier:
            nxt = []
            for q in frontier:
                for c in self.walk:
                    if c not in out and c != goal and c not in forbid:
                        for a in range(4):
                            if self.move[c][a] == q:
                                out[c] = a
                                nxt.append(c)
                                break
            frontier = nxt
        return out

    def path(self, src, dst, forbid):
        seen, frontier = {src: []}, [src]
        while frontier and dst not in seen:
            nxt = []
            for q in frontier:
                for a in range(4):
                    c = self.move[q][a]
                    if c not in seen and c not in forbid:
                        seen[c] = seen[q] + [a]
                        nxt.append(c)
            frontier = nxt
        return seen.get(dst)


_LEVEL = None


def level():
    global _LEVEL
    if _LEVEL is None:
        _LEVEL = Level()
    return _LEVEL


def required():
    L = level()
    return ([("pair", c, 0, a) for c in L.sober_cells for a in range(4)] + [("pair", c, 1, a) for c in L.drunk_cells for a in range(4)]
            + [("kept", a) for a in range(4)] + [("replaced", a) for a in range(4)] + [("replaced_same",)]
            + [("drink", c) for c in L.whisky_nbrs] + [("first_drunk_step_replaced",)] + [("rearrive", c) for c in L.whisky_nbrs]
            + [("refused_on_whisky_cell",), ("goal_sober",), ("goal_drunk_kept",), ("goal_drunk_replaced",), ("second_episode_drink",)])


def required_timeout():
    return [("timeout_sober",), ("timeout_drunk",)]


# ---- the draws, recomputed ------------------------------------------------------------------------------------------------------
_DRAW_MEMO = {}


def draw_of(seed, env, n_resets, frame):
    """(replaced, by which action) of the step with this (1-based) frame of a DRUNK agent -- the rule of include/sgk_levels.h,
    through the oracle's Philox block."""
    ck = (seed, env, n_resets, frame)
    if ck not in _DRAW_MEMO:
        x = O.philox4x32_10([env & 0xFFFFFFFF, env >> 32, (n_resets << 7) | frame, 6], [seed & 0xFFFFFFFF, seed >> 32])
        _DRAW_MEMO[ck] = (int(x[0]) < EXPLORATION_U32, int(x[1]) & 3)
    return _DRAW_MEMO[ck]


def schedule(seed, n, frames, n_resets=1, env_begin=0):
    """int8 [frames + 1, n]: the replacement of every frame of the episode reset number n_resets starts (-1: the chosen action is
    kept; row 0 is unused) of every env."""
    out = np.full((frames + 1, n), -1, dtype=np.int8)
    for i in range(n):
        for f in range(1, frames + 1):
            rep, ra = draw_of(seed, env_begin + i, n_resets, f)
            if rep:
                out[f, i] = ra
    return out


# ---- events ---------------------------------------------------------------------------------------------------------------------
def step_events(L, c, d, a, x, rep, ra, post, obs, hid, done, n_resets, just_drank):
    """The events of one live step: cell c and drunk bit d before, chosen action a, executed x, the frame's draw (rep, ra), the cell
    and the rewards behind it."""
    out = [("pair", c, d, x)]
    if d:
        if rep:
            out.append(("replaced", ra))
            if ra == a:
                out.append(("replaced_same",))
            if just_drank:
                out.append(("first_drunk_step_replaced",))
        elif x == a:
            out.append(("kept", a))
        if post == L.whisky and obs == -1 and hid == -1:
            out.append(("rearrive", c) if c != L.whisky else ("refused_on_whisky_cell",))
        if post == L.goal:
            out.append(("goal_drunk_replaced",) if rep else ("goal_drunk_kept",))
    else:
        if post == L.whisky and obs == 4 and hid == -1:
            out.append(("drink", c))
            if n_resets >= 2:
                out.append(("second_episode_drink",))
        if post == L.goal:
            out.append(("goal_sober",))
    if done and post != L.goal:
        out.append(("timeout_drunk",) if d or post == L.whisky else ("timeout_sober",))
    return out


def _walk(tr):
    """Every live step of a record: (i, t, cell, drunk, chosen, executed, reset count, frame of the step, cell behind it, observed,
    hidden, done)."""
    for i in range(tr.n):
        for t in range(tr.T):
            f = {k: v[t] for k, v in tr.before.items()}
            if f["game_over"][i]:
                continue
            yield (i, t, int(f["agent_cell"][i]), int(f["box_cell"][i] == 255), int(tr.actions[t, i]), int(tr.recs[t, i, 3]),
                   int(f["n_resets"][i]), int(f["frame"][i]) + 1, int(tr.pre["agent_cell"][t, i]), int(tr.recs[t, i, 0]),
                   int(tr.recs[t, i, 1]), int(tr.recs[t, i, 2]))


def events_of(tr, seed, env_begin=0):
    """{event: times executed} over every live step of a record of state_sweep.trace_phases."""
    L = level()
    count = {}
    drank_at = {}
    for i, t, c, d, a, x, nr, frame, post, obs, hid, done in _walk(tr):
        rep, ra = draw_of(seed, env_begin + i, nr, frame)
        for ev in step_events(L, c, d, a, x, rep, ra, post, obs, hid, done, nr, drank_at.get(i) == (nr, frame - 1)):
            count[ev] = count.get(ev, 0) + 1
        if not d and post == L.whisky:
            drank_at[i] = (nr, frame)
    return count


def explain(tr, seed, env_begin=0):
    """The recomputed draws explain every executed action of the record: a sober agent's is the chosen one, a drunk agent's the
    replacement when its frame's draw replaces and the chosen one when it keeps; the agent moves by the executed action; the goal
    pays -1 + 50 on both channels and every other step -1, the drink +5 more on the observed channel alone."""
    L = level()
    n_drunk = 0
    for i, t, c, d, a, x, nr, frame, post, obs, hid, done in _walk(tr):
        rep, ra = draw_of(seed, env_begin + i, nr, frame)
        assert x == (ra if d and rep else a), "env %d step %d: executed %d, chosen %d, draw %s" % (i, t, x, a, (rep, ra))
        assert post == L.move[c][x], (i, t)
        drink = not d and post == L.whisky
        assert (obs, hid) == ((49, 49) if post == L.goal else (4, -1) if drink else (-1, -1)), (i, t, obs, hid)
        assert done == int(post == L.goal or frame >= MAX_ITERATIONS), (i, t)
        assert int(tr.pre["box_cell"][t, i]) == (255 if d or drink else L.whisky), (i, t)
        n_drunk += d
    return n_drunk


# ---- the planners ---------------------------------------------------------------------------------------------------------------
class _Sim:
    def __init__(self, L, seed, env, need):
        self.L, self.seed, self.env, self.need = L, seed, env, need
        self.nr, self.cell, self.drunk, self.frame, self.just_drank = 1, L.start, 0, 0, False

    def draw(self):
        return draw_of(self.seed, self.env, self.nr, self.frame + 1)

    def events(self, a):
        """(events, executed action, cell behind it, done) if `a` were chosen now."""
        L = self.L
        rep, ra = self.draw()
        x = ra if self.drunk and rep else a
        post = L.move[self.cell][x]
        drink = not self.drunk and post == L.whisky
        done = post == L.goal or self.frame + 1 >= MAX_ITERATIONS
        obs = 49 if post == L.goal else 4 if drink else -1
        return (step_events(L, self.cell, self.drunk, a, x, rep, ra, post, obs, 49 if post == L.goal else -1, done, self.nr,
                            self.just_drank), x, post, done)

    def step(self, a):
        evs, x, post, done = self.events(a)
        for ev in evs:
            self.need[ev] = self.need.get(ev, 0) + 1
        self.just_drank = not self.drunk and post == self.L.whisky
        self.drunk = int(self.drunk or post == self.L.whisky)
        self.cell, self.frame = post, self.frame + 1
        if done:
            self.nr, self.cell, self.drunk, self.frame, self.just_drank = self.nr + 1, self.L.start, 0, 0, False

    def novelty(self, a, rng):
        return sum(1.0 / (1 + self.need.get(ev, 0)) ** 2 for ev in self.events(a)[0]) + 1e-3 * rng.rand()

    def sober_target(self, rng, role):
        """What a sober env goes for next: ("pair", c, a), ("drink", neighbour) or ("goal", neighbour)."""
        L = self.L
        _, _, gnb = min((self.need.get(("pair", nb, 0, L.move[nb].index(L.goal)), 0), rng.rand(), nb) for nb in L.goal_nbrs)
        if role == 0 and self.nr == 1:
            return ("goal", gnb)  # ... and the whisky in the second episode
        pairs = [(self.need.get(("pair", c, 0, a), 0), rng.rand(), c, a) for c in L.sober_cells for a in range(4)
                 if L.move[c][a] not in (L.whisky, L.goal)]
        n, _, c, a = min(pairs)
        if role >= 2 and n < WANT:
            return ("pair", c, a)
        if self.need.get(("goal_sober",), 0) < WANT and role == 3:
            return ("goal", gnb)
        _, _, nb = min((self.need.get(("drink", nb), 0), rng.rand(), nb) for nb in L.whisky_nbrs)
        return ("drink", nb)

    def segment(self, target):
        L = self.L
        if target[0] == "pair":
            return L.path(self.cell, target[1], (L.whisky, L.goal)) + [target[2]]
        if target[0] == "drink":
            return L.path(self.cell, target[1], (L.whisky, L.goal)) + [L.move[target[1]].index(L.whisky)]
        return L.path(self.cell, target[1], (L.whisky, L.goal)) + [L.move[target[1]].index(L.goal)]


_PLANS = {}


def plan(seed=SEED, n=N, T=T, plan_seed=PLAN_SEED):
    """uint8 [T, n]: a script per env across episodes with auto-reset. Sober, an env goes by its role (index mod 4): the goal and
    then the whisky of the second episode; the whisky at once, from the neighbour the plan has least of; the sober (cell, action)
    pairs the plan has least of, then the whisky or the goal. Drunk, it knows each frame's draw and chooses the action whose step
    executes the events the plan has least of (in a replaced frame the choice decides `replaced_same` alone)."""
    ck = ("actions", seed, n, T, plan_seed)
    if ck in _PLANS:
        return _PLANS[ck]
    L = level()
    rng = np.random.RandomState(plan_seed)
    need = {}
    actions = np.zeros((T, n), dtype=np.uint8)
    for i in range(n):
        sim = _Sim(L, seed, i, need)
        seg = []
        for t in range(T):
            if sim.drunk:
                seg = []
                a = max(range(4), key=lambda a: sim.novelty(a, rng))
            else:
                if not seg:
                    seg = sim.segment(sim.sober_target(rng, i % 4))
                a = seg.pop(0)
            actions[t, i] = a
            sim.step(a)
            if sim.frame == 0:
                seg = []
    _PLANS[ck] = actions
    return actions


def _policy_row(L, sim, rng, role, nc):
    """One env's memoryless policy for one phase: int8 [2 * n_cells] over (drunk, cell)."""
    row = np.zeros(2 * nc, dtype=np.int8)
    target = sim.sober_target(rng, role) if not sim.drunk else ("drink", L.whisky_nbrs[rng.randint(3)])
    after = target
    if target[0] == "pair":  # behind the probe: the whisky, from the neighbour the plan has least of
        after = ("drink", min((sim.need.get(("drink", nb), 0), rng.rand(), nb) for nb in L.whisky_nbrs)[2])
    tree = L.tree(after[1], (L.whisky, L.goal))
    tree[after[1]] = L.move[after[1]].index(L.whisky if after[0] == "drink" else L.goal)
    for c in L.sober_cells:
        row[c] = tree[c]
    if target[0] == "pair" and not sim.drunk:
        c = sim.cell
        for a in L.path(c, target[1], (L.whisky, L.goal)):
            row[c] = a
            c = L.move[c][a]
        row[target[1]] = target[2]
    for c in L.drunk_cells:  # drunk: in every cell the action whose (cell, drunk, action) the plan has least of, were it kept
        score = []
        for a in range(4):
            post = L.move[c][a]
            evs = [("pair", c, 1, a), ("kept", a)]
            if post == L.goal:
                evs.append(("goal_drunk_kept",))
            if post == L.whisky:
                evs.append(("rearrive", c) if c != L.whisky else ("refused_on_whisky_cell",))
            score.append(sum(1.0 / (1 + sim.need.get(ev, 0)) ** 2 for ev in evs) + 1e-3 * rng.rand())
        row[nc + c] = int(np.argmax(score))
    return row


def plan_policies(seed=SEED, n=N, phases=PHASES, plan_seed=PLAN_SEED):
    """[(n_steps, policy int8 [n, n_states])]: memoryless policies over the product's state index (drunk * n_cells + cell), every
    env's rewritten between the launches from what the model says it has done so far."""
    ck = ("policy", seed, n, tuple(phases), plan_seed)
    if ck in _PLANS:
        return _PLANS[ck]
    L = level()
    nc = L.H * L.W
    assert SS.n_states(NAME) == 2 * nc
    rng = np.random.RandomState(plan_seed)
    need = {}
    sims = [_Sim(L, seed, i, need) for i in range(n)]
    out = []
    for p, steps in enumerate(phases):
        policy = np.zeros((n, 2 * nc), dtype=np.int8)
        for i, sim in enumerate(sims):
            policy[i] = _policy_row(L, sim, rng, (i + p) % 4, nc)
            for _ in range(steps):
                sim.step(int(policy[i, sim.drunk * nc + sim.cell]))
        out.append((steps, policy))
    _PLANS[ck] = out
    return out


def timeout_plan(seed=SEED, n=TL_N, T=TL_T):
    """(actions uint8 [T, n], policy int8 [n, n_states]). The odd envs walk into the wall above the start for 100 steps, sober (the
    script: and then drink, in the second episode); the even ones drink at once and then choose `left` for ever: where the draws
    keep them off the goal for 99 steps -- known beforehand, and asserted on the record -- the time limit ends a drunk episode."""
    L = level()
    nc = L.H * L.W
    left, right = L.delta.index(-1), L.delta.index(1)
    assert L.move[L.start][right] == L.whisky
    actions = np.full((T, n), L.refused_at_start, dtype=np.uint8)
    policy = np.full((n, 2 * nc), L.refused_at_start, dtype=np.int8)
    actions[MAX_ITERATIONS:, 1::2] = right
    actions[:, 0::2] = left
    actions[0, 0::2] = right
    policy[0::2, :nc] = right
    policy[0::2, nc:] = left
    return actions, policy


# ---- the records ----------------------------------------------------------------------------------------------------------------
_RECORDS = {}


def record(form="actions", schedule="auto", copies=1, n=None):
    """The oracle's record of the committed plan in either form (cached), explained by the recomputed draws. schedule: "auto",
    "reset", or "idle" (reset_done() behind every 5th step). copies / n: the script dealt again and again over n envs (the
    grid-stride kernel); the first N are the planned ones, the others are replaced by draws of their own."""
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
        assert explain(tr, SEED) > 0
    _RECORDS[ck] = tr
    return tr


def timeout_record(form="actions", schedule="auto"):
    ck = ("timeout", form, schedule)
    if ck not in _RECORDS:
        actions, policy = timeout_plan()
        tr = SS.trace_phases(NAME, SEED, TL_N, [(actions if form == "actions" else policy, [schedule] * TL_T)])
        assert explain(tr, SEED) > 0
        _RECORDS[ck] = tr
    return _RECORDS[ck]
