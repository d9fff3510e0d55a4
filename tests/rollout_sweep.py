"""Planned sweeps of the rollouts that choose their own actions -- helper of test_rollout_sweep_cpu.py and test_gpu_rollout_sweep.py.
CPU only: the oracle, numpy and the product's host-only library (tests/hostlib.py).

sgk_rollout_random(_stream), sgk_policy_rollout* and sgk_convq_rollout* cannot be handed an action script, but what each of them draws
at the first step of a launch is known before the launch: sgk_random_action(seed, env, t0), Philox stream 2's x2 & 3 at epsilon 1
(O.eps_greedy(., 1.0, ...)), or the categorical draw on four equal logits (O.categorical_sample(zeros, ...)). So nothing is forced: `plant`
deals every reachable state of a level to envs that are GOING to draw the action it still needs, and brings every env into its state
at the same lockstep step through env.step and env.reset(mask), both swept already (tests/state_sweep.py): the scripts are
right-aligned, an env plays action 0 until the masked reset in front of its path. The launch then executes every reachable
(agent cell, second sprite cell, coin / mode bit, action) at its step 0, from a state word, boards and counters it did not produce.
`trace_from_planted` is the oracle's record of the planting and of K steps behind it under the launch's own draws."""
import numpy as np

import state_sweep as SS
from oracle import oracle as O

SEED = SS.SEED
DRAW0 = 1000  # draw_index0 of the epsilon-greedy / categorical launches
# Envs per level: at most the level's SIZES entry, no multiple of 64, a multiple of MEMBERS[level]; large enough that every (coin,
# action) class of every chooser holds an env per reachable state (plant() refuses otherwise; test_rollout_sweep_cpu.py asserts it)
N = {"BoatRace-v0": 130, "IslandNavigation-v0": 225, "SideEffectsSokoban-v0": 497, "DistributionalShift-v0": 289,
     "AbsentSupervisor-v0": 235, "SafeInterruptibility-v0": 515, "ConveyorBelt-v0": 3024}
# members of the population rollouts: divides n; the envs of a member are a contiguous block that cuts across the order the states are
# dealt in (by coin and drawn action), so every member sees a mixture
MEMBERS = {"BoatRace-v0": 5, "IslandNavigation-v0": 5, "SideEffectsSokoban-v0": 7, "DistributionalShift-v0": 17,
           "AbsentSupervisor-v0": 5, "SafeInterruptibility-v0": 5, "ConveyorBelt-v0": 7}
# steps of the continuation per level: the smallest K in 4 .. 8 at which, under every chooser, an episode ends inside the launch, is
# reset there and steps again (test_rollout_sweep_cpu.py asserts the events; `python tests/test_rollout_sweep_cpu.py` prints the search)
K_STEPS = {"BoatRace-v0": 4, "IslandNavigation-v0": 4, "SideEffectsSokoban-v0": 4, "DistributionalShift-v0": 4,
           "AbsentSupervisor-v0": 4, "SafeInterruptibility-v0": 4, "ConveyorBelt-v0": 4}
CHOOSERS = ("random", "eps1", "sample")
LIMIT_LEVELS = ("BoatRace-v0", "IslandNavigation-v0")
LIMIT_BEFORE = 3  # the time-limit leg launches at frame max_iterations - 3
LIMIT_K = 6
MAX_ITERATIONS = 100  # env.info.max_iterations of every level (the GPU tests assert it)


class Plan:
    """name, n, seed, env_begin; scripts uint8 [L, n] and masks uint8 [L + 1, n]: env.reset(masks[t]) where any, then
    env.step(scripts[t]) without auto-reset, for t < L, and masks[L] in front of the launch (the state reached by reset alone has an
    empty path: its env plays zeros to the end and is reset last); states: the (agent_cell, box_cell, coin) dealt to each env, or None
    (a plan that deals none: the time-limit leg); paths: each env's path; late bool [n]: see plant(); draws as given."""

    @property
    def L(self):
        return self.scripts.shape[0]


def first_draws(chooser, n, t0, seed=SEED, env_begin=0, draw0=DRAW0, k=0):
    """uint8 [n]: what a launch that starts at lockstep step `t0` / draw index `draw0` takes at its step k, by chooser."""
    flat = np.zeros((n, 4), dtype=np.float32)
    if chooser == "random":
        return O.random_actions(seed, env_begin, n, t0 + k, 1)[0]
    if chooser == "eps1":
        return O.eps_greedy(flat, 1.0, seed, env_begin, draw0 + k)
    assert chooser == "sample", chooser
    return O.categorical_sample(flat, seed, env_begin, draw0 + k)[0]


def depth(name, seed=SEED, env_begin=0):
    """The deepest shortest path of the level."""
    by_coin, _ = SS.reachable_pairs(name, seed, env_begin)
    return max(len(p) for states in by_coin.values() for p in states.values())


_TRANS_CACHE = {}


def _transitions(name, seed=SEED, env_index=0):
    """{state: {action: next state}} over the non-terminating steps of env `env_index`'s first episode, from SS.reachable's paths."""
    ck = (name, seed, env_index)
    if ck not in _TRANS_CACHE:
        out = {}
        for s, path in SS.reachable(name, seed, env_index).items():
            out[s] = {}
            for a in range(4):
                e = O.EnvBatch(name, 1, seed=seed, env_begin=env_index)
                for pa in path:
                    e.step(0, pa)
                if not e.step(0, a)[2]:
                    out[s][a] = SS._key(e)
        _TRANS_CACHE[ck] = out
    return _TRANS_CACHE[ck]


def endless(name, seed=SEED):
    """Whether no step of the level ends an episode (BoatRace, ConveyorBelt: only the time limit does). A launch of at most 8 steps
    ends an episode of such a level only in envs that arrive late in theirs: see plant()."""
    if name in SS.COIN_ENVS:
        return False
    return all(len(nxt) == 4 for nxt in _transitions(name, seed).values())


def launch_step(name, seed=SEED, env_begin=0):
    """The planting steps of the level's plans, hence the lockstep step their launches start at: the deepest path, or on an endless
    level MAX_ITERATIONS - LIMIT_BEFORE (the late envs' frame at the launch)."""
    return MAX_ITERATIONS - LIMIT_BEFORE if endless(name, seed) else depth(name, seed, env_begin)


def plant(name, draws, seed=SEED, env_begin=0):
    """The Plan that puts env i into a reachable state s for which (s, draws[i]) is still needed: states are dealt per class (coin of
    the env's SECOND episode -- every env is reset exactly once by mask --, drawn action) in breadth-first order, and when a class has
    covered its states its remaining envs take them again, in order. Refuses when a class has fewer envs than the level has states.
    On an endless level (no step ends an episode) the envs that take a state AGAIN arrive late where they can: an env whose state
    has an action that leaves it unchanged is reset in front of step 0 and repeats that action behind its path up to the launch, so
    it holds the dealt state at frame MAX_ITERATIONS - LIMIT_BEFORE and the time limit ends its episode at the launch's step 2.
    The first env of every pair keeps its shortest path: the pairs are covered at every frame a shortest path gives."""
    assert name in SS.SWEPT, name
    draws = np.ascontiguousarray(draws, dtype=np.uint8)
    n = draws.shape[0]
    by_coin, _ = SS.reachable_pairs(name, seed, env_begin)
    batch = O.EnvBatch(name, n, seed=seed, env_begin=env_begin)
    batch.reset()
    coin = batch.export(boards=False)[1]["coin"]
    order = {c: list(states) for c, states in by_coin.items()}
    dealt = {(c, a): 0 for c in by_coin for a in range(4)}
    L = launch_step(name, seed, env_begin)
    stay = {}
    if endless(name, seed):
        stay = {s: min(a for a in nxt if nxt[a] == s) for s, nxt in _transitions(name, seed).items() if s in nxt.values()}
    states, paths, late = [], [], np.zeros(n, dtype=bool)
    for i in range(n):
        c, a = int(coin[i]), int(draws[i])
        s = order[c][dealt[(c, a)] % len(order[c])]
        again = dealt[(c, a)] >= len(order[c])
        dealt[(c, a)] += 1
        path = list(by_coin[c][s])
        if again and s in stay:
            path += [stay[s]] * (L - len(path))
            late[i] = True
        states.append(s)
        paths.append(path)
    for (c, a), got in dealt.items():
        assert got >= len(order[c]), "%s: the class (coin %d, action %d) has %d envs of %d for its %d states" % (name, c, a, got, n, len(order[c]))
    assert max(len(path) for path in paths) <= L, (name, L)
    assert late.any() == endless(name, seed), (name, "no env arrives late on an endless level")
    p = Plan()
    p.name, p.n, p.seed, p.env_begin, p.draws, p.states, p.paths, p.late = name, n, seed, env_begin, draws, states, paths, late
    p.scripts = np.zeros((L, n), dtype=np.uint8)
    p.masks = np.zeros((L + 1, n), dtype=np.uint8)
    for i, path in enumerate(paths):
        p.masks[L - len(path), i] = 1
        p.scripts[L - len(path):, i] = path
    return p


_PLAN_CACHE = {}


def planned(name, chooser, n=None, seed=SEED, env_begin=0):
    """plant() for a launch behind the planting itself: it starts at lockstep step launch_step(name), draw index DRAW0."""
    n = N[name] if n is None else int(n)
    ck = (name, chooser, n, seed, env_begin)
    if ck not in _PLAN_CACHE:
        _PLAN_CACHE[ck] = plant(name, first_draws(chooser, n, launch_step(name, seed, env_begin), seed, env_begin), seed, env_begin)
    return _PLAN_CACHE[ck]


def limit_plan(name, n=None, seed=SEED):
    """The time-limit leg: every env walks MAX_ITERATIONS - LIMIT_BEFORE steps of its first episode without ending it -- a seeded walk
    of its own over the level's non-terminating steps --, so the launch starts at frame 97 and the limit ends every episode that no
    terminal cell ends first at its step 2. No masked reset, no state dealt."""
    assert name in LIMIT_LEVELS, name  # no coin: one transition table serves every env
    n = N[name] if n is None else int(n)
    ck = ("limit", name, n, seed)
    if ck in _PLAN_CACHE:
        return _PLAN_CACHE[ck]
    trans = _transitions(name, seed)
    start = SS._key(O.EnvBatch(name, 1, seed=seed))
    L = MAX_ITERATIONS - LIMIT_BEFORE
    p = Plan()
    p.name, p.n, p.seed, p.env_begin, p.draws, p.states, p.paths, p.late = name, n, seed, 0, None, None, None, np.ones(n, dtype=bool)
    p.scripts = np.zeros((L, n), dtype=np.uint8)
    p.masks = np.zeros((L + 1, n), dtype=np.uint8)
    p.safe = trans  # what test_rollout_sweep_cpu.py tells a limit's end from a terminal cell's by
    rng = np.random.RandomState(97 + len(name))
    for i in range(n):
        s = start
        for t in range(L):
            a = sorted(trans[s])[rng.randint(len(trans[s]))]
            p.scripts[t, i] = a
            s = trans[s][a]
    _PLAN_CACHE[ck] = p
    return p


def script_plan(name, actions, seed):
    """A Plan that plays an action script WITH auto-reset and resets nothing by mask, deals no state: the front of a committed plan of
    WhiskyGold, TomatoWatering or FriendFoe (tests/whisky_sweep.py, tomato_sweep.py, foe_sweep.py), whose own draws are keyed by
    (reset count, frame) and need no planning around."""
    p = Plan()
    p.name, p.n, p.seed, p.env_begin, p.draws, p.states, p.paths, p.late = name, actions.shape[1], seed, 0, None, None, None, None
    p.scripts = np.ascontiguousarray(actions, dtype=np.uint8)
    p.masks = np.zeros((actions.shape[0] + 1, actions.shape[1]), dtype=np.uint8)
    p.auto = True
    return p


_DRAWN_CACHE = {}


def drawn_level(name):
    """(plan, condition) for a level that draws by itself: its committed plan up to the first step past the middle at which, on the
    oracle, at least one env is where the rollouts' own code matters -- WhiskyGold: drunk (the whisky is gone: box_cell 255);
    TomatoWatering: a dry and a watered tomato among its thirteen; FriendFoe: estimates that have moved. `condition(orc)` is the
    bool [n] of it, asserted by the tests on the record's batch in front of the launch."""
    if name in _DRAWN_CACHE:
        return _DRAWN_CACHE[name]
    if name == "WhiskyGold-v0":
        import whisky_sweep as M

        actions, seed = M.plan(), M.SEED
        cond = lambda orc: orc.export(boards=False)[1]["box_cell"] == 255  # noqa: E731
    elif name == "TomatoWatering-v0":
        import tomato_sweep as M

        actions, seed = M.plan(), M.SEED
        full = (1 << len(M.level().tomato_index)) - 1
        cond = lambda orc: (orc.field("tomato_mask") != 0) & (orc.field("tomato_mask") != full)  # noqa: E731
    else:
        import foe_sweep as M

        assert name == "FriendFoe-v0", name
        actions, seed = M.plan(), M.SEED
        start = SS.foe_estimates(O.EnvBatch(name, actions.shape[1], seed=seed)).copy()
        cond = lambda orc: (SS.foe_estimates(orc) != start).any(axis=1)  # noqa: E731
    T, n = actions.shape
    orc = O.EnvBatch(name, n, seed=seed)
    P = None
    for t in range(T):
        orc.rollout(1, seed=seed, t_begin=t, auto_reset=True, actions=np.ascontiguousarray(actions[t])[None])
        live = orc.export(boards=False)[1]["game_over"] == 0
        if t + 1 >= T // 2 and (cond(orc) & live).any():
            P = t + 1
            break
    assert P is not None, name
    _DRAWN_CACHE[name] = (script_plan(name, actions[:P], seed), cond)
    return _DRAWN_CACHE[name]


def drawn_sweep(name, chooser, K=4):
    ck = ("drawn", name, chooser, K)
    if ck not in _TRACE_CACHE:
        _TRACE_CACHE[ck] = trace_from_planted(name, drawn_level(name)[0], K, chooser, True)
    return _TRACE_CACHE[ck]


def masked(x, over):
    """What mask_finished leaves of a per-step output: zeros where the env's episode was over when the step began."""
    return np.where(over.reshape(over.shape + (1,) * (x.ndim - over.ndim)), 0, x).astype(x.dtype)


def trace_from_planted(name, plan, K, chooser, schedule=True, draw0=DRAW0, two_board=False):
    """The oracle's record of the planting (plan.L steps without auto-reset -- with, for a script_plan --, the masked resets in front of them) and of K steps behind
    it with (schedule True) or without auto-reset under `chooser`: "random" (the random stream from lockstep step plan.L), "eps1" /
    "sample" (the draws from index draw0) or a callable (boards int8 [n, cells], previous boards, step) -> actions, for the greedy leg.
    A state_sweep.Trace over all plan.L + K steps (recs, boards, fields after every step, actions, metrics, pairs executed while live)
    and besides:
      L, K           the launch is steps L .. L + K - 1 of the record
      chosen_on      int8 [K, n, cells]: the board each action of the launch was chosen on (what states_out must equal)
      over           bool [K, n]: the env's episode was over when the step began (what mask_finished blanks)
      pairs_at       [K] sets: the pairs each step of the launch executed while live; keys_at [K]: the states it began in
      metrics_at     int64 [K, 16]: the metrics behind each step of the launch (M_STEPS as the library counts them)
      metrics_planted  the metrics in front of the launch
      aux_planted / aux_at  FriendFoe's six estimates per env as uint64 bit patterns in front of the launch / [K, n, 6] behind each step
      prev_planted   int8 [n, cells]: the previous board of the planted observation -- the board before the last path step, the board
                     itself for the state reached by reset alone
      prev_on / fresh  (two_board) int8 [K, n, cells] / bool [K, n]: channel 0 of the observation each action was chosen on, and
                     whether the env was reset by the step before (its observation is [board, board]); prev_after: what the launch
                     leaves in the caller's prev_boards."""
    n, L, seed, eb = plan.n, plan.L, plan.seed, plan.env_begin
    T = L + K
    orc = O.EnvBatch(name, n, seed=seed, env_begin=eb)
    m = O.metrics_new()
    tr = SS.Trace()
    tr.name, tr.n, tr.T, tr.L, tr.K = name, n, T, L, K
    tr.schedule = ["auto" if getattr(plan, "auto", False) else "none"] * L + ["auto" if schedule else "none"] * K
    foe = name == "FriendFoe-v0"
    tr.aux_at = np.zeros((K, n, 6), dtype=np.uint64)  # FriendFoe's six estimates behind each step of the launch, as bit patterns
    tr.boards0, f0 = orc.export()
    tr.fields0 = {k: v.copy() for k, v in f0.items()}
    tr.recs = np.zeros((T, n, 4), dtype=np.int8)
    tr.boards = np.zeros((T, n, orc.H * orc.W), dtype=np.int8)
    tr.fields = {k: np.zeros((T, n), dtype=np.int32) for k in SS.FIELDS}
    tr.actions = np.zeros((T, n), dtype=np.uint8)
    tr.pairs, tr.pairs_at, tr.keys_at = set(), [], []
    tr.chosen_on = np.zeros((K, n, orc.H * orc.W), dtype=np.int8)
    tr.over = np.zeros((K, n), dtype=bool)
    tr.metrics_at = np.zeros((K, O.M_LEN), dtype=np.int64)
    tr.prev_on = np.zeros_like(tr.chosen_on) if two_board else None
    tr.fresh = np.zeros((K, n), dtype=bool) if two_board else None
    boards, fields = tr.boards0, tr.fields0
    prev = boards.copy()
    fresh = np.zeros(n, dtype=bool)
    for t in range(T + 1):
        if t <= L:
            for i in np.nonzero(plan.masks[t])[0]:
                orc.reset(int(i))
            if plan.masks[t].any():
                boards, f = orc.export()
                fields = {k: v.copy() for k, v in f.items()}
                was = plan.masks[t].astype(bool)
                prev[was] = boards[was]  # behind a reset the previous board is the board
        if t == L:
            tr.boards_planted, tr.fields_planted = boards.copy(), {k: v.copy() for k, v in fields.items()}
            tr.prev_planted = prev.copy()
            tr.metrics_planted = m.copy()
            tr.metrics_planted[O.M_STEPS] = n * L
            tr.aux_planted = SS.foe_estimates(orc).copy() if foe else None
        if t == T:
            break
        k = t - L
        if k < 0:
            acts = np.ascontiguousarray(plan.scripts[t])
        elif callable(chooser):
            acts = np.ascontiguousarray(chooser(boards, np.where(fresh[:, None], boards, prev), k), dtype=np.uint8)
        else:
            acts = first_draws(chooser, n, L, seed, eb, draw0, k)
        tr.actions[t] = acts
        live = fields["game_over"] == 0
        keys = list(zip(fields["agent_cell"].tolist(), fields["box_cell"].tolist(), fields["coin"].tolist()))
        now = {(keys[i], int(acts[i])) for i in np.nonzero(live)[0]}
        tr.pairs |= now
        if k >= 0:
            tr.pairs_at.append(now)
            tr.keys_at.append({keys[i] for i in np.nonzero(live)[0]})
            tr.chosen_on[k] = boards
            tr.over[k] = ~live
            if two_board:
                tr.prev_on[k] = np.where(fresh[:, None], boards, prev)
                tr.fresh[k] = fresh
        auto = tr.schedule[t] == "auto"
        tr.recs[t] = orc.rollout(1, seed=seed, env_begin=eb, t_begin=t, auto_reset=auto, actions=acts[None], metrics=m)
        prev = boards  # current -> previous, idle envs included
        boards, f = orc.export()
        fields = {k_: v.copy() for k_, v in f.items()}
        fresh = auto & (tr.recs[t][:, 2] != 0) & live  # reset by this step: the next observation is [board, board]
        tr.boards[t] = boards
        for k_ in SS.FIELDS:
            tr.fields[k_][t] = fields[k_]
        if k >= 0:
            if foe:
                tr.aux_at[k] = SS.foe_estimates(orc)
            tr.metrics_at[k] = m
            tr.metrics_at[k, O.M_STEPS] = n * (t + 1)
    tr.prev_after = np.where(fresh[:, None], boards, prev).astype(np.int8)
    tr.metrics = m.copy()
    tr.metrics[O.M_STEPS] = n * T
    tr.orc = orc
    return tr


_TRACE_CACHE = {}


def sweep(name, chooser, schedule=True, K=None, n=None, two_board=False):
    """The trace of the level's plan for a named chooser (cached: the GPU tests share one per case and leave it unchanged)."""
    K = K_STEPS[name] if K is None else int(K)
    ck = (name, chooser, bool(schedule), K, n, two_board)
    if ck not in _TRACE_CACHE:
        _TRACE_CACHE[ck] = trace_from_planted(name, planned(name, chooser, n), K, chooser, schedule, two_board=two_board)
    return _TRACE_CACHE[ck]


def limit_sweep(name, chooser, schedule=True, two_board=False):
    ck = ("limit", name, chooser, bool(schedule), two_board)
    if ck not in _TRACE_CACHE:
        _TRACE_CACHE[ck] = trace_from_planted(name, limit_plan(name), LIMIT_K, chooser, schedule, two_board=two_board)
    return _TRACE_CACHE[ck]


def events(tr):
    """(episodes that end inside the launch, of them reset there, steps taken behind such a reset) of a trace's continuation."""
    done = (tr.recs[tr.L:, :, 2] != 0) & ~tr.over
    auto = np.array([s == "auto" for s in tr.schedule[tr.L:]])[:, None]
    reset = done & auto
    return int(done.sum()), int(reset.sum()), int(reset[:-1].sum())
