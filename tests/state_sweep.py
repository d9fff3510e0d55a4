"""Scripted sweeps over every reachable (state, action) of a level -- helper of test_state_sweep_cpu.py and
test_gpu_state_sweep.py. CPU only: the oracle, numpy and the product's host-only library (tests/hostlib.py).

A random walk cannot force a rarely reached state (ConveyorBelt's deepest one needs a 19-step push sequence), so the sweeps do not
walk: `reachable` is a breadth-first search over the oracle's state key (agent cell, second sprite cell, coin / mode bit) that
keeps the shortest action path to every non-terminal state, `probes` gives every reachable (state, action) pair to one env of a
batch -- as an action script (the path, the probed action, zeros) and as a memoryless policy over the product's state index --,
and `trace` is the oracle's record of a batch that follows either: step records, boards and state fields after EVERY step, the
metrics at the end and the set of pairs it executed while the episode was live. A test asserts coverage on that set and holds a
device path to the trace step by step, so that the coverage transfers to the device."""
import ctypes
import types

import numpy as np

import hostlib
from oracle import oracle as O

COIN_ENVS = ("AbsentSupervisor-v0", "SafeInterruptibility-v0")
# the seven levels whose transition is a function of (state, action) alone (the coin being part of the state): the sweep must execute
# every reachable pair of these
SWEPT = ("BoatRace-v0", "IslandNavigation-v0", "SideEffectsSokoban-v0", "DistributionalShift-v0", "AbsentSupervisor-v0",
         "SafeInterruptibility-v0", "ConveyorBelt-v0")
# WhiskyGold replaces actions by its own draws once the whisky is drunk, TomatoWatering and FriendFoe draw every step: the same
# machinery with scripts built on env index 0, no coverage requirement HERE (what they reach is logged). Their requirements are stated in
# events and planned per env around that env's own draws, which never depend on the actions: TomatoWatering's in tests/tomato_sweep.py,
# WhiskyGold's in tests/whisky_sweep.py, FriendFoe's in tests/foe_sweep.py (the latter two: test_draw_sweeps_cpu.py, test_gpu_draw_sweeps.py)
UNSWEPT = ("WhiskyGold-v0", "TomatoWatering-v0", "FriendFoe-v0")
DEPTH_CAP = 98  # the episode limit is 100 steps; the deepest state (ConveyorBelt) is found at depth 19
SEED = 5
# (n, T) per level: n envs hold one probe per pair for either coin with room to spare, T = the deepest path + the probed step + 1;
# no n is a multiple of 64 (every kernel runs a partial last wave on every level), 3 024 = 47 whole waves + 16 lanes
SIZES = {"BoatRace-v0": (130, 6), "IslandNavigation-v0": (225, 8), "SideEffectsSokoban-v0": (497, 16),
         "DistributionalShift-v0": (289, 12), "AbsentSupervisor-v0": (241, 10), "SafeInterruptibility-v0": (515, 13),
         "ConveyorBelt-v0": (3024, 21), "WhiskyGold-v0": (290, 12), "TomatoWatering-v0": (130, 10), "FriendFoe-v0": (130, 8)}
FIELDS = ("episode_return", "hidden_return", "frame", "game_over", "agent_cell", "box_cell", "n_episodes", "last_episode_return",
          "last_performance", "coin")

_BOARD_CACHE = {}


def _board_of_state(env, si, lib=None):
    """Render state index `si` (agent cell, or agent cell * n_cells + box cell) with the product's own level tables, read through
    sgk_debug_level of `lib`: the library under test (the GPU tests pass libsgk.so), or by default the host-only build of the same
    rule tables (tests/hostlib.py), which is what a test without a GPU has."""
    key = (env.name, int(si), None if lib is None else id(lib))
    if key in _BOARD_CACHE:
        return _BOARD_CACHE[key]
    if lib is None:
        lib = hostlib.load()
    dims = (ctypes.c_int32 * 4)()
    templ = (ctypes.c_uint8 * 64)()
    aval = (ctypes.c_uint8 * 64)()
    if lib.sgk_debug_level(O.ENV_IDS[env.name], dims, templ, aval) != 0:
        raise RuntimeError("sgk_debug_level failed")
    nc = env.n_cells
    board = np.array(templ[:nc], dtype=np.int8)
    if env.name == "SideEffectsSokoban-v0":
        cell, box = divmod(int(si), nc)
        board[box] = 4
    elif env.name == "ConveyorBelt-v0":  # (agent cell, object cell); block 0 (a wall cell) = the object arrived: ':' on the end cell
        cell, box = divmod(int(si), nc)
        if box == 0:
            board[3 * env.W + 5] = 4
        else:
            board[box] = 3
    elif env.name == "FriendFoe-v0":  # (agent cell, room type): friend / neutral / adversary floor
        room, cell = divmod(int(si), nc)
        board[(board == 5)] = 5 + room
    elif env.name == "WhiskyGold-v0":  # (agent cell, whisky still there): the drunk half of the table follows the sober one
        drunk, cell = divmod(int(si), nc)
        if not drunk:
            board[dims[3]] = 3
    elif env.name == "AbsentSupervisor-v0":  # (agent cell, supervisor present): the absent half follows the present one
        absent, cell = divmod(int(si), nc)
        if absent:
            board[board == 5] = 1  # the supervisor cells of the border show the blank backdrop
        board[dims[3]] = 3
    elif env.name == "SafeInterruptibility-v0":  # (agent cell, button pressed): the pressed half follows the other
        pressed, cell = divmod(int(si), nc)
        if pressed:
            board[: env.W] = 5  # the top row of B's (value 5); the interruption tile is gone
        else:
            board[dims[3]] = 2  # the interruption tile (value 2)
    else:
        cell = int(si)
    board[cell] = aval[cell]
    _BOARD_CACHE[key] = board
    return board


def n_states(name):
    """Rows of a tabular agent's table on this level (SgkRules.n_states)."""
    import test_tables_cpu as TT

    return int(TT._rules(hostlib.load(), O.ENV_IDS[name]).n_states)


_INDEX_CACHE = {}


def state_index_of_board(name):
    """{board bytes: the product's state index}: _board_of_state inverted over the whole table. (An index whose cells coincide
    renders a board another index owns, or none an env can show; the first index keeps a board, and a reachable board has one.)"""
    if name not in _INDEX_CACHE:
        H, W = O.shape(name)
        env = types.SimpleNamespace(name=name, n_cells=H * W, W=W)
        index = {}
        # WhiskyGold's (sober, on the whisky's cell) is no state -- arriving there drinks --, and it renders the board of (drunk, on that
        # cell), which is one: that board belongs to the drunk index
        no_state = {int(O.EnvBatch(name, 1).field("box_cell")[0])} if name == "WhiskyGold-v0" else set()
        for si in range(n_states(name)):
            if si not in no_state:
                index.setdefault(_board_of_state(env, si).tobytes(), si)
        _INDEX_CACHE[name] = index
    return _INDEX_CACHE[name]


def _key(e):
    return int(e.field("agent_cell")[0]), int(e.field("box_cell")[0]), int(e.field("coin")[0])


_REACH_CACHE = {}


def reachable(name, seed=SEED, env_index=0, depth_cap=DEPTH_CAP):
    """{(agent_cell, box_cell, coin): shortest action path from reset} over every non-terminal state the env `env_index` of a batch
    seeded `seed` can be in during its first episode (its coin is that env's), in breadth-first order."""
    ck = (name, seed, env_index, depth_cap)
    if ck in _REACH_CACHE:
        return _REACH_CACHE[ck]

    def make():
        return O.EnvBatch(name, 1, seed=seed, env_begin=env_index)

    start = _key(make())
    seen = {start: []}
    frontier = [start]
    while frontier:
        nxt = []
        for key in frontier:
            for a in range(4):
                e = make()
                for pa in seen[key]:
                    e.step(0, pa)
                _, _, done, _ = e.step(0, a)
                k2 = _key(e)
                if not done and k2 not in seen and len(seen[key]) < depth_cap:
                    seen[k2] = seen[key] + [a]
                    nxt.append(k2)
        frontier = nxt
    _REACH_CACHE[ck] = seen
    return seen


def reachable_pairs(name, seed=SEED, env_begin=0):
    """{coin: {state: path}} with one search per value of the per-episode coin (one, for levels without), and the set of every
    ((agent_cell, box_cell, coin), action) the level can execute."""
    coin = O.EnvBatch(name, 64, seed=seed, env_begin=env_begin).field("coin")
    if name in UNSWEPT:  # scripts built on env index 0, no deeper than the level's T leaves room for (TomatoWatering's 2^13 masks)
        by_coin = {int(coin[0]): reachable(name, seed, env_begin, SIZES[name][1] - 2)}
    else:
        by_coin = {int(c): reachable(name, seed, env_begin + int(np.nonzero(coin == c)[0][0])) for c in sorted(set(coin.tolist()))}
        assert len(by_coin) == (2 if name in COIN_ENVS else 1), (name, sorted(by_coin))
    pairs = {(s, a) for states in by_coin.values() for s in states for a in range(4)}
    return by_coin, pairs


def lds_resident(name):
    """Whether the tabular-Q kernels that keep the table (rollout) or the policy (evaluate) on the chip take this level: its table
    state is the agent cell alone and at most 32 cells are live (sgk_tabq.hip: tabq_rollout_lds_bytes)."""
    import test_tables_cpu as TT

    R = TT._rules(hostlib.load(), O.ENV_IDS[name])
    return name != "TomatoWatering-v0" and R.n_states == R.n_cells and R.n_live_slots <= 32


def _state_index_along(name, seed, env_index, path, episode=1):
    """The product's state index of every state the env passes on `path` from reset, the one it ends in included."""
    index = state_index_of_board(name)
    e = O.EnvBatch(name, 1, seed=seed, env_begin=env_index)
    for _ in range(episode - 1):
        e.reset()
    out = [index[e.board(0).tobytes()]]
    for a in path:
        e.step(0, a)
        out.append(index[e.board(0).tobytes()])
    return out


_PROBE_CACHE = {}


def probes(name, seed=SEED, n=None, T=None, env_begin=0, with_policy=True, episode=1):
    """One probe per reachable (state, action), dealt to the envs of a batch of n (created with `seed` at `env_begin`) whose
    first-episode coin is the probe's; when every pair has an env the rest take the pairs again, in order.
    Returns (actions uint8 [T, n]: the path, the probed action, zeros; policy int8 [n, n_states] or None: the path's action in the
    path's states, the probed action in the target state, 0 elsewhere -- a shortest path never revisits a state, so an env that
    follows its policy from reset plays its script up to and including the probed step; probe_step int32 [n]: the step that
    executes the probe). episode=2: for a batch that was reset once more before it plays (evaluate() resets: the coins are redrawn)."""
    n = SIZES[name][0] if n is None else int(n)
    T = SIZES[name][1] if T is None else int(T)
    ck = (name, seed, n, T, env_begin, with_policy, episode)
    if ck in _PROBE_CACHE:
        return _PROBE_CACHE[ck]
    by_coin, _ = reachable_pairs(name, seed, env_begin)
    batch = O.EnvBatch(name, n, seed=seed, env_begin=env_begin)
    for _ in range(episode - 1):
        batch.reset()
    coin = batch.field("coin")
    if name in UNSWEPT:
        coin = np.full(n, next(iter(by_coin)), dtype=np.int32)  # every env plays env 0's scripts, whatever it draws itself
    todo = {c: [(s, a) for s in states for a in range(4)] for c, states in by_coin.items()}
    dealt = {c: 0 for c in by_coin}
    actions = np.zeros((T, n), dtype=np.uint8)
    policy = np.zeros((n, n_states(name)), dtype=np.int8) if with_policy else None
    probe_step = np.zeros(n, dtype=np.int32)
    index_memo = {}
    for i in range(n):
        c = int(coin[i])
        s, a = todo[c][dealt[c] % len(todo[c])]
        dealt[c] += 1
        path = by_coin[c][s]
        assert len(path) + 1 <= T, (name, len(path), T)
        actions[: len(path), i] = path
        actions[len(path), i] = a
        probe_step[i] = len(path)
        if with_policy and name not in UNSWEPT:
            if (c, s) not in index_memo:
                index_memo[(c, s)] = _state_index_along(name, seed, env_begin + i, path, episode)
            along = index_memo[(c, s)]
            assert len(set(along)) == len(along), (name, s)  # a shortest path never revisits a state
            for si, pa in zip(along, path + [a]):
                policy[i, si] = pa
    if name in UNSWEPT:
        policy = None
    else:
        for c in by_coin:  # every pair got an env
            assert dealt[c] >= len(todo[c]), (name, c, dealt[c], len(todo[c]))
    _PROBE_CACHE[ck] = (actions, policy, probe_step)
    return _PROBE_CACHE[ck]


def policy_actions(name, boards, policy):
    """What envs showing `boards` [n, n_cells] do under `policy` [n, n_states]: uint8 [n]."""
    index = state_index_of_board(name)
    return np.array([policy[i, index[boards[i].tobytes()]] for i in range(boards.shape[0])], dtype=np.uint8)


class Trace:
    """The oracle's record of a run: recs int8 [T, n, 4], boards int8 [T, n, n_cells] and fields {name: int32 [T, n]} after every
    step (for a step of kind "reset": after the reset behind it; boards_pre: before it), boards0 / fields0 before the first, actions uint8 [T, n] as
    chosen, metrics int64 [16] at the end (M_STEPS as the library counts them: n per lockstep step), pairs = the set of
    ((agent_cell, box_cell, coin), action) executed while the episode was live."""


def trace(name, seed, n, actions=None, policy=None, schedule=True, T=None, env_begin=0, t_begin=0, episode=1):
    """Run the oracle's batch under an action script (`actions` uint8 [T, n]; None with neither: its random actions from lockstep
    step `t_begin`) or a memoryless `policy`. `schedule`: True / False = every step with / without auto-reset; or a list, one
    entry per step: "auto" (auto-reset), "none" (finished envs idle) or "reset" (no auto-reset, reset_done() behind the step)."""
    if T is None:
        T = actions.shape[0]
    if not isinstance(schedule, (list, tuple)):
        schedule = ["auto" if schedule else "none"] * T
    assert len(schedule) == T
    orc = O.EnvBatch(name, n, seed=seed, env_begin=env_begin)
    for _ in range(episode - 1):  # the whole batch reset again before it plays
        orc.reset()
    m = O.metrics_new()
    tr = Trace()
    tr.name, tr.n, tr.T, tr.schedule = name, n, T, list(schedule)
    tr.boards0, f0 = orc.export()
    tr.fields0 = {k: v.copy() for k, v in f0.items()}
    tr.recs = np.zeros((T, n, 4), dtype=np.int8)
    tr.boards = np.zeros((T, n, orc.H * orc.W), dtype=np.int8)
    tr.boards_pre = tr.boards  # the boards between a step and the reset behind it (kind "reset"): an array of its own when one occurs
    if "reset" in schedule:
        tr.boards_pre = np.zeros_like(tr.boards)
    tr.fields = {k: np.zeros((T, n), dtype=np.int32) for k in FIELDS}
    tr.actions = np.zeros((T, n), dtype=np.uint8)
    tr.pairs = set()
    boards, fields = tr.boards0, tr.fields0
    for t in range(T):
        if policy is not None:
            acts = policy_actions(name, boards, policy)
        elif actions is not None:
            acts = np.ascontiguousarray(actions[t], dtype=np.uint8)
        else:
            acts = O.random_actions(seed, env_begin, n, t_begin + t, 1)[0]
        tr.actions[t] = acts
        live = fields["game_over"] == 0
        tr.pairs.update(zip(zip(fields["agent_cell"][live].tolist(), fields["box_cell"][live].tolist(), fields["coin"][live].tolist()),
                            acts[live].tolist()))
        tr.recs[t] = orc.rollout(1, seed=seed, env_begin=env_begin, t_begin=t_begin + t, auto_reset=schedule[t] == "auto",
                                 actions=acts[None], metrics=m)
        if schedule[t] == "reset":
            tr.boards_pre[t] = orc.export()[0]
            for i in np.nonzero(orc.field("game_over"))[0]:
                orc.reset(int(i))
        boards, f = orc.export()
        fields = {k: v.copy() for k, v in f.items()}
        tr.boards[t] = boards
        for k in FIELDS:
            tr.fields[k][t] = fields[k]
    tr.metrics = m.copy()
    tr.metrics[O.M_STEPS] = n * T
    tr.orc = orc  # the batch in its final state (FriendFoe's estimates, last_performance(i))
    return tr


_AUX_OFFSET = []


def foe_estimates(orc):
    """FriendFoe's six float64 estimates of every env of an oracle batch as bit patterns, uint64 [n, 6], in one numpy view of the
    batch's records instead of n calls (65 637 envs x every step). Where the six doubles lie in a record is FOUND, not assumed: the
    bytes of foe_policy() behind one played episode occur exactly once in that env's record; a test holds the view to foe_policy()."""
    if not _AUX_OFFSET:
        e = O.EnvBatch("FriendFoe-v0", 1, seed=1)
        for a in (0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0, 3, 0, 0, 0, 2):  # four shortest episodes: up, up, up, left / right (auto-reset by hand)
            if e.step(0, a)[2]:
                e.reset(0)
        want = e.foe_policy(0).tobytes()
        assert len({x for x in np.frombuffer(want, dtype=np.float64).tolist()}) >= 3
        raw = e.buf.raw[: e.rec]
        at = raw.find(want)
        assert at >= 0 and at % 8 == 0 and raw.find(want, at + 1) < 0
        _AUX_OFFSET.append(at)
    at = _AUX_OFFSET[0]
    raw = np.frombuffer(orc.buf, dtype=np.uint8, count=orc.rec * orc.n).reshape(orc.n, orc.rec)
    return np.ascontiguousarray(raw[:, at:at + 48]).view(np.uint64).reshape(orc.n, 6)


PRE_FIELDS = ("agent_cell", "box_cell", "game_over", "frame", "n_episodes")


def trace_phases(name, seed, n, phases, env_begin=0, pre=True):
    """The oracle's record of ONE batch that plays `phases` one behind the other: a list of (payload, schedule) with payload = an
    action script uint8 [T_p, n] or a memoryless policy int8 [n, n_states], and schedule = one of trace()'s kinds per step of the
    phase ("auto" / "none" / "reset"); (None, "reset_all") between two phases resets the whole batch and the metrics. A Trace over all
    steps as trace() makes it, and besides:
      aux0 / aux   uint64 [n, 6] / [T, n, 6]: FriendFoe's estimates as bit patterns before the first and behind EVERY step
      before       {field of PRE_FIELDS, "n_resets": int32 [T, n]} and boards_before: the state every step starts from, and how often
                   the env has been reset by then
      pre          {field of PRE_FIELDS: int32 [T, n]} and boards_pre: the state a step leaves BEFORE the reset that may follow it
                   (`pre`: every "auto" step is played as the step and the resets of the finished envs, which is what auto-reset means;
                   pre=False plays it in one call of the oracle -- a batch of 65 637 envs -- and leaves these four out)
      phase_end    the index of every phase's last step; metrics_at: the metrics behind it (M_STEPS as the library counts them)."""
    orc = O.EnvBatch(name, n, seed=seed, env_begin=env_begin)
    foe = name == "FriendFoe-v0"
    T = sum(len(sch) for payload, sch in phases if payload is not None)
    m, t_metrics = O.metrics_new(), 0
    tr = Trace()
    tr.name, tr.n, tr.T, tr.schedule = name, n, T, [k for payload, sch in phases if payload is not None for k in sch]
    tr.boards0, f0 = orc.export()
    tr.fields0 = {k: v.copy() for k, v in f0.items()}
    tr.recs = np.zeros((T, n, 4), dtype=np.int8)
    tr.boards = np.zeros((T, n, orc.H * orc.W), dtype=np.int8)
    tr.boards_pre = np.zeros_like(tr.boards) if pre else None
    tr.fields = {k: np.zeros((T, n), dtype=np.int32) for k in FIELDS}
    tr.pre = {k: np.zeros((T, n), dtype=np.int32) for k in PRE_FIELDS} if pre else None
    tr.before = {k: np.zeros((T, n), dtype=np.int32) for k in PRE_FIELDS + ("n_resets",)} if pre else None
    n_resets = np.ones(n, dtype=np.int32)  # counted here, reset by reset (the create-time reset is number 1): what keys the draws
    tr.boards_before = np.zeros_like(tr.boards) if pre else None
    tr.actions = np.zeros((T, n), dtype=np.uint8)
    tr.aux0 = foe_estimates(orc) if foe else np.zeros((n, 6), dtype=np.uint64)
    tr.aux = np.zeros((T, n, 6), dtype=np.uint64)
    tr.phase_end, tr.metrics_at = [], []
    boards, f = tr.boards0, tr.fields0
    t = 0
    for payload, sch in phases:
        if payload is None:  # (None, "reset_all"): the whole batch is reset and the metrics start again -- what evaluate() does first
            assert sch == "reset_all"
            orc.reset()
            n_resets += 1
            m, t_metrics = O.metrics_new(), t
            boards, f = orc.export()
            continue
        script = payload.dtype == np.uint8
        assert payload.shape == ((len(sch), n) if script else (n, n_states(name))), payload.shape
        for j, kind in enumerate(sch):
            acts = np.ascontiguousarray(payload[j]) if script else policy_actions(name, boards, payload)
            tr.actions[t] = acts
            if pre:
                tr.boards_before[t] = boards
                for k in PRE_FIELDS:
                    tr.before[k][t] = f[k]
                tr.before["n_resets"][t] = n_resets
            tr.recs[t] = orc.rollout(1, seed=seed, env_begin=env_begin, t_begin=t, auto_reset=kind == "auto" and not pre,
                                     actions=acts[None], metrics=m)
            if pre:
                tr.boards_pre[t], fp = orc.export()
                for k in PRE_FIELDS:
                    tr.pre[k][t] = fp[k]
                if kind != "none":
                    for i in np.nonzero(fp["game_over"])[0]:
                        orc.reset(int(i))
                        n_resets[i] += 1
            elif kind == "reset":
                for i in np.nonzero(orc.field("game_over"))[0]:
                    orc.reset(int(i))
            boards, f = orc.export()
            tr.boards[t] = boards
            for k in FIELDS:
                tr.fields[k][t] = f[k]
            if foe:
                tr.aux[t] = foe_estimates(orc)
            t += 1
        tr.phase_end.append(t - 1)
        mm = m.copy()
        mm[O.M_STEPS] = n * (t - t_metrics)
        tr.metrics_at.append(mm)
    tr.metrics = tr.metrics_at[-1].copy()
    tr.orc = orc
    return tr


def sweep(name, form="actions", schedule=True, seed=SEED, n=None, T=None, episode=1):
    """The trace of the level's probes in either form (cached: the GPU tests share one per (level, form, schedule))."""
    sk = tuple(schedule) if isinstance(schedule, (list, tuple)) else bool(schedule)
    ck = (name, form, sk, seed, n, T, episode)
    if ck not in _SWEEP_CACHE:
        actions, policy, _ = probes(name, seed, n, T, episode=episode)
        n_, T_ = actions.shape[1], actions.shape[0]
        if form == "policy":
            assert policy is not None, "%s has no scripted policy" % name
            T_ = len(schedule) if isinstance(schedule, (list, tuple)) else T_
            _SWEEP_CACHE[ck] = trace(name, seed, n_, policy=policy, schedule=schedule, T=T_, episode=episode)
        else:
            _SWEEP_CACHE[ck] = trace(name, seed, n_, actions=actions, schedule=schedule, episode=episode)
    return _SWEEP_CACHE[ck]


_SWEEP_CACHE = {}


def coverage(name, tr, seed=SEED):
    """(reachable states, reachable pairs, pairs of them the trace executed)."""
    by_coin, pairs = reachable_pairs(name, seed)
    return sum(len(s) for s in by_coin.values()), len(pairs), len(pairs & tr.pairs)
