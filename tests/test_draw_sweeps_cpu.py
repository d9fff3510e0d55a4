"""The planned sweeps of WhiskyGold and FriendFoe without a GPU (tests/whisky_sweep.py, tests/foe_sweep.py): the oracle's record of
the committed plans -- as action scripts and as memoryless policies rewritten between phases -- executes EVERY required event, a
condition, not a measurement; the levels' own draws, recomputed, explain every replaced action, every episode's bandit type and every
level of the records; the time-limit plans end episodes at max_iterations; and the product's host code (sgk_debug_host_step /
sgk_debug_reset_word: the kernels' transition and episode bookkeeping on the packed state word) follows the records state word by
state word -- on FriendFoe the six float64 estimates too, bit for bit, through every episode boundary. test_gpu_draw_sweeps.py holds
the device paths to the same records step by step, which is how the events reach the device.

`python tests/test_draw_sweeps_cpu.py` writes profiles/draw_sweeps/coverage.log."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # run as a script (the report): what tests/conftest.py does for pytest
    sys.path.insert(0, ROOT)

import foe_sweep as FS  # noqa: E402
import hostlib  # noqa: E402
import state_sweep as SS  # noqa: E402
import whisky_sweep as WS  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_tables_cpu import _unpack  # noqa: E402

GRID_N = 65536 + 64 + 37  # the batch of the grid-stride step kernel (test_gpu_draw_sweeps.py)


def _events(mod, tr):
    return WS.events_of(tr, WS.SEED) if mod is WS else FS.events_of(tr)[0]


def _required(mod, form):
    return WS.required() if mod is WS else FS.required(form)


def test_the_committed_choices_are_within_the_size_cap():
    for mod in (WS, FS):
        assert mod.N % 64 != 0 and mod.N <= 520 and mod.T <= 64 and sum(mod.PHASES) <= 64
        assert mod.TL_N <= 70 and mod.TL_N % 64 != 0 and mod.TL_T <= 104
        assert mod.plan().shape == (mod.T, mod.N) and mod.plan().dtype == np.uint8 and int(mod.plan().max()) < 4
        pols = mod.plan_policies()
        assert [steps for steps, _ in pols] == list(mod.PHASES) and len(pols) >= 3
        for _, pol in pols:
            assert pol.shape == (mod.N, SS.n_states(mod.NAME)) and pol.dtype == np.int8 and 0 <= pol.min() and pol.max() < 4
        assert any((a[1] != b[1]).any() for a, b in zip(pols, pols[1:]))  # the tables are rewritten between the launches
    assert len(WS.required()) == 132 + 8 + 1 + 3 + 1 + 3 + 5 and len(FS.required("policy")) == 120 + 12 + 10 + 1


@pytest.mark.parametrize("form", ["actions", "policy"])
@pytest.mark.parametrize("schedule", ["auto", "reset"])
def test_whisky_gold_the_oracles_record_executes_every_event(form, schedule):
    """Every schedule kind a device path is held to: record() has already checked that the recomputed draws explain every executed
    action of it."""
    got = WS.events_of(WS.record(form, schedule), WS.SEED)
    missing = [ev for ev in WS.required() if not got.get(ev)]
    assert not missing, missing


@pytest.mark.parametrize("form", ["actions", "policy"])
@pytest.mark.parametrize("schedule", ["auto", "reset"])
def test_friend_foe_the_oracles_record_executes_every_event(form, schedule):
    """record() has already checked that the recomputed draws and the model estimator explain every type, level and estimate bit."""
    got, depth = FS.events_of(FS.record(form, schedule))
    missing = [ev for ev in FS.required(form) if not got.get(ev)]
    assert not missing, missing
    assert depth == FS.DEPTH[form] >= 6


def test_no_event_is_exempt_in_the_policy_form():
    """Nothing proved unreachable for memoryless policies rewritten between phases: the policy form is held to the full list, and to
    quiet_launch besides."""
    assert set(FS.required("actions")) < set(FS.required("policy"))


def test_the_idle_schedules_are_explained_and_keep_every_event_but_some_pairs():
    """reset_done() behind every 5th step: finished envs idle in between, so fewer episodes fit and the scripts, planned for
    auto-reset, drift off their plan. The requirement is stated on the auto-reset records above; of this one (which env.step's idle
    mode is held to, and which record() explains by the draws like the others) only what it does execute is stated: every event
    that is not a pair, and how many pairs it misses is in profiles/draw_sweeps/coverage.log."""
    for mod in (WS, FS):
        got = _events(mod, mod.record("actions", "idle"))
        missing = [ev for ev in _required(mod, "actions") if ev[0] != "pair" and not got.get(ev)]
        assert not missing, (mod.NAME, missing)


def test_whisky_gold_the_schedule_matrix_is_the_draws():
    sch = WS.schedule(WS.SEED, 5, 12, n_resets=2, env_begin=3)
    assert sch.shape == (13, 5) and sch.min() >= -1 and sch.max() <= 3
    for i in range(5):
        for f in range(1, 13):
            rep, ra = WS.draw_of(WS.SEED, 3 + i, 2, f)
            assert sch[f, i] == (ra if rep else -1)
    assert 0.8 < (WS.schedule(WS.SEED, 40, 40) >= 0)[1:].mean() < 0.97  # nine frames of ten are replaced


def test_whisky_gold_event_counters_on_hand_written_steps():
    L = WS.level()
    up, down, left, right = (L.delta.index(d) for d in (-L.W, L.W, -1, 1))
    A, W, G = L.start, L.whisky, L.goal
    ev = WS.step_events
    # sober: the drink from the start cell, in the first and in a later episode; a plain move; the goal
    assert ev(L, A, 0, right, right, True, up, W, 4, -1, 0, 1, False) == [("pair", A, 0, right), ("drink", A)]
    assert ev(L, A, 0, right, right, False, 0, W, 4, -1, 0, 2, False) == [("pair", A, 0, right), ("drink", A), ("second_episode_drink",)]
    assert ev(L, A, 0, down, down, True, up, A + L.W, -1, -1, 0, 1, False) == [("pair", A, 0, down)]
    assert ev(L, G - 1, 0, right, right, True, up, G, 49, 49, 1, 1, False) == [("pair", G - 1, 0, right), ("goal_sober",)]
    # drunk on the whisky cell right behind the drink: replaced by `up`, into the wall
    assert ev(L, W, 1, right, up, True, up, W, -1, -1, 0, 1, True) == [("pair", W, 1, up), ("replaced", up), ("first_drunk_step_replaced",),
                                                                    ("refused_on_whisky_cell",)]
    # drunk and kept; replaced by the chosen action itself; back onto the empty cell; the goal either way; the time limit
    assert ev(L, W, 1, right, right, False, up, W + 1, -1, -1, 0, 1, True) == [("pair", W, 1, right), ("kept", right)]
    assert ev(L, W + 1, 1, left, left, True, left, W, -1, -1, 0, 1, False) == [("pair", W + 1, 1, left), ("replaced", left), ("replaced_same",),
                                                                            ("rearrive", W + 1)]
    assert ev(L, G - 1, 1, left, right, True, right, G, 49, 49, 1, 1, False) == [("pair", G - 1, 1, right), ("replaced", right),
                                                                              ("goal_drunk_replaced",)]
    assert ev(L, G - 1, 1, right, right, False, 0, G, 49, 49, 1, 1, False) == [("pair", G - 1, 1, right), ("kept", right), ("goal_drunk_kept",)]
    assert ev(L, A, 1, left, left, False, 0, A - 1, -1, -1, 1, 1, False)[-1] == ("timeout_drunk",)
    assert ev(L, A, 0, up, up, False, 0, A, -1, -1, 1, 1, False)[-1] == ("timeout_sober",)


def test_friend_foe_event_counters_on_hand_written_episodes():
    log = FS._EnvLog()
    log.phase_begins()
    assert log.begin(FS.FRIEND) == []
    assert log.opened(FS.FRIEND, 0, 1) == [("open", 0, 0, 1), ("first_of_type", 0)]
    assert log.begin(FS.FRIEND) == [("same_type_twice",)]
    assert log.opened(FS.FRIEND, 1, 0) == [("open", 0, 1, 0), ("friend_level1",)]
    assert log.begin(FS.ADVERSARY) == [("type_change",)]
    assert log.opened(FS.ADVERSARY, 0, 0) == [("open", 2, 0, 0), ("first_of_type", 2)]
    assert log.opened(FS.ADVERSARY, 1, 1) == [("open", 2, 1, 1), ("adversary_level1",)]
    assert log.opened(FS.FRIEND, 0, 0) == [("open", 0, 0, 0), ("flip_back", 0)]
    assert log.timed_out() == [("timeout",), ("timeout_moved",)]
    assert log.opened(FS.NEUTRAL, 1, 1) == [("open", 1, 1, 1), ("all_three",), ("open_after_timeout",)]
    assert log.opened(FS.ADVERSARY, 0, 1) == [("open", 2, 0, 1), ("flip_back", 2), ("all_three",)]
    assert log.phase_ends() == []
    log.phase_begins()
    assert log.phase_ends() == [("quiet_launch",)]
    for k in range(2):  # the friend's estimate has three updates above: the fourth and the fifth
        assert ("depth", 6) not in log.opened(FS.FRIEND, 0, 0)
    assert ("depth", 6) in log.opened(FS.FRIEND, 0, 0)  # the sixth
    fresh = FS._EnvLog()
    fresh.phase_begins()
    assert fresh.timed_out() == [("timeout",)] and fresh.phase_ends() == []
    # the estimator: the level's own numbers
    e = FS.Estimator()
    assert e.level(0, 0) == 0 and e.level(2, 0) == 0 and e.level(1, 1) == 1
    e.update(0, 1)
    e.update(2, 0)
    assert e.p[0] == [0.375, 0.625] and e.level(0, 0) == 1 and e.p[2] == [0.625, 0.375] and e.level(2, 0) == 1
    e.update(0, 0)
    assert e.p[0] == [0.53125, 0.46875] and e.level(0, 0) == 0


def test_friend_foe_the_view_of_the_estimates_is_foe_policy():
    tr = FS.record("actions")
    assert (tr.aux[-1] == tr.orc.foe_policy().reshape(tr.n, 6).view(np.uint64)).all()
    assert (tr.aux[-1] != tr.aux0).any(axis=1).all()  # every env's estimates have moved


@pytest.mark.parametrize("form", ["actions", "policy"])
def test_the_time_limit_plans_end_episodes_at_max_iterations(form):
    """What a time-limit end holds: the step record is (-1, -1, done = 1, the action) -- include/sgk.h does not tell a time limit
    from a terminal state, so this pins the oracle's behaviour, and the replay ring's terminal flag is that done bit --, n_episodes
    advances, and on FriendFoe the estimates keep their bits and the next episode's type is the one recomputed for reset count + 1
    (explain, inside timeout_record)."""
    for mod in (WS, FS):
        tr = mod.timeout_record(form)
        got = _events(mod, tr)
        missing = [ev for ev in mod.required_timeout() if not got.get(ev)]
        assert not missing, (mod.NAME, missing)
        at = (tr.pre["frame"] == mod.MAX_ITERATIONS) & (tr.pre["game_over"] == 1)
        goal = np.isin(tr.pre["agent_cell"], [WS.level().goal] if mod is WS else FS.level().boxes)
        at &= ~goal
        assert at.any()
        t, i = np.nonzero(at)
        assert (tr.recs[t, i, :3] == np.array([-1, -1, 1], dtype=np.int8)).all()
        assert (tr.fields["n_episodes"][t, i] == tr.fields["n_episodes"][t - 1, i] + 1).all() and (tr.fields["frame"][t, i] == 0).all()
        if mod is FS:
            assert (tr.aux[t, i] == tr.aux[t - 1, i]).all()
            assert (tr.aux[t, i] != tr.aux0[i]).any(axis=1).any()  # ... also where they had moved before


def _follow(mod, tr, lib):
    """The host build of the kernels' transition along a record: rewards, done, executed action and every field of the state word
    behind every step and behind every reset; FriendFoe's six doubles bit for bit behind every step."""
    env_id = O.ENV_IDS[mod.NAME]
    f, pre = tr.fields, tr.pre
    out, wout = (ctypes.c_int32 * 4)(), ctypes.c_uint64()
    foe = mod is FS
    for i in range(tr.n):
        aux = (ctypes.c_double * 6)(*([0.5] * 6))
        n_resets = 1
        word = lib.sgk_debug_reset_word(env_id, mod.SEED, i, n_resets, aux)
        types = []
        for t in range(tr.T):
            if _unpack(word)["over"]:  # a finished env idles until the record resets it
                assert tuple(tr.recs[t, i, :3]) == (0, 0, 1), (i, t)
            else:
                if foe and _unpack(word)["frame"] == 0:
                    s = _unpack(word)
                    types.append(s["ext"] & 3)
                    board = tr.boards0[i] if t == 0 else tr.boards[t - 1, i]
                    assert s["ext"] & 3 == int(board.max()) - 5, (i, t)
                assert lib.sgk_debug_host_step(env_id, word, n_resets, int(tr.actions[t, i]), mod.SEED, i, ctypes.byref(wout), out, aux) == 0
                word = wout.value
                assert list(out) == tr.recs[t, i].astype(int).tolist(), (mod.NAME, i, t)
                s = _unpack(word)
                want = {"pos": pre["agent_cell"][t, i], "box": pre["box_cell"][t, i], "frame": pre["frame"][t, i], "over": pre["game_over"][t, i]}
                assert {k: s[k] for k in want} == {k: int(v) for k, v in want.items()}, (mod.NAME, i, t)
            if foe:
                assert np.frombuffer(aux, dtype=np.uint64).tolist() == tr.aux[t, i].tolist(), (i, t)
            if _unpack(word)["over"] and tr.schedule[t] != "none":
                n_resets += 1
                word = lib.sgk_debug_reset_word(env_id, mod.SEED, i, n_resets, aux)
            s = _unpack(word)
            want = {"pos": f["agent_cell"][t, i], "box": f["box_cell"][t, i], "frame": f["frame"][t, i], "over": f["game_over"][t, i],
                    "ret": f["episode_return"][t, i], "hid": f["hidden_return"][t, i]}
            assert {k: s[k] for k in want} == {k: int(v) for k, v in want.items()}, (mod.NAME, i, t)
            assert n_resets == f["n_episodes"][t, i] + 1 - int(f["game_over"][t, i]), (i, t)
        if foe:
            d = FS.draws(mod.SEED, tr.n, 40)
            assert types == d[1:len(types) + 1, i, 0].tolist(), i


@pytest.mark.parametrize("mod", [WS, FS], ids=["WhiskyGold", "FriendFoe"])
@pytest.mark.parametrize("which", ["actions", "policy", "idle", "timeout"])
def test_the_host_code_follows_the_records_state_word_by_state_word(mod, which):
    tr = {"actions": lambda: mod.record("actions"), "policy": lambda: mod.record("policy", "reset"),
          "idle": lambda: mod.record("actions", "idle"), "timeout": lambda: mod.timeout_record("actions")}[which]()
    _follow(mod, tr, hostlib.load())


@pytest.mark.parametrize("mod", [WS, FS], ids=["WhiskyGold", "FriendFoe"])
def test_the_plan_dealt_over_the_grid_stride_batch_begins_with_the_planned_envs(mod):
    """65 637 envs created at env index 0 play the script again and again: the first N are the envs of the record, so every event is
    executed there too (the others are replaced / typed by draws of their own)."""
    small, big = mod.record("actions"), mod.record("actions", copies=-(-GRID_N // mod.N), n=GRID_N)
    assert big.n == GRID_N > 65536 and GRID_N % 64 != 0
    assert (big.recs[:, :mod.N] == small.recs).all() and (big.boards[:, :mod.N] == small.boards).all()
    assert (big.aux[:, :mod.N] == small.aux).all()
    for k in SS.FIELDS:
        assert (big.fields[k][:, :mod.N] == small.fields[k]).all(), k


# ---- the report ------------------------------------------------------------------------------------------------------------------
def _existing_walks(mod):
    """The oracle's replay of the walks the suite took on this level before: {label: record}."""
    import types

    name = mod.NAME
    out = {}
    actions, _, _ = SS.probes(name)
    out["test_gpu_state_sweep: scripts built on env index 0, n=%d T=%d" % actions.shape[::-1]] = (SS.SEED, 0, SS.trace_phases(
        name, SS.SEED, actions.shape[1], [(actions, ["auto"] * actions.shape[0])]))
    n = 1000
    rng = np.random.RandomState(n + len(name))
    acts = np.stack([rng.randint(0, 4, size=n).astype(np.uint8) for _ in range(230)])
    out["test_step_parity_on_given_actions n=1000, 230 steps"] = (0, 0, SS.trace_phases(name, 0, n, [(acts, ["auto"] * 230)]))
    n, seed, base = 1500, 0x5AFE, 4096
    acts = O.random_actions(seed, base, n, 0, 466)
    out["test_random_rollouts_... n=1500, 346 steps + 120 idle"] = (seed, base, SS.trace_phases(
        name, seed, n, [(acts, ["auto"] * 346 + ["none"] * 120)], env_begin=base))
    a = types.SimpleNamespace(lr=0.5, discount=0.99, epsilon=0.05, epsilon_anneal=300)
    n, steps, seed = 200, 700, 21
    orc = O.EnvBatch(name, n, seed=seed)
    agents = [O.TabQ(orc.H * orc.W, a.lr, a.discount, a.epsilon, a.epsilon_anneal) for _ in range(n)]
    acts = O.tabq_rollout(orc, agents, steps, seed=seed, record_actions=True)
    out["test_tabq_fused_rollout_bit_exact n=200, 700 steps"] = (seed, 0, SS.trace_phases(name, seed, n, [(acts, ["auto"] * steps)]))
    return out


def report(path=os.path.join(ROOT, "profiles", "draw_sweeps", "coverage.log")):
    lines = ["# WhiskyGold and FriendFoe: the events tests/whisky_sweep.py and tests/foe_sweep.py require and how many of them a run",
             "# executes, counted on the oracle's record. 'sweep': the committed plans, which tests/test_gpu_draw_sweeps.py holds the device",
             "# paths to step by step. 'walk': the oracle's replay of the walks the suite took on the level before (the columns of",
             "# profiles/state_sweep/coverage.log, in events). depth: the most updates of one estimate of one env.",
             "# written by: python tests/test_draw_sweeps_cpu.py"]

    def row(label, mod, req, got, extra=""):
        kinds = []
        for kind in dict.fromkeys(ev[0] for ev in req):
            mine = [ev for ev in req if ev[0] == kind]
            kinds.append("%s %d/%d" % (kind, sum(1 for ev in mine if got.get(ev)), len(mine)))
        missed = [ev for ev in req if not got.get(ev)]
        lines.append("  %-78s executed %3d of %3d%s" % (label, len(req) - len(missed), len(req), extra))
        lines.append("      " + ", ".join(kinds) + ("" if not missed else "; first missed: %s" % (missed[:4],)))

    for mod in (WS, FS):
        foe = mod is FS
        lines.append("%s: seed %d, N %d, T %d (action scripts), phases %s (policies), planner seed %d%s; time limit: N %d, T %d" % (
            mod.NAME, mod.SEED, mod.N, mod.T, list(mod.PHASES), mod.PLAN_SEED, ", D %s" % (FS.DEPTH,) if foe else "", mod.TL_N, mod.TL_T))
        for form in ("actions", "policy"):
            for schedule in ("auto", "reset", "idle")[: 3 if form == "actions" else 2]:
                tr = mod.record(form, schedule)
                got = _events(mod, tr)
                extra = "  depth %d" % FS.events_of(tr)[1] if foe else ""
                row("sweep %s, %s (n %d, %d steps)" % (form, schedule, tr.n, tr.T), mod, _required(mod, form), got, extra)
            tr = mod.timeout_record(form)
            row("sweep time limit, %s (n %d, %d steps)" % (form, tr.n, tr.T), mod, mod.required_timeout(), _events(mod, tr))
        req = _required(mod, "actions") + mod.required_timeout()
        for label, (seed, base, tr) in _existing_walks(mod).items():
            got = WS.events_of(tr, seed, base) if mod is WS else FS.events_of(tr)[0]
            row("walk  " + label, mod, req, got, "  depth %d" % FS.events_of(tr)[1] if foe else "")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    print("\n".join(report()))
