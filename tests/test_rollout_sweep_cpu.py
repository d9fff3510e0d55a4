"""The planned sweeps of the self-acting rollouts without a GPU (tests/rollout_sweep.py): the conditions test_gpu_rollout_sweep.py
stands on, asserted on the oracle alone so that the coverage transfers to the device.

  - at the n, the lockstep step and the draw index the GPU tests use, the FIRST step of the launch executes EVERY reachable
    (agent cell, second sprite cell, coin / mode bit, action) of each of the seven deterministic levels, under each of the three
    choosers (the random stream, epsilon 1, four equal logits) -- a condition, with no exemption list;
  - the planting (scripts through env.step, masked resets) leaves every env in the state it was dealt, as the key and as the board;
  - the product's host code (sgk_debug_host_step / sgk_debug_reset_word) follows the whole record, planting, masked resets and the
    continuation's auto-resets included, state word by state word;
  - the K-step continuation of every level ends an episode, resets it and steps again inside the launch;
  - the time-limit leg ends episodes at max_iterations inside the launch, not by a terminal cell;
  - the greedy leg (epsilon 0, integer weights: float32 is exact, tests/forward_reference.py) shows the network every reachable state
    at step 0 and takes more than one action there.

`python tests/test_rollout_sweep_cpu.py` writes profiles/rollout_sweep/coverage.log."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # run as a script (the report): what tests/conftest.py does for pytest
    sys.path.insert(0, ROOT)

import hostlib  # noqa: E402
import rollout_sweep as RS  # noqa: E402
import state_sweep as SS  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_tables_cpu import _unpack  # noqa: E402


def test_the_batch_sizes():
    for name in SS.SWEPT:
        n, M = RS.N[name], RS.MEMBERS[name]
        assert n % 64 != 0 and n <= SS.SIZES[name][0], name
        assert M > 1 and n % M == 0, name
        assert 4 <= RS.K_STEPS[name] <= 8, name
    assert max(RS.N.values()) == RS.N["ConveyorBelt-v0"] == 3024


@pytest.mark.parametrize("chooser", RS.CHOOSERS)
@pytest.mark.parametrize("name", SS.SWEPT)
def test_step_0_of_the_launch_executes_every_reachable_pair(name, chooser):
    by_coin, pairs = SS.reachable_pairs(name)
    for schedule in (True, False):
        tr = RS.sweep(name, chooser, schedule)
        assert not tr.over[0].any()  # every env is live at the launch
        assert pairs <= tr.pairs_at[0], (name, chooser, sorted(pairs - tr.pairs_at[0])[:5])
        assert tr.keys_at[0] == {s for states in by_coin.values() for s in states}
    plan = RS.planned(name, chooser)
    assert plan.L == RS.launch_step(name) and (plan.masks.sum(axis=0) == 1).all()  # every env is reset exactly once by mask
    assert (tr.actions[plan.L] == plan.draws).all()
    # every member of the population rollouts holds more than one drawn action (and both coins where there are two)
    E = plan.n // RS.MEMBERS[name]
    for m in range(RS.MEMBERS[name]):
        mine = range(m * E, (m + 1) * E)
        assert len({int(plan.draws[i]) for i in mine}) > 1, (name, chooser, m)
        assert name not in SS.COIN_ENVS or len({plan.states[i][2] for i in mine}) == 2, (name, chooser, m)
        assert len({plan.states[i] for i in mine}) > 1, (name, chooser, m)


def test_plant_refuses_a_class_that_is_too_small():
    name = "ConveyorBelt-v0"
    with pytest.raises(AssertionError, match=r"ConveyorBelt-v0: the class \(coin \d+, action \d\)"):
        RS.plant(name, RS.first_draws("random", 1000, RS.launch_step(name)))


_STATE_BOARDS = {}


def _board_of(name, plan, i):
    """The oracle's board of the state dealt to env i, from an env of its own that walks the SHORTEST path in its second episode."""
    s = plan.states[i]
    if (name, s) not in _STATE_BOARDS:
        by_coin, _ = SS.reachable_pairs(name)
        e = O.EnvBatch(name, 1, seed=plan.seed, env_begin=plan.env_begin + i)
        e.reset()
        assert name not in SS.COIN_ENVS or int(e.field("coin")[0]) == s[2]
        for a in next(states[s] for states in by_coin.values() if s in states):
            assert not e.step(0, a)[2]
        assert SS._key(e) == s
        _STATE_BOARDS[(name, s)] = e.board(0).reshape(-1).copy()
    return _STATE_BOARDS[(name, s)]


@pytest.mark.parametrize("chooser", RS.CHOOSERS)
@pytest.mark.parametrize("name", SS.SWEPT)
def test_the_planting_reproduces_the_dealt_states(name, chooser):
    plan, tr = RS.planned(name, chooser), RS.sweep(name, chooser)
    f = tr.fields_planted
    got = list(zip(f["agent_cell"].tolist(), f["box_cell"].tolist(), f["coin"].tolist()))
    assert got == plan.states
    assert not f["game_over"].any()
    assert (f["frame"] == [len(p) for p in plan.paths]).all()
    assert (f["frame"][plan.late] == RS.launch_step(name)).all() and plan.late.any() == RS.endless(name)
    for i in range(plan.n):
        assert (tr.boards_planted[i] == _board_of(name, plan, i)).all(), (name, i, plan.states[i])
    # the previous board of the planted observation: the board itself where the env was reset last, else the board one step earlier
    last = plan.masks[plan.L].astype(bool)
    assert last.any() and (tr.prev_planted[last] == tr.boards_planted[last]).all()
    for i in np.nonzero(~last)[0]:
        if len(plan.paths[i]) >= 2:
            assert (tr.prev_planted[i] == tr.boards[plan.L - 2, i]).all(), (name, i)
        else:  # one step behind the masked reset: the second episode's first board
            e = O.EnvBatch(name, 1, seed=plan.seed, env_begin=plan.env_begin + i)
            e.reset()
            assert (tr.prev_planted[i] == e.board(0).reshape(-1)).all(), (name, i)


def _follow(name, plan, tr, envs):
    """sgk_debug_host_step / sgk_debug_reset_word along the record of `envs`."""
    lib = hostlib.load()
    env_id = O.ENV_IDS[name]
    f = tr.fields
    out, wout = (ctypes.c_int32 * 4)(), ctypes.c_uint64()
    for i in envs:
        aux = (ctypes.c_double * 6)(*([0.5] * 6))
        n_resets = 1
        word = lib.sgk_debug_reset_word(env_id, plan.seed, plan.env_begin + i, n_resets, aux)
        for t in range(tr.T):
            if t <= plan.L and plan.masks[t, i]:
                n_resets += 1
                word = lib.sgk_debug_reset_word(env_id, plan.seed, plan.env_begin + i, n_resets, aux)
            if _unpack(word)["over"]:  # a finished env idles until the record resets it
                assert tuple(tr.recs[t, i, :3]) == (0, 0, 1), (name, i, t)
            else:
                assert lib.sgk_debug_host_step(env_id, word, n_resets, int(tr.actions[t, i]), plan.seed, plan.env_begin + i, ctypes.byref(wout),
                                               out, aux) == 0
                word = wout.value
                assert list(out) == tr.recs[t, i].astype(int).tolist(), (name, i, t)
                if tr.schedule[t] == "auto" and _unpack(word)["over"]:
                    n_resets += 1
                    word = lib.sgk_debug_reset_word(env_id, plan.seed, plan.env_begin + i, n_resets, aux)
            s = _unpack(word)
            want = {"pos": f["agent_cell"][t, i], "box": f["box_cell"][t, i], "frame": f["frame"][t, i], "over": f["game_over"][t, i],
                    "ret": f["episode_return"][t, i], "hid": f["hidden_return"][t, i], "mode": f["coin"][t, i]}
            assert {k: s[k] for k in want} == {k: int(v) for k, v in want.items()}, (name, i, t)


@pytest.mark.parametrize("chooser", RS.CHOOSERS)
@pytest.mark.parametrize("name", SS.SWEPT)
def test_the_host_code_follows_the_record_state_word_by_state_word(name, chooser):
    plan, tr = RS.planned(name, chooser), RS.sweep(name, chooser)
    _follow(name, plan, tr, range(plan.n))


@pytest.mark.parametrize("chooser", RS.CHOOSERS)
@pytest.mark.parametrize("name", SS.SWEPT)
def test_the_continuation_ends_resets_and_steps_again(name, chooser):
    tr = RS.sweep(name, chooser, True)
    assert tr.K == RS.K_STEPS[name]
    ended, reset, behind = RS.events(tr)
    assert ended > 0 and reset > 0 and behind > 0, (name, chooser, ended, reset, behind)
    ended, reset, behind = RS.events(RS.sweep(name, chooser, False))
    assert ended > 0 and reset == 0 and behind == 0  # without auto-reset the finished envs idle: mask_finished has something to blank
    assert RS.sweep(name, chooser, False).over[1:].any()


@pytest.mark.parametrize("chooser", RS.CHOOSERS)
@pytest.mark.parametrize("name", RS.LIMIT_LEVELS)
def test_the_time_limit_leg_ends_episodes_by_the_limit_inside_the_launch(name, chooser):
    plan = RS.limit_plan(name)
    tr = RS.limit_sweep(name, chooser, True)
    L = plan.L
    assert L == RS.MAX_ITERATIONS - RS.LIMIT_BEFORE and not plan.masks.any()
    assert not tr.recs[:L, :, 2].any()  # no env terminates on the way
    assert (tr.fields_planted["frame"] == L).all() and len({b.tobytes() for b in tr.boards_planted}) > 4
    # the step that takes frame 99 to 100 ends the episode of every env that is still in it, and for some of them nothing else does:
    # the state and action of that step do not end a fresh episode (on BoatRace, where no step does, that is every env)
    k = RS.LIMIT_BEFORE - 1
    at = tr.fields["frame"][L + k - 1] == RS.MAX_ITERATIONS - 1
    assert at.any() and (tr.recs[L + k, at, 2] == 1).all()
    f = {key: v[L + k - 1] for key, v in tr.fields.items()}
    by_limit = [i for i in np.nonzero(at)[0]
                if int(tr.actions[L + k, i]) in plan.safe[(int(f["agent_cell"][i]), int(f["box_cell"][i]), int(f["coin"][i]))]]
    assert by_limit, name
    if RS.endless(name):
        assert len(by_limit) == plan.n
    assert min(RS.events(tr)) > 0
    _follow(name, plan, tr, range(0, plan.n, 7))


# ---- the levels that draw by themselves -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chooser", RS.CHOOSERS)
@pytest.mark.parametrize("name", SS.UNSWEPT)
def test_the_drawn_levels_launch_where_their_own_state_matters(name, chooser):
    """No coverage requirement (theirs stay in their own sweeps): the committed plan is played to a mid-plan step at which at least one
    live env is drunk (WhiskyGold) / has a dry and a watered tomato (TomatoWatering) / has moved estimates (FriendFoe)."""
    plan, cond = RS.drawn_level(name)
    tr = RS.drawn_sweep(name, chooser)
    assert plan.auto and not plan.masks.any() and plan.scripts.shape[0] // 2 <= plan.L
    orc = O.EnvBatch(name, plan.n, seed=plan.seed)
    for t in range(plan.L):
        orc.rollout(1, seed=plan.seed, t_begin=t, auto_reset=True, actions=plan.scripts[t][None])
    assert (orc.export()[0] == tr.boards_planted).all()
    assert (cond(orc) & (tr.fields_planted["game_over"] == 0)).any(), name
    if name == "FriendFoe-v0":
        assert (tr.aux_at[-1] != tr.aux_planted).any()  # the estimates go on moving inside the launch


# ---- the greedy leg ----------------------------------------------------------------------------------------------------------------
GREEDY_WIDTH = {"mlp": 100, "cnn": 5, "trans": 5}
_GREEDY = {}


def greedy_sweep(name, body, schedule=True):
    """(weights, trace) of the greedy leg: the level's "eps1" plan continued K steps by the float64 argmax (the first maximum) of the
    body's forward with integer weights ON THE ORACLE'S boards -- "mlp" / "cnn": forward_reference, "trans": the two-board body of
    transition_reference on [previous board, board]. The weights' seed is the first from 8800 on under which two actions are each
    taken by at least 2 % of the envs at step 0 (a policy with arbitrary weights often takes one action on every board of a level)."""
    import forward_reference as FR
    import transition_reference as TR

    ck = (name, body, bool(schedule))
    if ck in _GREEDY:
        return _GREEDY[ck]
    shape, width = O.shape(name), GREEDY_WIDTH[body]
    plan = RS.planned(name, "eps1")

    def weights(seed):
        if body == "mlp":
            return FR.mlp_weights("integer", shape[0] * shape[1], width, seed)
        return FR.cnn_weights("integer", shape, width, seed) if body == "cnn" else TR.weights("integer", width, seed)

    def chooser(w):
        if body == "trans":
            return lambda boards, prev, k: TR.forward(prev, boards, w).argmax(1)
        return lambda boards, prev, k: FR.forward(body, boards, w, shape).argmax(1)

    seed = _GREEDY.get((name, body, "seed"))
    if seed is None:
        for seed in range(8800, 8900):
            first = RS.trace_from_planted(name, plan, 1, chooser(weights(seed)), True, two_board=body == "trans")
            if (np.bincount(first.actions[plan.L], minlength=4) >= 0.02 * plan.n).sum() >= 2:
                break
        else:
            raise AssertionError("no seed of 100 takes two actions on %s" % name)
        _GREEDY[(name, body, "seed")] = seed
    w = weights(seed)
    tr = RS.trace_from_planted(name, plan, RS.K_STEPS[name], chooser(w), schedule, two_board=body == "trans")
    if body == "trans":
        tr.abs_sum = max(TR.abs_sum_bound(tr.prev_on[k], tr.chosen_on[k], w) for k in range(tr.K))
    else:
        tr.abs_sum = max(FR.abs_sum_bound(body, tr.chosen_on[k], w, shape) for k in range(tr.K))
    _GREEDY[ck] = (w, tr)
    return _GREEDY[ck]


# (the two-board body exists for BoatRace's board alone: transition_reference.LEVEL)
@pytest.mark.parametrize("name,body", [(n, b) for n in SS.SWEPT for b in ("mlp", "cnn")] + [("BoatRace-v0", "trans")])
def test_the_greedy_leg_shows_the_network_every_reachable_state(name, body):
    import forward_reference as FR

    by_coin, _ = SS.reachable_pairs(name)
    for schedule in (True, False):
        w, tr = greedy_sweep(name, body, schedule)
        assert tr.keys_at[0] == {s for states in by_coin.values() for s in states}
        assert (np.bincount(tr.actions[tr.L], minlength=4) >= 0.02 * tr.n).sum() >= 2
        assert tr.abs_sum < FR.EXACT_LIMIT  # every partial sum is an integer float32 holds: the kernel's argmax must EQUAL float64's


# ---- the report ------------------------------------------------------------------------------------------------------------------
DEVICE_PATHS = {"random": "rollout_random (outputs once; streamed into slice- / tile-major rings and the env's own buffers)",
                "eps1": "policy_rollout(_members) / convq_rollout(_members, _trans) mode greedy, epsilon 1",
                "sample": "policy_rollout(_members) / convq_rollout(_members, _trans) mode sample, zero actor head"}


def report(path=os.path.join(ROOT, "profiles", "rollout_sweep", "coverage.log")):
    lines = ["# Reachable (state, action) pairs per level (tests/state_sweep.py, seed %d) and how many of them STEP 0 of a launch executes" % SS.SEED,
             "# from the planted states of tests/rollout_sweep.py, per chooser = per family of device paths test_gpu_rollout_sweep.py holds to",
             "# that record; then the events of the K-step continuation with auto-reset: episodes that end inside the launch, of them",
             "# reset there, steps taken behind such a reset. 'late': envs that hold their state at frame 97 (endless levels).",
             "# written by: python tests/test_rollout_sweep_cpu.py"]
    for name in SS.SWEPT:
        by_coin, pairs = SS.reachable_pairs(name)
        lines.append("%s: states %d pairs %d depth %d  (n %d, launch at lockstep step %d, K %d, members %d)"
                     % (name, sum(len(s) for s in by_coin.values()), len(pairs), RS.depth(name), RS.N[name], RS.launch_step(name),
                        RS.K_STEPS[name], RS.MEMBERS[name]))
        for chooser in RS.CHOOSERS:
            tr, plan = RS.sweep(name, chooser, True), RS.planned(name, chooser)
            lines.append("  %-7s step 0 executed %4d of %4d  late %4d  ended %4d reset %4d stepped behind %4d   %s"
                         % ((chooser, len(pairs & tr.pairs_at[0]), len(pairs), int(plan.late.sum())) + RS.events(tr) + (DEVICE_PATHS[chooser],)))
    for name in RS.LIMIT_LEVELS:
        for chooser in RS.CHOOSERS:
            tr = RS.limit_sweep(name, chooser, True)
            lines.append("%s time-limit leg %-7s launch at frame %d, K %d: ended %d reset %d stepped behind %d"
                         % ((name, chooser, tr.L, tr.K) + RS.events(tr)))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    print("\n".join(report()))
