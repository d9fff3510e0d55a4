"""The scripted state sweeps without a GPU (tests/state_sweep.py): on the seven deterministic levels the oracle's trace of the
probes executes EVERY reachable (agent cell, second sprite cell, coin / mode bit, action) -- a condition, not a measurement --, in
the action form and in the policy form, and the product's host code (sgk_debug_host_step: the kernels' transition and episode
bookkeeping on the packed state word) follows the same trace state word by state word. test_gpu_state_sweep.py holds every
scriptable device path to these traces step by step, which is how the coverage reaches the board writers and state carriers of
the device. WhiskyGold, TomatoWatering and FriendFoe draw by themselves: they run the same machinery with scripts built on env
index 0 and carry no coverage requirement here (theirs: test_tomato_sweep_cpu.py, test_draw_sweeps_cpu.py).

`python tests/test_state_sweep_cpu.py` writes profiles/state_sweep/coverage.log: per level the reachable states and pairs, what
the sweeps execute, and for comparison what the oracle's replay of the suite's own walks executes."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # run as a script (the report): what tests/conftest.py does for pytest
    sys.path.insert(0, ROOT)

import hostlib  # noqa: E402
import state_sweep as SS  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_tables_cpu import _unpack  # noqa: E402


def _idle_schedule(T):
    """No auto-reset, reset_done() behind every 5th step: finished envs idle in between (test_gpu_state_sweep.py drives it too)."""
    return ["reset" if t % 5 == 4 else "none" for t in range(T)]


@pytest.mark.parametrize("name", SS.SWEPT)
def test_the_action_script_executes_every_reachable_pair(name):
    by_coin, pairs = SS.reachable_pairs(name)
    assert len(by_coin) == (2 if name in SS.COIN_ENVS else 1)
    assert max(len(p) for states in by_coin.values() for p in states.values()) + 2 <= SS.SIZES[name][1] <= 21
    assert len(pairs) >= 32
    for schedule in (True, False, _idle_schedule(SS.SIZES[name][1])):
        tr = SS.sweep(name, "actions", schedule)
        assert pairs <= tr.pairs, (name, schedule, sorted(pairs - tr.pairs)[:5])
    actions, _, probe_step = SS.probes(name)
    assert not actions[probe_step.max() + 1:].any()  # the path, the probed action, then zeros


@pytest.mark.parametrize("name", SS.SWEPT)
def test_the_policy_form_plays_the_script(name):
    """An env that follows its memoryless policy from reset plays its script up to and including the probed step (a shortest path
    never revisits a state): same actions, records, boards and fields there. Behind the probe the script plays zeros and the
    policy goes on by its table, so each form has its own trace from then on; both execute every pair."""
    _, pairs = SS.reachable_pairs(name)
    actions, policy, probe_step = SS.probes(name)
    assert policy.shape == (SS.SIZES[name][0], SS.n_states(name)) and policy.dtype == np.int8
    for schedule in (True, False):
        ta, tp = SS.sweep(name, "actions", schedule), SS.sweep(name, "policy", schedule)
        assert pairs <= tp.pairs, (name, sorted(pairs - tp.pairs)[:5])
        upto = np.arange(ta.T)[:, None] <= probe_step[None, :]  # [T, n]
        assert (ta.actions == tp.actions)[upto].all()
        assert (ta.recs == tp.recs)[upto].all()
        assert (ta.boards == tp.boards)[upto].all()
        for k in SS.FIELDS:
            assert (ta.fields[k] == tp.fields[k])[upto].all(), k


@pytest.mark.parametrize("name", SS.SWEPT + SS.UNSWEPT)
def test_the_host_code_follows_the_trace_state_word_by_state_word(name):
    lib = hostlib.load()
    env_id = O.ENV_IDS[name]
    tr = SS.sweep(name, "actions", False)
    f = tr.fields
    out, wout = (ctypes.c_int32 * 4)(), ctypes.c_uint64()
    for i in range(tr.n):
        aux = (ctypes.c_double * 6)(*([0.5] * 6))
        word = lib.sgk_debug_reset_word(env_id, SS.SEED, i, 1, aux)
        for t in range(tr.T):
            assert lib.sgk_debug_host_step(env_id, word, 1, int(tr.actions[t, i]), SS.SEED, i, ctypes.byref(wout), out, aux) == 0
            word = wout.value
            assert list(out) == tr.recs[t, i].astype(int).tolist(), (name, i, t)
            s = _unpack(word)
            want = {"pos": f["agent_cell"][t, i], "box": f["box_cell"][t, i], "frame": f["frame"][t, i], "over": f["game_over"][t, i],
                    "ret": f["episode_return"][t, i], "hid": f["hidden_return"][t, i]}
            assert {k: s[k] for k in want} == {k: int(v) for k, v in want.items()}, (name, i, t)
            if name not in ("FriendFoe-v0", "TomatoWatering-v0"):
                assert s["mode"] == int(f["coin"][t, i]), (name, i, t)


def test_the_unswept_levels_run_the_same_machinery():
    """No coverage requirement: what the scripts of env index 0 reach on the levels that draw by themselves is logged."""
    for name in SS.UNSWEPT:
        tr = SS.sweep(name, "actions", True)
        states, pairs, hit = SS.coverage(name, tr)
        print("%s: %d states and %d pairs within the scripts' depth, %d executed" % (name, states, pairs, hit))
        assert 0 < hit <= pairs


def test_the_oracles_draws_have_period_2_to_the_32():
    """The oracle's half of a pin of tests/test_gpu_counter_horizons.py, which holds the device to these functions at the same
    indices: only the low 32 bits of a draw index reach the counter (sgk_draws.h: ctr = {env_lo, env_hi, draw, stream}), so draw
    2^32 + 5 is draw 5 and 2^32 and 2^63 are draw 0."""
    seed, base = 0xBEEF, (1 << 33) + 12345
    sc = np.stack([np.random.RandomState(k).permutation(4) for k in range(64)]).astype(np.float32)
    zeros = np.zeros((64, 4), dtype=np.float32)
    for a, b in ((2**32 + 5, 5), (2**32, 0), (2**63, 0)):
        assert (O.eps_greedy(sc, 0.5, seed, base, a) == O.eps_greedy(sc, 0.5, seed, base, b)).all()
        assert (O.categorical_sample(zeros, seed, base, a)[0] == O.categorical_sample(zeros, seed, base, b)[0]).all()
    assert (O.eps_greedy(sc, 0.5, seed, base, 2**32 - 1) != O.eps_greedy(sc, 0.5, seed, base, 2**32)).any()


# ---- the report ------------------------------------------------------------------------------------------------------------------
def _existing_walks(name):
    """The oracle's replay of the walks the suite already takes on the device: {label: set of executed pairs}."""
    out = {}
    n = 1000
    rng = np.random.RandomState(n + len(name))
    acts = np.stack([rng.randint(0, 4, size=n).astype(np.uint8) for _ in range(230)])
    out["test_step_parity_on_given_actions n=1000"] = SS.trace(name, 0, n, actions=acts, schedule=True).pairs
    n, seed, base = 1500, 0x5AFE, 4096
    tr = SS.trace(name, seed, n, schedule=["auto"] * 346 + ["none"] * 120, T=466, env_begin=base)
    out["test_random_rollouts_... n=1500"] = tr.pairs
    import types

    a = types.SimpleNamespace(lr=0.5, discount=0.99, epsilon=0.05, epsilon_anneal=300)
    n, steps, seed = 200, 700, 21
    orc = O.EnvBatch(name, n, seed=seed)
    agents = [O.TabQ(orc.H * orc.W, a.lr, a.discount, a.epsilon, a.epsilon_anneal) for _ in range(n)]
    acts = O.tabq_rollout(orc, agents, steps, seed=seed, record_actions=True)
    out["test_tabq_fused_rollout_bit_exact"] = SS.trace(name, seed, n, actions=acts, schedule=True).pairs
    return out


def device_paths(name):
    """(device path, form, schedule, episode) of every trace tests/test_gpu_state_sweep.py holds a device path to on this level."""
    T = SS.SIZES[name][1]
    out = [("env.step pitched / compact, auto-reset", "actions", True, 1),
           ("env.step pitched / compact, reset_done() every 5th step", "actions", _idle_schedule(T), 1)]
    if name in ("BoatRace-v0", "IslandNavigation-v0", "AbsentSupervisor-v0", "ConveyorBelt-v0"):  # test_gpu_state_sweep.SERVER_LEVELS
        out += [("sgk_step_host (step server, <= 64 envs), auto-reset", "actions", True, 1),
                ("sgk_step_host (step server), reset_done() every 5th", "actions", _idle_schedule(T), 1)]
    if name in SS.SWEPT:
        kernels = "lds / hbm" if SS.lds_resident(name) else "hbm"
        out += [("step_store + reset_done_store, rings of 5", "actions", ["reset"] * T, 1),
                ("tabq act + env.step, auto-reset", "policy", True, 1),
                ("tabq act + env.step, no reset", "policy", False, 1),
                ("tabq step / learn_steps / rollout %s" % kernels, "policy", ["reset"] * T, 1),
                ("tabq evaluate %s (second episode's coins)" % kernels, "policy", ["reset"] * T + ["none"] * 100, 2)]
    return out


def report(path=os.path.join(ROOT, "profiles", "state_sweep", "coverage.log")):
    lines = ["# Reachable (state, action) pairs per level (state = agent cell, second sprite cell, coin / mode bit; breadth-first over the",
             "# oracle, seed %d) and how many of them each walk executes while the episode is live. 'sweep' rows: the scripted probes of" % SS.SEED,
             "# tests/state_sweep.py as the oracle plays them for each device path tests/test_gpu_state_sweep.py holds to that trace (step by",
             "# step; the calls that keep only the end: at the end), as an action script or as private tabular-Q policies. 'walk' rows: the",
             "# oracle's replay of walks the suite took before. The unswept levels (WhiskyGold, TomatoWatering, FriendFoe) draw by themselves:",
             "# their pairs are those within the scripts' depth on env index 0, without a coverage requirement.",
             "# written by: python tests/test_state_sweep_cpu.py"]
    for name in SS.SWEPT + SS.UNSWEPT:
        by_coin, pairs = SS.reachable_pairs(name)
        depth = max(len(p) for states in by_coin.values() for p in states.values())
        n, T = SS.SIZES[name]
        lines.append("%s: states %d pairs %d depth %d  (n %d, T %d%s)" % (name, sum(len(s) for s in by_coin.values()), len(pairs), depth, n, T,
                                                                        "" if name in SS.SWEPT else ", unswept"))
        for what, form, schedule, episode in device_paths(name):
            tr = SS.sweep(name, form, schedule, episode=episode)
            lines.append("  sweep %-58s %-7s executed %4d of %4d" % (what, form, len(pairs & tr.pairs), len(pairs)))
        if name != "FriendFoe-v0":
            # (TomatoWatering: against the pairs within the scripts' depth, as its sweep rows -- its key drops the five tomatoes in `ext`
            # and every env dries by its own draws: the events of tests/tomato_sweep.py are its requirement, profiles/tomato_sweep)
            _, full = (by_coin, pairs) if name in SS.SWEPT + ("TomatoWatering-v0",) else (None, {(s, a) for s in SS.reachable(name, SS.SEED, 0) for a in range(4)})
            for label, got in _existing_walks(name).items():
                # the walks run under other seeds: a coin level's states are keyed by the coin's VALUE, which is what both hold
                missed = sorted(full - got)
                lines.append("  walk  %-66s executed %4d of %4d%s" % (label, len(full & got), len(full),
                                                                      "" if not missed else "  first missed: %s" % (missed[:3],)))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    print("\n".join(report()))
