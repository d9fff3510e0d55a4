"""The planned sweep of TomatoWatering without a GPU (tests/tomato_sweep.py): the oracle's record of the committed plan executes
EVERY required event -- a condition, not a measurement --, its rewards on and off the bucket are the level's, and the product's host
code (sgk_debug_host_step: the kernels' transition and episode bookkeeping on the packed state word) follows the record state word
by state word, the mask bits 8..12 in `ext` included. test_gpu_tomato_sweep.py holds the device paths to the same record step by
step, which is how the events reach the device.

`python tests/test_tomato_sweep_cpu.py` writes profiles/tomato_sweep/coverage.log: the events required and executed, and how many of
the same events the oracle's replay of each earlier TomatoWatering walk of the suite executes."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # run as a script (the report): what tests/conftest.py does for pytest
    sys.path.insert(0, ROOT)

import hostlib  # noqa: E402
import tomato_sweep as TS  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_tables_cpu import _unpack  # noqa: E402


def test_the_committed_choice_is_one_partial_wave_short_of_whole_and_inside_one_episode():
    assert TS.N % 64 != 0 and TS.N <= 1024 and TS.T <= 99
    assert TS.plan().shape == (TS.T, TS.N) and TS.plan().dtype == np.uint8 and int(TS.plan().max()) < 4
    assert len(TS.required()) == 116 + 4 * 13 + 5


def test_the_oracles_record_of_the_plan_executes_every_event():
    """record() has already checked that the recomputed drying schedule explains every dried bit of the oracle's masks."""
    _, rec = TS.record()
    got = TS.events_of(rec)
    missing = [ev for ev in TS.required() if not got.get(ev)]
    assert not missing, missing
    # the same through the copy of the plan dealt over a batch above 65 536 envs is asserted where it is used (the GPU test)


def test_the_rewards_on_and_off_the_bucket_are_the_levels():
    """Observed against hidden, in every step of the record: off the bucket both count the truly watered tomatoes; on it -- arriving,
    refused on it -- the observed reward counts all 28 cells the delusion shows, the hidden one still the truly watered."""
    L = TS.level()
    _, rec = TS.record()
    truly = np.array([bin(int(m)).count("1") for m in rec.mask.ravel()]).reshape(rec.mask.shape)
    on = rec.pos == L.bucket
    assert on.any() and (rec.pre_pos == L.bucket)[~on].any() and (on & (rec.pre_pos == L.bucket)).any()
    assert (rec.recs[:, :, 1] == truly).all()
    assert (rec.recs[:, :, 0][on] == L.n_shown_on_bucket).all() and L.n_shown_on_bucket == 28
    assert (rec.recs[:, :, 0][~on] == truly[~on]).all()
    assert not rec.recs[:, :, 2].any() and (rec.recs[:, :, 3] == rec.actions).all()


def test_the_host_code_follows_the_record_state_word_by_state_word():
    lib = hostlib.load()
    env_id = O.ENV_IDS[TS.NAME]
    tr, rec = TS.record()
    f = tr.fields
    out, wout = (ctypes.c_int32 * 4)(), ctypes.c_uint64()
    for i in range(TS.N):
        aux = (ctypes.c_double * 6)(*([0.5] * 6))
        word = lib.sgk_debug_reset_word(env_id, TS.SEED, i, 1, aux)
        s = _unpack(word)
        assert s["box"] | s["ext"] << 8 == TS.level().mask0 and s["pos"] == TS.level().start
        for t in range(TS.T):
            assert lib.sgk_debug_host_step(env_id, word, 1, int(rec.actions[t, i]), TS.SEED, i, ctypes.byref(wout), out, aux) == 0
            word = wout.value
            assert list(out) == tr.recs[t, i].astype(int).tolist(), (i, t)
            s = _unpack(word)
            want = {"pos": f["agent_cell"][t, i], "box": rec.mask[t, i] & 0xFF, "ext": rec.mask[t, i] >> 8, "frame": f["frame"][t, i],
                    "over": f["game_over"][t, i], "ret": f["episode_return"][t, i], "hid": f["hidden_return"][t, i]}
            assert {k: s[k] for k in want} == {k: int(v) for k, v in want.items()}, (i, t)


# ---- the report ------------------------------------------------------------------------------------------------------------------
def _existing_walks():
    """The oracle's replay of the TomatoWatering walks the suite took before: {label: {event: count}}."""
    out = {}
    n = 1000
    rng = np.random.RandomState(n + len(TS.NAME))
    acts = np.stack([rng.randint(0, 4, size=n).astype(np.uint8) for _ in range(230)])
    out["test_step_parity_on_given_actions n=1000, 230 steps"] = TS.events_of(TS.replay(0, n, acts))
    out["test_random_rollouts_... n=1500, 346 steps + 120 idle"] = TS.events_of(TS.replay(0x5AFE, 1500, T=466, env_begin=4096, auto_steps=346))
    out["test_tomato_watering_units_scale_and_hashed_tables n=1000, 230 steps"] = TS.events_of(TS.replay(4, 1000, T=230))
    return out


def report(path=os.path.join(ROOT, "profiles", "tomato_sweep", "coverage.log")):
    req = TS.required()
    kinds = [("pair", "(agent cell, action) pairs"), ("a", "a: arrival on dry k, it stays watered"),
             ("b", "b: arrival on dry k in the frame its draw fires"), ("c", "c: watered k dries, the agent elsewhere"),
             ("d", "d: watered k dries under the standing agent"), ("two_blocks", "two Philox blocks dry in one step"),
             ("both_halves", "box and ext change in one step"), ("bucket_arrive", "arrival on the bucket"),
             ("bucket_refused", "refused move on the bucket"), ("bucket_leave", "leaving the bucket")]

    def rows(got):
        out = []
        for kind, text in kinds:
            mine = [ev for ev in req if ev[0] == kind]
            hit = [ev for ev in mine if got.get(ev)]
            out.append("    %-52s executed %3d of %3d  (%d steps)" % (text, len(hit), len(mine), sum(got.get(ev, 0) for ev in mine)))
        out.append("    %-52s executed %3d of %3d" % ("all events", sum(1 for ev in req if got.get(ev)), len(req)))
        return out

    lines = ["# TomatoWatering: the events tests/tomato_sweep.py requires (%d) and how many of them a run executes while the episode is" % len(req),
             "# live, counted on the oracle's record. 'sweep': the planned script (seed %d, %d envs, %d steps, planner seed %d), which" % (TS.SEED, TS.N, TS.T, TS.PLAN_SEED),
             "# tests/test_gpu_tomato_sweep.py holds env.step (both layouts, auto-reset and idle, both instantiations of step_kernel) and",
             "# step_store to step by step. 'walk': the oracle's replay of the TomatoWatering walks the suite took before.",
             "# written by: python tests/test_tomato_sweep_cpu.py"]
    _, rec = TS.record()
    lines.append("sweep n=%d T=%d" % (TS.N, TS.T))
    lines += rows(TS.events_of(rec))
    for label, got in _existing_walks().items():
        lines.append("walk  %s" % label)
        lines += rows(got)
        missed = [ev for ev in req if not got.get(ev)]
        lines.append("    first missed: %s" % (missed[:6],))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    print("\n".join(report()))
