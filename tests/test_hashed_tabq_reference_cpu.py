"""tests/hashed_tabq_reference.py without a GPU: with a capacity nobody reaches it IS the oracle's dictionary agent, bit for bit,
and the inputs test_gpu_hashed_tabq.py runs at capacity 64 put agents into every class the device's full-table rule has to be
right for -- conditions on the inputs, checked on the reference alone."""
import numpy as np

import hashed_tabq_reference as HR
from oracle import oracle as O

ROOMY = 1 << 20


def _bits(row):
    return [float(x).hex() for x in row]


def test_without_a_reachable_capacity_it_is_the_oracles_agent_bit_for_bit():
    envs, agents, acts = HR.run(ROOMY)
    orc = O.EnvBatch(HR.NAME, HR.N, seed=HR.SEED)
    ref = [O.TabQ(orc.H * orc.W, HR.ARGS["lr"], HR.ARGS["discount"], HR.ARGS["epsilon"], HR.ARGS["epsilon_anneal"]) for _ in range(HR.N)]
    want = O.tabq_rollout(orc, ref, HR.T, seed=HR.SEED, record_actions=True)
    assert acts.tobytes() == want.tobytes()
    for i, (a, r) in enumerate(zip(agents, ref)):
        assert a.n_rows == r.n_rows and not a.overflowed and a.refused == 0, i
        for key, row in a.rows.items():
            assert _bits(row) == _bits(r.lookup(np.frombuffer(key, dtype=np.int8))), i
    assert envs.boards().tobytes() == orc.boards().tobytes()


def test_the_inputs_fill_tables_exactly_and_past_the_brim_at_capacity_64():
    _, agents, _ = HR.run(64)
    below, full, over = HR.classes(agents)
    print("capacity 64, T = %d: %d below, %d exactly full, %d overflowed" % (HR.T, len(below), len(full), len(over)))
    assert len(below) >= 8 and len(over) >= 8 and len(full) >= 3
    assert all(agents[i].n_rows == 64 and agents[i].refused > 0 for i in over)
    assert all(agents[i].refused == 0 for i in below + full)
    assert HR.hash_info(agents) == (64, 64, True)
    # an overflowed agent holds exactly the first 64 boards the unbounded agent admitted, and went on learning on those
    _, roomy, _ = HR.run(ROOMY)
    changed = 0
    for i in over:
        assert list(agents[i].rows) == list(roomy[i].rows)[:64]
        changed += any(_bits(agents[i].rows[k]) != _bits(roomy[i].rows[k]) for k in agents[i].rows)
    # (a board without a row reads what a fresh row holds, zeros, so the rows that survive differ from the unbounded agent's only
    # where a board that got no row would have learnt something and was met again: a few agents, and at least one is needed)
    print("overflowed agents whose surviving rows differ from the unbounded agent's: %d of %d" % (changed, len(over)))
    assert changed >= 1
    for i in below + full:
        assert list(agents[i].rows) == list(roomy[i].rows)
        assert all(_bits(agents[i].rows[k]) == _bits(roomy[i].rows[k]) for k in agents[i].rows)


def test_the_boundary_case_tells_the_two_orders_of_claiming_the_start_board_apart():
    """Agents created one env step into the episode have not looked its start board up when it ends (agent step 99). Claimed in the
    step that ends the episode (the fused device calls) or at the next step's act (the reference trainer, the per-step calls): the
    same actions and the same ORDER of admission, so 31 steps on the tables are the same -- and on the boundary they are not."""
    for cap in (ROOMY, 64):
        _, late, acts_late = HR.run(cap, 99, pre_steps=1)
        _, early, acts_early = HR.run(cap, 99, claim_start_on_reset=True, pre_steps=1)
        assert acts_late.tobytes() == acts_early.tobytes()
        more = [i for i, (a, b) in enumerate(zip(late, early)) if b.n_rows == a.n_rows + 1]
        refused = [i for i, (a, b) in enumerate(zip(late, early)) if a.n_rows == cap and not a.overflowed and b.overflowed]
        print("capacity %d on the boundary: %d agents hold the start board early only, %d full agents are refused early only"
              % (cap, len(more), len(refused)))
        for i, (a, b) in enumerate(zip(late, early)):
            assert list(b.rows)[:a.n_rows] == list(a.rows) and b.n_rows - a.n_rows in (0, 1), i
            assert all(_bits(a.rows[k]) == _bits(b.rows[k]) for k in a.rows), i
        assert len(more) >= 8 and (cap == ROOMY or len(refused) >= 3)
        _, late, acts_late = HR.run(cap, 130, pre_steps=1)
        _, early, acts_early = HR.run(cap, 130, claim_start_on_reset=True, pre_steps=1)
        assert acts_late.tobytes() == acts_early.tobytes()
        for a, b in zip(late, early):
            assert list(a.rows) == list(b.rows) and a.overflowed == b.overflowed
            assert all(_bits(a.rows[k]) == _bits(b.rows[k]) for k in a.rows)
    for claim in (False, True):
        _, agents, _ = HR.run(64, 99, claim_start_on_reset=claim, pre_steps=1)
        below, full, over = HR.classes(agents)
        print("capacity 64, pre-step, T = 99, claim %s: %d below, %d exactly full, %d overflowed" % (claim, len(below), len(full), len(over)))
        assert len(below) >= 8 and len(over) >= 8 and len(full) >= 3


def test_the_evaluation_case_reaches_the_limit_too():
    _, trained, agents = HR.run_then_evaluate(64, 80)
    b0, f0, o0 = HR.classes(trained)
    below, full, over = HR.classes(agents)
    print("capacity 64, 80 learning steps then evaluate(1): %d / %d / %d -> %d / %d / %d" % (len(b0), len(f0), len(o0), len(below), len(full), len(over)))
    assert len(b0) >= 300 and max(a.n_rows for a in trained) == 64  # a training state that leaves agents near the limit
    assert len(below) >= 8 and len(full) >= 3 and len(over) - len(o0) >= 8  # ... which the evaluation's own lookups reach
    for a, b in zip(trained, agents):  # an evaluation admits boards and learns nothing
        assert list(b.rows)[:a.n_rows] == list(a.rows)
        assert all(_bits(a.rows[k]) == _bits(b.rows[k]) for k in a.rows)
        assert all(not any(b.rows[k]) for k in list(b.rows)[a.n_rows:])


def test_capacity_128_is_the_regime_a_user_runs():
    _, agents, _ = HR.run(128)
    cap, used, overflowed = HR.hash_info(agents)
    print("capacity 128, T = %d: the fullest agent holds %d boards" % (HR.T, used))
    assert not overflowed and used > 0.6 * cap
