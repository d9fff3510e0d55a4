"""Ensemble acting for the PPO-CNN population -- sgk_convq_act_members_all (the member instantiation of convq_act_kernel), the body-agnostic
sgk_members_vote, EnsembleMixin on BatchedPPOCNNPopulation -- on the GPU. Every comparison is exact: integers as they are, floats through
their bytes (the float64 bound of section 3 is tests/test_gpu_forward_float64.py's).

1. the cross product is M single calls: member m's actions and scores == env.convq_act(member m's slices, epsilon 0), on 2 ENVS + 5 envs
   (two full passes and a partial one) of three board shapes x channel counts, with and without the scores;
2. a member's second grid-stride pass, and nothing written at index >= N of a row;
3. the scores against the float64 conv forward (tests/forward_reference.py): equal with small-integer weights, within 8 x torch-float32's
   own error with real ones;
4. members [A, A, B, B]: equal rows, and two copies of A vote A's own greedy actions;
5. ensemble_act == the numpy vote (tests/ensemble_reference.py) over the M single-call rows, with votes_out, subsets, out= and one voter;
6. five load_member copies of one agent: evaluate_ensemble == batched_default_eval of that agent on a twin env, dissent 0;
7. evaluate_ensemble of three distinct members == the loop done by hand on a twin handle, eagerly and from a recorded graph, also after a
   learn() changed the weights in place; the population is untouched;
8. guard bands: neither output leaves its buffer (tests/guard_arena.py; tests/test_convq_ensemble_abi.py points here).

N and the population constructor: BatchedPPOCNNPopulation needs n_envs % n_members == 0, and 2 ENVS + 5 is a multiple of five for no board
shape (ENVS is 17, 14, 12, 9, 9, 8 or 7), so where a population is involved N is 2 ENVS + 5 rounded UP to a multiple of M: still two full
passes and a partial one, never fewer envs. The raw call (sections 1 - 3, 8) has no such constraint and runs at 2 ENVS + 5 exactly.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import hashlib
import types

import numpy as np
import pytest

import ensemble_reference as ER
import forward_reference as FR
import guard_arena as GA
import learner_reference as R
import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib
from safe_grid_agents_amd import ppo_cnn_population as PC
from safe_grid_agents_amd.loops import batched_default_eval

pytestmark = pytest.mark.gpu

BOAT, SOKOBAN, SHIFT = "BoatRace-v0", "SideEffectsSokoban-v0", "DistributionalShift-v0"
# (level, channels): ENVS = 17 with the scalar fifth channel; ENVS = 12 on one MFMA row tile; ENVS = 7 with two MFMA row tiles
SHAPES = [(BOAT, 5), (SOKOBAN, 4), (SHIFT, 8)]
WEIGHT_NAMES = ("w1", "b1", "w2", "b2", "wb", "bb", "wh", "bh", "wl", "bl")
ACTION_SENTINEL, TAIL = 77, 64


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _envs_per_pass(level):
    return FR.conv_envs_per_pass(*R.CNN_SHAPES[level])


def _n_small(level, members=1):
    """2 ENVS + 5, rounded up to a multiple of `members` (see the module docstring)."""
    n = 2 * _envs_per_pass(level) + 5
    return -(-n // members) * members


def _args(C, rollouts, seed=5):
    return types.SimpleNamespace(discount=0.99, batch_size=7, rollouts=rollouts, epochs=2, n_layers=2, n_hidden=None, n_channels=C, device=0,
                                 log_gradients=False, cheat=False, seed=seed, lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01)


def _random_weights(torch, rng, members, cells, C, dev):
    """The ten acting tensors stacked [M, ...], seeded (scale: outputs that are neither flat nor saturated)."""
    shapes = {"w1": (C, 1, 3, 3), "b1": (C,), "w2": (C, C, 3, 3), "b2": (C,), "wb": (C, 1, 1, 1), "bb": (C,), "wh": (C, C, 3, 3), "bh": (C,),
              "wl": (4, C * cells), "bl": (4,)}
    return {k: torch.as_tensor(rng.normal(0.0, 0.05 if k == "wl" else 0.3, (members,) + s).astype(np.float32)).to(dev)
            for k, s in shapes.items()}


def _stack(torch, per_member, dev):
    """[[ten float32 arrays] per member] (forward_reference.cnn_weights) -> the stacked dict."""
    return {k: torch.as_tensor(np.stack([w[i] for w in per_member])).contiguous().to(dev) for i, k in enumerate(WEIGHT_NAMES)}


def _single(weights, m):
    return {k: v[m] for k, v in weights.items()}


def _episodes(env):
    return env._device_views()["n_episodes"].cpu().numpy()


def _handle_state(env, episodes_before=0):
    """Everything an evaluation leaves in the handle: boards, last step records, the decoded state words, the episode arrays, the metrics.
    n_episodes counts over the handle's life (no reset clears it): what it gained since episodes_before (_episodes(env) then)."""
    v = env._device_views()
    out = {"boards": env.boards_host(), "records": env.step_records_host(), "metrics": env.metrics()}
    out.update({"word " + k: a for k, a in env.episode_state_host().items()})
    out.update({k: v[k].cpu().numpy() for k in ("last_return", "last_performance")})
    out["n_episodes"] = _episodes(env) - episodes_before
    return out


def _same_bytes(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def _population_hash(pop):
    """One digest over everything the ensemble must leave alone: weights, Adam's moments, step and draw counters, the old policy, the
    per-member hyper-parameters and the members' metrics."""
    h = hashlib.sha256()
    tensors = dict(pop.tensors())
    tensors.update({"old_" + k: t for k, t in pop.old.items()})
    tensors["member_metrics"], tensors["member_keys"] = pop.member_metrics, pop.member_keys
    if pop.hyper is not None:
        tensors.update({"hyper_" + k: t for k, t in pop.hyper.items()})
    for k in sorted(tensors):
        h.update(k.encode())
        h.update(tensors[k].cpu().numpy().tobytes())
    h.update(repr(pop.draws).encode())
    return h.hexdigest()


# ---- 1. the cross product is M single calls -------------------------------------------------------------------------------------------
def _check_cross_product(torch, env, weights, members, C):
    """member_actions[m] / member_scores[m] of ONE sgk_convq_act_members_all call against sgk_convq_act(epsilon 0) with member m's slices.
    Both outputs are over-allocated FLAT buffers whose [M, N] / [M, N, 4] views are their heads: every entry of the views was written
    (sentinels), row m + 1 starts right behind row m's entry N - 1 (a store at index >= N of a row would change the next row's first
    bytes, which are compared with the single call's), and the tail behind the last row keeps its sentinel."""
    n, dev = env.n_envs, "cuda:%d" % env.device
    flat_a = torch.full((members * n + TAIL,), ACTION_SENTINEL, dtype=torch.uint8, device=dev)
    flat_s = torch.full((members * n * 4 + 4 * TAIL,), float("nan"), dtype=torch.float32, device=dev)
    actions, scores = flat_a[:members * n].view(members, n), flat_s[:members * n * 4].view(members, n, 4)
    boards, words = env.boards_host(), env.episode_state_host()
    assert env.convq_act_members_all(weights, members, C, out=actions, scores_out=scores) is actions
    alone = torch.full((members, n), ACTION_SENTINEL, dtype=torch.uint8, device=dev)
    assert env.convq_act_members_all(weights, members, C, out=alone, scores_out=None) is alone  # the scores are optional
    fresh = env.convq_act_members_all(weights, members, C)
    got_a, got_s = actions.cpu().numpy(), scores.cpu().numpy()
    assert alone.cpu().numpy().tobytes() == got_a.tobytes() and fresh.cpu().numpy().tobytes() == got_a.tobytes()
    assert fresh.shape == (members, n) and fresh.dtype == torch.uint8
    assert got_a.max() <= 3 and not np.isnan(got_s).any()
    assert (flat_a[members * n:] == ACTION_SENTINEL).all() and torch.isnan(flat_s[members * n * 4:]).all()
    for m in range(members):
        want_s = torch.full((n, 4), float("nan"), dtype=torch.float32, device=dev)
        want_a = env.convq_act(_single(weights, m), 0.0, 0, C, scores_out=want_s).cpu().numpy()
        assert got_a[m].tobytes() == want_a.tobytes(), (m, np.flatnonzero(got_a[m] != want_a)[:8])
        assert got_s[m].tobytes() == want_s.cpu().numpy().tobytes(), (m, np.flatnonzero((got_s[m] != want_s.cpu().numpy()).any(axis=1))[:8])
        assert (got_a[m] == got_s[m].argmax(axis=1)).all()  # greedy: the first maximum
    assert len({got_s[m].tobytes() for m in range(members)}) == members  # the members are different networks
    assert env.boards_host().tobytes() == boards.tobytes()  # the env is read, never written
    _same_bytes(words, env.episode_state_host(), "state words")
    return got_a, got_s


@pytest.mark.parametrize("level,C", SHAPES)
def test_the_cross_product_is_one_convq_act_per_member(level, C):
    """M = 3 members on 2 ENVS + 5 envs, 5 random steps into their episodes so that the boards differ: every member's workgroups take two
    full passes and a partial one of five envs (39 envs in one workgroup per pass on BoatRace, 29 on Sokoban, 19 on DistributionalShift)."""
    torch = _torch()
    n = _n_small(level)
    assert n == 2 * _envs_per_pass(level) + 5
    env = S.BatchedGridworldEnv(level, n, seed=31, env_index_base=1000)
    try:
        env.step_random(5, auto_reset=True)
        assert len({b.tobytes() for b in env.boards_host()}) > 1
        w = _random_weights(torch, np.random.default_rng(100 + C), 3, env.n_cells, C, "cuda:%d" % env.device)
        _check_cross_product(torch, env, w, 3, C)
    finally:
        env.close()


def test_one_member_is_the_single_call():
    """n_members = 1: the member instantiation on the single kernel's grid, member 0's slices being the tensors themselves."""
    torch = _torch()
    env = S.BatchedGridworldEnv(SOKOBAN, _n_small(SOKOBAN), seed=33, layout="pitched")
    try:
        env.step_random(5, auto_reset=True)
        _check_cross_product(torch, env, _random_weights(torch, np.random.default_rng(1), 1, env.n_cells, 5, "cuda:%d" % env.device), 1, 5)
    finally:
        env.close()


# ---- 2. a member's second grid-stride pass --------------------------------------------------------------------------------------------
def test_a_members_second_grid_stride_pass_is_exact_and_stops_at_n():
    """launch_convq_act_members (csrc/sgk_convq.hip) starts member_wgs = min(passes, max(per_cu n_cus / M, 1)) workgroups per member, each
    taking the passes blockIdx.x, blockIdx.x + member_wgs, ... of ENVS = 17 BoatRace envs. per_cu is the single launcher's: min(3 waves
    per SIMD with five channels, 160 KB / 34 912 bytes of LDS) = 3. With M = 3 and N = 17 (member_wgs + 2) + 3 there are member_wgs + 3
    passes, so a member's workgroups 0 .. 2 run a second pass (its boards requested during the first) and the last pass holds 3 envs:
    4 389 envs on 256 compute units. Every row equals the single call; the next row's first bytes and the sentinel tail show that
    nothing was written at index >= N of a row (_check_cross_product)."""
    torch = _torch()
    cus = torch.cuda.get_device_properties(0).multi_processor_count  # what the library's n_cus is (csrc/sgk_api.hip)
    envs, members, per_cu = _envs_per_pass(BOAT), 3, 3
    assert envs == 17
    member_wgs = max(per_cu * cus // members, 1)
    n = envs * (member_wgs + 2) + 3
    assert -(-n // envs) == member_wgs + 3 and n % envs == 3 and n <= 40000
    env = S.BatchedGridworldEnv(BOAT, n, seed=32)
    try:
        env.step_random(5, auto_reset=True)
        w = _random_weights(torch, np.random.default_rng(7), members, env.n_cells, 5, "cuda:%d" % env.device)
        _check_cross_product(torch, env, w, members, 5)
    finally:
        env.close()


# ---- 3. against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,C", SHAPES)
def test_member_scores_against_float64(level, C):
    """Three members with weights of their own (forward_reference.cnn_weights, one seed per member) on the env's own boards. "integer":
    every partial sum is an integer below 2^24 (asserted), so float32 is exact in any order and the scores must EQUAL the float64
    forward's. "real": err_k = max|got - s64| / max|s64| <= learner_reference.bound(err_t) = 8 x torch-float32's own figure (at least 16
    ulp), the bound tests/test_gpu_forward_float64.py holds sgk_convq_act to. The greedy action is the float64 argmax wherever the top-2
    gap is above 4 bound max|s64| (everywhere with integer weights, exact ties included: the first maximum)."""
    torch = _torch()
    shape, n, M = R.CNN_SHAPES[level], _n_small(level), 3
    env = S.BatchedGridworldEnv(level, n, seed=35)
    try:
        env.step_random(5, auto_reset=True)
        boards = env.boards_host().reshape(n, -1)
        dev = "cuda:%d" % env.device
        for family in ("integer", "real"):
            per_member = [FR.cnn_weights(family, shape, C, 7100 + 10 * C + m) for m in range(M)]
            scores = torch.full((M, n, 4), float("nan"), dtype=torch.float32, device=dev)
            actions = env.convq_act_members_all(_stack(torch, per_member, dev), M, C, scores_out=scores).cpu().numpy()
            got = scores.cpu().numpy()
            for m, w in enumerate(per_member):
                s64 = FR.forward("cnn", boards, w, shape)
                if family == "integer":
                    assert boards.min() >= 0 and FR.abs_sum_bound("cnn", boards, w, shape) < FR.EXACT_LIMIT
                    wrong = np.flatnonzero((got[m] != s64).any(axis=1))
                    assert np.array_equal(got[m], s64), (m, len(wrong), wrong[:8])
                    assert np.array_equal(actions[m], s64.argmax(1)), m
                else:
                    err_t = R.rel_err(FR.forward("cnn", boards, w, shape, dtype=torch.float32), s64)
                    err_k, limit = R.rel_err(got[m], s64), R.bound(err_t)
                    print("%s C=%d member %d: err_k %.3e err_t %.3e limit %.3e" % (level, C, m, err_k, err_t, limit))
                    assert err_k <= limit, (m, err_k, err_t, limit)
                    clear = FR.top2_gap(s64) > 4.0 * limit * float(np.abs(s64).max())
                    assert (actions[m][clear] == s64.argmax(1)[clear]).all(), m
    finally:
        env.close()


# ---- 4. / 5. the population's vote ----------------------------------------------------------------------------------------------------
def _two_by_two(env, C, seed):
    """A population of M = 4 whose members are [A, A, B, B]: two distinct random-init weight sets."""
    pop = S.BatchedPPOCNNPopulation(env, _args(C, env.n_envs // 4, seed=seed), 4)
    pop.load_member(1, PC.unstack_state_dict(pop.cur, 0))
    pop.load_member(3, PC.unstack_state_dict(pop.cur, 2))
    return pop


@pytest.mark.parametrize("level,C", [(BOAT, 5), (SOKOBAN, 4)])
def test_copies_vote_as_one(level, C):
    """Members [A, A, B, B]: rows 0 == 1 and 2 == 3 of the cross product; with members=[0, 1] the vote is A's own greedy action on every
    env (2-0), and so is one voter's; with all four every env is a 4-0 or a 2-2 vote and a tie goes to the lower action."""
    torch = _torch()
    n = _n_small(level, 4)
    env = S.BatchedGridworldEnv(level, n, seed=41)
    try:
        dev = "cuda:%d" % env.device
        pop = _two_by_two(env, C, seed=5)
        env.step_random(5, auto_reset=True)
        w = pop._ensemble_weights()
        votes = torch.full((n, 4), 777, dtype=torch.uint16, device=dev)
        actions = pop.ensemble_act(votes_out=votes).cpu().numpy()
        ma = pop._ens["member_actions"].cpu().numpy()
        assert ma.shape == (4, n) and ma[0].tobytes() == ma[1].tobytes() and ma[2].tobytes() == ma[3].tobytes()
        own_a = env.convq_act(_single(w, 0), 0.0, 0, C).cpu().numpy()
        own_b = env.convq_act(_single(w, 2), 0.0, 0, C).cpu().numpy()
        assert ma[0].tobytes() == own_a.tobytes() and ma[2].tobytes() == own_b.tobytes()
        assert pop.ensemble_act(members=[0, 1]).cpu().numpy().tobytes() == own_a.tobytes()
        assert pop.ensemble_act(members=[3]).cpu().numpy().tobytes() == own_b.tobytes()
        want = ER.vote(ma)
        assert actions.tobytes() == want[0].tobytes() and votes.cpu().numpy().tobytes() == want[1].tobytes()
        disagree = ma[0] != ma[2]
        print("%s: A and B disagree on %d of %d envs" % (level, int(disagree.sum()), n))
        assert (actions[disagree] == np.minimum(ma[0], ma[2])[disagree]).all() and (actions[~disagree] == ma[0][~disagree]).all()
    finally:
        env.close()


@pytest.mark.parametrize("level,C", [(BOAT, 5), (SHIFT, 8)])
def test_ensemble_act_is_the_numpy_vote_over_the_single_calls(level, C):
    """M = 3 random-init members: ensemble_act's actions and votes_out == tests/ensemble_reference.py's vote over the three rows that
    env.convq_act(member m, epsilon 0) returns -- all members, the subsets [2, 0] and [1, 2] (a tensor), one voter (its own actions);
    `out` is returned as given; the population is what it was."""
    torch = _torch()
    M = 3
    n = _n_small(level, M)
    env = S.BatchedGridworldEnv(level, n, seed=43, env_index_base=300)
    try:
        dev = "cuda:%d" % env.device
        pop = S.BatchedPPOCNNPopulation(env, _args(C, n // M, seed=11), M)
        before = _population_hash(pop)
        env.step_random(5, auto_reset=True)
        w = pop._ensemble_weights()
        assert all(w[k].data_ptr() == pop._acting_weights(pop.cur)[k].data_ptr() for k in WEIGHT_NAMES)  # evaluate()'s tensors, in place
        rows = np.stack([env.convq_act(_single(w, m), 0.0, 0, C).cpu().numpy() for m in range(M)])
        for members in (None, [2, 0], torch.tensor([1, 2], device=dev), [1]):
            listed = None if members is None else [int(v) for v in members]
            votes = torch.full((n, 4), 777, dtype=torch.uint16, device=dev)
            out = torch.full((n,), 9, dtype=torch.uint8, device=dev)
            assert pop.ensemble_act(members=members, out=out, votes_out=votes) is out
            want = ER.vote(rows, members=listed)
            assert out.cpu().numpy().tobytes() == want[0].tobytes(), listed
            assert votes.cpu().numpy().tobytes() == want[1].tobytes(), listed
            assert pop._ens["member_actions"].cpu().numpy().tobytes() == rows.tobytes()  # the acting launch covers every member
        assert pop.ensemble_act(members=[1]).cpu().numpy().tobytes() == rows[1].tobytes()
        assert _population_hash(pop) == before
        for members, message in (([], "selects nobody"), ([1, 1], "twice"), ([0, 3], "members 0 .. 2")):
            with pytest.raises(ValueError, match=message):
                pop.ensemble_act(members=members)
    finally:
        env.close()


# ---- 6. identical members are one agent -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,C", [(BOAT, 5), (SOKOBAN, 4)])
def test_identical_members_are_one_agent(level, C):
    """M = 5 load_member copies of one BatchedPPOAgent(body="cnn"): evaluate_ensemble(T = 7) -- T - 1 steps of {act-all, vote, step,
    reset_done}, then max_iterations steps without the reset -- leaves what batched_default_eval of the single agent (its greedy weights
    through sgk_convq_rollout) leaves on a twin env with the same seed and env_index_base, and nobody ever dissents. N = 40 on BoatRace,
    30 on Sokoban (2 ENVS + 5 rounded up to a multiple of five: the module docstring)."""
    torch = _torch()
    T, M = 7, 5
    n = _n_small(level, M)
    assert n % M == 0 and 2 * _envs_per_pass(level) + 5 <= n < 3 * _envs_per_pass(level)
    e1, e2 = (S.BatchedGridworldEnv(level, n, seed=51, env_index_base=700) for _ in range(2))
    try:
        torch.manual_seed(9)
        agent = S.BatchedPPOAgent(e1, _args(C, n), body="cnn")
        assert agent.fused_conv and agent.greedy_weights() is not None  # (the single agent's evaluation is the fused rollout)
        pop = S.BatchedPPOCNNPopulation(e2, _args(C, n // M), M)
        for m in range(M):
            pop.load_member(m, agent.net.state_dict())
        before = _population_hash(pop)
        want = batched_default_eval(agent, e1, T)
        got, dissent = pop.evaluate_ensemble(T)
        assert got.vec == want.vec
        assert want.vec[_lib.M_EPISODES] >= n
        _same_bytes(_handle_state(e1), _handle_state(e2), level)
        horizon = int(e1.info.max_iterations)
        assert dissent["dissent"] == 0 and dissent["disagreement"] == 0.0 and 0 < dissent["votes"] <= M * n * (T - 1 + horizon)
        assert _population_hash(pop) == before
    finally:
        e1.close(); e2.close()


# ---- 7. the evaluation is the loop done by hand ---------------------------------------------------------------------------------------
def _by_hand(torch, env, weights, M, C, T, members=None):
    """evaluate_ensemble's schedule from the existing calls: env.convq_act(epsilon 0) per member, the vote on the host, env.step /
    reset_done."""
    dissent = np.zeros(2, dtype=np.int64)
    singles = [_single(weights, m) for m in range(M)]
    env.metrics_reset()
    env.reset()

    def step(reset_done):
        live = ~env.episode_state_host()["over"].astype(bool)
        ma = np.stack([env.convq_act(w, 0.0, 0, C).cpu().numpy() for w in singles])
        actions, _, d = ER.vote(ma, members=members, live=live)
        dissent[:] += d
        env.step(torch.as_tensor(actions).to("cuda:%d" % env.device), auto_reset=False)
        if reset_done:
            env.reset_done()

    for _ in range(T - 1):
        step(True)
    for _ in range(int(env.info.max_iterations)):
        step(False)
    return env.metrics(), dissent


@pytest.mark.parametrize("level,C", [(BOAT, 5), (SOKOBAN, 8)])
def test_the_evaluation_is_the_loop_done_by_hand(level, C):
    """M = 3 distinct members, T = 7: metrics, the handle (episode state included) and the dissent / votes counters against the
    hand-written loop on a twin env; graph=True (one recorded lockstep step per phase, replayed) gives the same bytes, twice; a subset
    [2, 0] likewise. Then set_member_hyper and a learn() change the weights IN PLACE: the hand-written loop with the new weights is what
    the eager call and a replay of the graphs recorded BEFORE the change (the same recordings: the tensors' addresses stayed) give. The
    ensemble leaves cur, old, Adam's moments, the step and draw counters, the hyper-parameters and the member metrics as bytes."""
    torch = _torch()
    T, M = 7, 3
    n = _n_small(level, M)
    e1, e2 = (S.BatchedGridworldEnv(level, n, seed=61, env_index_base=64) for _ in range(2))
    try:
        pop = S.BatchedPPOCNNPopulation(e2, _args(C, n // M), M, member_hyper={"lr": [1e-3, 2e-3, 4e-3]})

        def compare(members, graphs):
            episodes = _episodes(e1)
            want_metrics, want_dissent = _by_hand(torch, e1, pop._ensemble_weights(), M, C, T, members)
            want_state = _handle_state(e1, episodes)
            assert (want_state["n_episodes"] >= 1).all() and want_dissent[1] > 0
            for graph in graphs:
                episodes = _episodes(e2)
                bm, dissent = pop.evaluate_ensemble(T, members=members, graph=graph)
                assert bm.vec == want_metrics.tolist(), (members, graph)
                assert [dissent["dissent"], dissent["votes"]] == want_dissent.tolist(), (members, graph)
                assert dissent["disagreement"] == want_dissent[0] / want_dissent[1]
                _same_bytes(want_state, _handle_state(e2, episodes), (level, members, graph))
            return want_dissent

        before = _population_hash(pop)
        d = compare(None, (False, True, True))
        print("%s: disagreement %d / %d" % (level, d[0], d[1]))
        recorded = dict(pop._ens["graphs"])
        assert len(recorded) == 1 and len(next(iter(recorded.values()))) == 2
        assert _population_hash(pop) == before
        # the weights change in place: a learn() under new per-member learning rates
        pop.set_member_hyper("lr", [1e-2, 2e-2, 4e-2])
        old_bytes = {k: t.cpu().numpy().tobytes() for k, t in pop.cur.items()}
        pop.learn(pop.gather_rollout())
        torch.cuda.synchronize()
        assert all(pop.cur[k].cpu().numpy().tobytes() != old_bytes[k] for k in ("w1", "w2", "wa", "la"))
        before = _population_hash(pop)
        compare(None, (True, False))
        now = pop._ens["graphs"]
        assert list(now) == list(recorded) and all(a is b for a, b in zip(next(iter(now.values())), next(iter(recorded.values()))))
        compare([2, 0], (False, True, True))
        assert _population_hash(pop) == before
    finally:
        e1.close(); e2.close()


# ---- 8. guard bands -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", GA.PATTERNS)
@pytest.mark.parametrize("level,C", [(BOAT, 5), (SHIFT, 8)])
def test_the_outputs_stay_inside_their_guard_bands(level, C, pattern):
    """member_actions and member_scores (the two pointers of sgk_members_act_out) carved from a guard_arena.Arena: 256-byte aligned, a
    guard of max(4096 bytes, one member row) on each side, under both patterns. The ten stacked weight tensors are frozen inputs. After
    the call with both outputs and the call with the actions alone: no guard byte and no input byte changed, no output entry still
    holds the pattern, the env's boards and state words are what they were, and the bytes equal a twin call on ordinary tensors."""
    torch = _torch()
    M = 3
    n = _n_small(level)
    env = S.BatchedGridworldEnv(level, n, seed=81)
    try:
        env.step_random(7, auto_reset=True)
        dev = "cuda:%d" % env.device
        plain = _random_weights(torch, np.random.default_rng(5 + C), M, env.n_cells, C, dev)
        arena = GA.Arena(dev, pattern, 1 << 20)
        w = {}
        for k in WEIGHT_NAMES:
            w[k] = arena.adopt("w_" + k, plain[k])
            arena.freeze("w_" + k)
        member_actions = arena.carve("member_actions", (M, n), torch.uint8)
        member_scores = arena.carve("member_scores", (M, n, 4), torch.float32)
        member_actions_only = arena.carve("member_actions_only", (M, n), torch.uint8)
        assert arena.layout_ok() and arena.check() == []
        for name, row in (("member_actions", n), ("member_scores", 16 * n), ("member_actions_only", n)):
            start, _, guard, outer = arena.span(name)
            assert outer == row and guard >= max(GA.MIN_GUARD, row) and start % GA.ALIGN == 0
        boards, words = env.boards_host(), env.episode_state_host()
        env.convq_act_members_all(w, M, C, out=member_actions, scores_out=member_scores)
        env.convq_act_members_all(w, M, C, out=member_actions_only)
        torch.cuda.synchronize()
        assert arena.check() == []
        for name in ("member_actions", "member_scores", "member_actions_only"):
            assert arena.unwritten(name) == 0, name
        twin_s = torch.empty((M, n, 4), dtype=torch.float32, device=dev)
        twin_a = env.convq_act_members_all(plain, M, C, scores_out=twin_s)
        assert member_actions.cpu().numpy().tobytes() == twin_a.cpu().numpy().tobytes()
        assert member_actions_only.cpu().numpy().tobytes() == twin_a.cpu().numpy().tobytes()
        assert member_scores.cpu().numpy().tobytes() == twin_s.cpu().numpy().tobytes()
        assert env.boards_host().tobytes() == boards.tobytes()
        _same_bytes(words, env.episode_state_host(), "state words")
    finally:
        env.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_what_cannot_run_is_refused_with_the_reason():
    torch = _torch()
    env = S.BatchedGridworldEnv(BOAT, 34, seed=1)
    try:
        dev = "cuda:%d" % env.device
        w = _random_weights(torch, np.random.default_rng(0), 2, env.n_cells, 5, dev)
        ma = torch.zeros((2, 34), dtype=torch.uint8, device=dev)
        for call, message in (
            (lambda: env.convq_act_members_all(w, 3, 5), "shape"), (lambda: env.convq_act_members_all(w, 0, 5), "n_members"),
            (lambda: env.convq_act_members_all(w, 2, 4), "shape"),
            (lambda: env.convq_act_members_all(w, 2, 5, out=torch.zeros((2, 33), dtype=torch.uint8, device=dev)), "out has shape"),
            (lambda: env.convq_act_members_all(w, 2, 5, out=ma.cpu()), "lives on"),
            (lambda: env.convq_act_members_all(w, 2, 5, out=ma, scores_out=torch.zeros((2, 34, 4), dtype=torch.float64, device=dev)), "dtype"),
        ):
            with pytest.raises(ValueError, match=message):
                call()
        six = _random_weights(torch, np.random.default_rng(0), 2, env.n_cells, 6, dev)  # a channel count without an instantiation
        with pytest.raises(_lib.SgkError, match="n_channels"):
            env.convq_act_members_all(six, 2, 6)
        with pytest.raises(_lib.SgkError, match="n_layers"):
            env.convq_act_members_all(w, 2, 5, n_layers=3)
        assert (ma == 0).all()
    finally:
        env.close()
