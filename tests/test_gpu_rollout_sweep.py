"""The rollouts that choose their own actions, swept: sgk_rollout_random, sgk_rollout_random_stream, sgk_policy_rollout(_members),
sgk_convq_rollout(_members) and sgk_convq_rollout_trans each execute EVERY reachable (agent cell, second sprite cell, coin / mode
bit, action) of the seven deterministic levels at the FIRST step of a launch, from planted states, and are held to the oracle's record
(tests/rollout_sweep.py) as bytes: every step's record, action and the board it was chosen on where the call hands them out, the
boards, every field of episode_state_host() / last_episode_host() and the metrics behind the launch.

No action is forced. What a launch draws at its first step is known before it (the random stream at the lockstep step; the
epsilon-greedy draw at epsilon 1; the categorical draw on a zero actor head), so the plan deals each reachable state to envs that are
going to draw the action it still needs and brings them there through env.step and env.reset(mask), which test_gpu_state_sweep.py
holds to the oracle on every pair. Every case asserts the planted batch against the record BEFORE it launches. The coverage is
asserted on the record (test_rollout_sweep_cpu.py, and again here), the device equals the record, so the coverage reaches what each
kernel has of its own: how it loads the state word at launch, its board painter (the ring and tile writers of the streamed rollout,
the observation the MLP rollout builds from registers, the LDS int8 rows of the conv rollout, the second row set of the two-board
one), `frame` and the returns carried into a launch that starts mid-episode, and the final write-back. The K-step continuation ends
episodes, resets them and steps on inside the launch; the time-limit leg launches at frame 97 of 100.

The greedy leg (epsilon 0, integer weights under which float32 is exact) has no pair requirement: every reachable state is SEEN by the
network through each rollout's own painter at step 0, and float64 chooses on the ORACLE's board, so a painter that draws a state
wrongly shows as another action."""
import numpy as np
import pytest

import rollout_sweep as RS
import safe_grid_agents_amd as S
import state_sweep as SS
from oracle import oracle as O
from safe_grid_agents_amd import _lib
from test_gpu_forward_float64 import cnn_dict, member_dict, mlp_dict
from test_gpu_grid_passes import capped
from test_gpu_state_sweep import _assert_state, _same_bytes, _torch
from test_rollout_sweep_cpu import GREEDY_WIDTH, greedy_sweep

pytestmark = pytest.mark.gpu

SEED, DRAW0 = RS.SEED, RS.DRAW0
LEVELS = pytest.mark.parametrize("name", SS.SWEPT)
LAYOUTS = pytest.mark.parametrize("layout", ["pitched", "compact"])
# (auto_reset, mask_finished) of the network rollouts
MODES = pytest.mark.parametrize("auto_reset,mask", [(True, False), (False, False), (False, True)], ids=["auto", "idle", "idle-masked"])
FORMS = pytest.mark.parametrize("form", ["eps1", "sample"])
RING, FIRST = 3, 2  # trajectory rings of 3 slices, fewer than any K, written from slice 2 on: every launch wraps


def _covered(name, tr):
    """The condition the sweep exists for, on the record the device is about to be held to: step 0 of the launch executes every pair."""
    by_coin, pairs = SS.reachable_pairs(name)
    assert pairs <= tr.pairs_at[0], (name, sorted(pairs - tr.pairs_at[0])[:5])
    assert tr.n % 64 != 0
    return tr


def _fields(tr, t):
    return {k: v[t] for k, v in tr.fields.items()}


def _planted(name, plan, tr, layout="compact", env=None):
    """A handle in the plan's states: the scripts through env.step (no auto-reset unless the plan says so), the masked resets in front
    of their steps; then the batch against the record -- boards, every field, the lockstep counter, the metrics."""
    torch = _torch()
    own = env is None
    if own:
        env = S.BatchedGridworldEnv(name, plan.n, seed=plan.seed, env_index_base=plan.env_begin, layout=layout)
    try:
        assert env.info.max_iterations == RS.MAX_ITERATIONS
        for t in range(plan.L + 1):
            if plan.masks[t].any():
                env.reset(torch.as_tensor(plan.masks[t], device="cuda"))
            if t < plan.L:
                env.step(torch.as_tensor(plan.scripts[t], device="cuda"), auto_reset=getattr(plan, "auto", False))
        where = "%s planted" % name
        _assert_state(env, tr.boards_planted, tr.fields_planted, where)
        assert env.lockstep_t == plan.L, where
        assert env.metrics().tolist() == tr.metrics_planted.tolist(), where
        if name == "FriendFoe-v0":
            assert (env.bandit_policy().reshape(plan.n, 6).view(np.uint64) == tr.aux_planted).all(), where
    except BaseException:
        if own:
            env.close()
        raise
    return env


def _assert_behind(env, tr, k, where, records=True):
    """The handle behind step k of the launch: the last records (where the call leaves them in the env's buffer), boards, every field,
    the metrics."""
    t = tr.L + k
    if records:
        _same_bytes(env.step_records_host(), tr.recs[t], where + " records")
    _assert_state(env, tr.boards[t], _fields(tr, t), where)
    assert env.metrics().tolist() == tr.metrics_at[k].tolist(), where + " metrics"
    assert env.lockstep_t == t + 1, where
    if tr.name == "FriendFoe-v0":
        assert (env.bandit_policy().reshape(tr.n, 6).view(np.uint64) == tr.aux_at[k]).all(), where + " estimates"


# ---- 1. sgk_rollout_random: outputs once -------------------------------------------------------------------------------------------
@LEVELS
@LAYOUTS
def test_rollout_random_executes_every_pair_at_its_first_step(name, layout):
    """One launch of ONE step from the planted batch: records, boards, every field, the last-episode arrays and the metrics right
    behind the probed step."""
    plan, tr = RS.planned(name, "random"), _covered(name, RS.sweep(name, "random", True, K=1))
    env = _planted(name, plan, tr, layout)
    try:
        env.step_random(1, auto_reset=True, fused=True)
        _assert_behind(env, tr, 0, "%s %s rollout_random K=1" % (name, layout))
    finally:
        env.close()


@LEVELS
@LAYOUTS
@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto", "idle"])
def test_rollout_random_continues_from_the_planted_states(name, layout, auto_reset):
    """K steps in one launch on a twin handle: the episodes that end inside it are reset there and step on (or idle)."""
    plan, tr = RS.planned(name, "random"), _covered(name, RS.sweep(name, "random", auto_reset))
    env = _planted(name, plan, tr, layout)
    try:
        env.step_random(tr.K, auto_reset=auto_reset, fused=True)
        _assert_behind(env, tr, tr.K - 1, "%s %s rollout_random K=%d" % (name, layout, tr.K))
    finally:
        env.close()


# ---- 2. sgk_rollout_random_stream ----------------------------------------------------------------------------------------------------
def _stream(env, tr, dest, where, auto_reset=True, launches=None):
    """The streamed rollout over the K steps of the record in launches of (2, K - 2) steps: into the env's own buffers (the last step
    of each launch is what they keep) or into rings of RING slices from slice FIRST on, compared slice by slice behind each launch
    -- every step of the continuation before the wrap overwrites it."""
    torch = _torch()
    n, K = tr.n, tr.K
    launches = (2, K - 2) if launches is None else launches
    assert sum(launches) == K and max(launches) <= RING
    if dest != "own":
        n_tiles = (n + 63) // 64
        shape = (lambda x: (n_tiles, RING, 64, x)) if dest == "tile" else (lambda x: (RING, n, x))
        boards = torch.full(shape(env.n_cells), -7, dtype=torch.int8, device="cuda")
        recs = torch.full(shape(4), -7, dtype=torch.int8, device="cuda")
    k = 0
    for steps in launches:
        if dest == "own":
            env.step_random(steps, auto_reset=auto_reset, fused="stream")
        else:
            env.rollout_random_stream(steps, boards=boards, recs=recs, first_slice=(FIRST + k) % RING, auto_reset=auto_reset, layout=dest)
            got_b = (env.ring_slices(boards) if dest == "tile" else boards).cpu().numpy()
            got_r = (env.ring_slices(recs) if dest == "tile" else recs).cpu().numpy()
            for j in range(steps):
                sl = (FIRST + k + j) % RING
                _same_bytes(got_b[sl], tr.boards[tr.L + k + j], "%s step %d slice %d boards" % (where, k + j, sl))
                _same_bytes(got_r[sl], tr.recs[tr.L + k + j], "%s step %d slice %d records" % (where, k + j, sl))
        k += steps
        _assert_behind(env, tr, k - 1, "%s behind step %d" % (where, k - 1))


@LEVELS
@pytest.mark.parametrize("dest", ["slice", "tile", "own"])
def test_streamed_rollout_executes_every_pair_at_its_first_step(name, dest):
    plan, tr = RS.planned(name, "random"), _covered(name, RS.sweep(name, "random", True))
    env = _planted(name, plan, tr)
    try:
        _stream(env, tr, dest, "%s stream %s" % (name, dest))
    finally:
        env.close()


@LEVELS
def test_streamed_rollout_keeps_the_probed_step_alone(name):
    """One launch of one step into the env's own buffers and a pitched handle: the streamed kernel's own start-up and write-back with
    nothing between them."""
    plan, tr = RS.planned(name, "random"), _covered(name, RS.sweep(name, "random", True, K=1))
    env = _planted(name, plan, tr, "pitched")
    try:
        env.step_random(1, auto_reset=True, fused="stream")
        _assert_behind(env, tr, 0, "%s stream K=1" % name)
    finally:
        env.close()


@pytest.mark.parametrize("dest", ["slice", "tile"])
def test_streamed_rollout_takes_the_planted_states_through_a_second_pass(dest, monkeypatch):
    """BoatRace at 17 189 envs on a handle whose launches are capped at 64 workgroups (256 waves): the tiles from 256 on are a wave's
    SECOND tile, whose state word comes from memory behind the first tile's write-back. The plan deals the pairs over the whole batch,
    so both passes hold every pair; asserted on the record for the envs of the later pass."""
    import grid_passes as GP

    name, n = "BoatRace-v0", GP.N_STREAM
    plan = RS.planned(name, "random", n=n)
    tr = _covered(name, RS.sweep(name, "random", True, n=n))
    later = GP.later_pass(n)
    keys = list(zip(tr.fields_planted["agent_cell"].tolist(), tr.fields_planted["box_cell"].tolist(), tr.fields_planted["coin"].tolist()))
    assert later.any() and SS.reachable_pairs(name)[1] <= {(keys[i], int(tr.actions[tr.L, i])) for i in np.nonzero(later)[0]}
    with capped(monkeypatch, name, n, seed=SEED) as env:
        _planted(name, plan, tr, env=env)
        _stream(env, tr, dest, "%s capped stream %s" % (name, dest))


# ---- 3. / 4. sgk_policy_rollout and its members ------------------------------------------------------------------------------------
def _buffers(torch, K, n, cells):
    return {"states": torch.full((K, n, cells), 77, dtype=torch.int8, device="cuda"),
            "actions": torch.full((K, n), 9, dtype=torch.uint8, device="cuda"),
            "recs": torch.full((K, n, 4), 5, dtype=torch.int8, device="cuda")}


def _assert_trajectory(buf, tr, mask, where, lo=0):
    """states_out (the oracle's board each action was chosen on), actions_out and recs_out of steps lo .. of the launch; with
    mask_finished the states and actions of an env whose episode was over are zeros."""
    K = buf["actions"].shape[0]
    over = tr.over[lo:lo + K] & bool(mask)
    _same_bytes(buf["actions"].cpu().numpy(), RS.masked(tr.actions[tr.L + lo:tr.L + lo + K], over), where + " actions")
    _same_bytes(buf["states"].cpu().numpy(), RS.masked(tr.chosen_on[lo:lo + K], over), where + " states")
    _same_bytes(buf["recs"].cpu().numpy(), tr.recs[tr.L + lo:tr.L + lo + K], where + " records")


def _real(torch, shape, seed):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.3).numpy()


def _mlp_weights(cells, hidden, form, seed):
    """torch-layout float32 weights; "sample": a zero actor head (the logits are exactly 0 and the categorical draw on them is exact);
    "eps1": arbitrary ones (every env explores: the action is the draw's, whatever the scores)."""
    torch = _torch()
    w = [_real(torch, s, seed + i) for i, s in enumerate(((hidden, cells), (hidden,), (hidden, hidden), (hidden,), (4, hidden), (4,)))]
    if form == "sample":
        w[4][:], w[5][:] = 0.0, 0.0
    return w


def _cnn_weights(cells, C, form, seed, in_channels=1):
    torch = _torch()
    shapes = ((C, in_channels, 3, 3), (C,), (C, C, 3, 3), (C,), (C, in_channels, 1, 1), (C,), (C, C, 3, 3), (C,), (4, C * cells), (4,))
    w = [_real(torch, s, seed + i) for i, s in enumerate(shapes)]
    if form == "sample":
        w[8][:], w[9][:] = 0.0, 0.0
    return w


def _launch_kw(form, auto_reset, mask):
    return dict(mode="greedy" if form == "eps1" else "sample", epsilon=1.0 if form == "eps1" else 0.0, draw_index0=DRAW0, auto_reset=auto_reset,
                mask_finished=mask)


@LEVELS
@FORMS
@MODES
@pytest.mark.parametrize("hidden", [64, 100])
def test_policy_rollout_executes_every_pair_at_its_first_step(name, form, auto_reset, mask, hidden):
    torch = _torch()
    plan, tr = RS.planned(name, form), _covered(name, RS.sweep(name, form, auto_reset))
    env = _planted(name, plan, tr)
    try:
        buf = _buffers(torch, tr.K, tr.n, env.n_cells)
        env.policy_rollout(mlp_dict(_mlp_weights(env.n_cells, hidden, form, 11)), tr.K, **_launch_kw(form, auto_reset, mask), **buf)
        where = "%s policy_rollout %s h%d" % (name, form, hidden)
        _assert_trajectory(buf, tr, mask, where)
        _assert_behind(env, tr, tr.K - 1, where, records=False)
    finally:
        env.close()


def _assert_member_metrics(mm, before, after, where):
    """What the members booked in this launch adds up to what the handle booked in it: the sums, and the maxima the handle ends with."""
    mm = mm.cpu().numpy()
    sums = [O.M_SUM_RETURN, O.M_SUM_SAFETY, O.M_SUM_MARGIN, O.M_SUM_MARGIN_POS, O.M_EPISODES, O.M_MARGIN_POS_COUNT]
    maxs = [O.M_MAX_RETURN, O.M_MAX_SAFETY, O.M_MAX_MARGIN, O.M_MAX_MARGIN_POS]
    assert mm[:, sums].sum(axis=0).tolist() == (after[sums] - before[sums]).tolist(), where
    assert np.maximum(before[maxs], mm[:, maxs].max(axis=0)).tolist() == after[maxs].tolist(), where


def _fresh_member_metrics(torch, M):
    m = np.stack([O.metrics_new() for _ in range(M)])
    return torch.as_tensor(m, device="cuda")


@LEVELS
@FORMS
@pytest.mark.parametrize("auto_reset,mask", [(True, False), (False, True)], ids=["auto", "idle-masked"])
def test_policy_rollout_members_executes_every_pair_at_its_first_step(name, form, auto_reset, mask):
    """M members of n / M envs each with weights of their own; "eps1" through the per-member epsilon array, all ones, with the
    launch's own epsilon 0 (a member that read the scalar would act greedily). Every member holds a mixture of states, coins and drawn
    actions (test_rollout_sweep_cpu.py); the per-member metrics add up to the handle's."""
    torch = _torch()
    M = RS.MEMBERS[name]
    plan, tr = RS.planned(name, form), _covered(name, RS.sweep(name, form, auto_reset))
    env = _planted(name, plan, tr)
    try:
        buf = _buffers(torch, tr.K, tr.n, env.n_cells)
        w = member_dict([_mlp_weights(env.n_cells, 100, form, 100 * m + 13) for m in range(M)])
        mm = _fresh_member_metrics(torch, M)
        kw = _launch_kw(form, auto_reset, mask)
        if form == "eps1":
            kw.update(epsilon=0.0, member_epsilon=torch.ones(M, dtype=torch.float64, device="cuda"))
        before = env.metrics()
        env.policy_rollout_members(w, M, tr.K, member_metrics=mm, **kw, **buf)
        where = "%s policy_rollout_members %s" % (name, form)
        _assert_trajectory(buf, tr, mask, where)
        _assert_behind(env, tr, tr.K - 1, where, records=False)
        _assert_member_metrics(mm, before, env.metrics(), where)
    finally:
        env.close()


# ---- 5. sgk_convq_rollout and its members ----------------------------------------------------------------------------------------------
_CONV = {}


def _conv_accepts(name):
    """Whether the fused conv body takes this level's board, by the binding's own refusal (sgk_convq_act_members_all names the boards
    it does not cover before it launches anything)."""
    if name not in _CONV:
        torch = _torch()
        env = S.BatchedGridworldEnv(name, 4, seed=SEED)
        try:
            w = {k: v.unsqueeze(0).contiguous() for k, v in cnn_dict(_cnn_weights(env.n_cells, 4, "sample", 1)).items()}
            try:
                env.convq_act_members_all(w, 1, 4)
                _CONV[name] = True
            except _lib.SgkError as exc:
                assert "does not cover" in str(exc), exc
                _CONV[name] = False
        finally:
            env.close()
    return _CONV[name]


def test_the_conv_body_takes_every_swept_level():
    """The list the conv cases run over is the binding's; it must not shrink unnoticed: every swept level has a board the body is
    instantiated for (tests/learner_reference.py: CNN_SHAPES)."""
    import learner_reference as R

    for name in SS.SWEPT:
        assert _conv_accepts(name) == (O.shape(name) in R.CNN_SHAPES.values()), name
    assert sum(_conv_accepts(name) for name in SS.SWEPT) == len(SS.SWEPT)


@LEVELS
@FORMS
@MODES
@pytest.mark.parametrize("C", [4, 5, 8])
def test_convq_rollout_executes_every_pair_at_its_first_step(name, form, auto_reset, mask, C):
    torch = _torch()
    if not _conv_accepts(name):
        return
    plan, tr = RS.planned(name, form), _covered(name, RS.sweep(name, form, auto_reset))
    env = _planted(name, plan, tr)
    try:
        buf = _buffers(torch, tr.K, tr.n, env.n_cells)
        env.convq_rollout(cnn_dict(_cnn_weights(env.n_cells, C, form, 17)), tr.K, C, **_launch_kw(form, auto_reset, mask), **buf)
        where = "%s convq_rollout %s C%d" % (name, form, C)
        _assert_trajectory(buf, tr, mask, where)
        _assert_behind(env, tr, tr.K - 1, where, records=False)
    finally:
        env.close()


@LEVELS
@FORMS
@pytest.mark.parametrize("C", [4, 5, 8])
def test_convq_rollout_members_executes_every_pair_at_its_first_step(name, form, C):
    torch = _torch()
    if not _conv_accepts(name):
        return
    M = RS.MEMBERS[name]
    plan, tr = RS.planned(name, form), _covered(name, RS.sweep(name, form, True))
    env = _planted(name, plan, tr)
    try:
        buf = _buffers(torch, tr.K, tr.n, env.n_cells)
        one = [cnn_dict(_cnn_weights(env.n_cells, C, form, 100 * m + 19)) for m in range(M)]
        w = {k: torch.stack([d[k] for d in one]).contiguous() for k in one[0]}
        mm = _fresh_member_metrics(torch, M)
        before = env.metrics()
        env.convq_rollout_members(w, M, tr.K, C, member_metrics=mm, **_launch_kw(form, True, False), **buf)
        where = "%s convq_rollout_members %s C%d" % (name, form, C)
        _assert_trajectory(buf, tr, False, where)
        _assert_behind(env, tr, tr.K - 1, where, records=False)
        _assert_member_metrics(mm, before, env.metrics(), where)
    finally:
        env.close()


# ---- 6. sgk_convq_rollout_trans -----------------------------------------------------------------------------------------------------------
TRANS_LEVEL = "BoatRace-v0"


def _trans_launches(env, tr, w, C, kw, mask, where, launches):
    """The two-board rollout over the record's K steps in `launches`, the caller's prev_boards planted from the record and handed from
    launch to launch: prev_states (channel 0 of every observation), states, actions, records, and what prev_boards holds behind."""
    torch = _torch()
    prev = torch.as_tensor(tr.prev_planted.copy(), device="cuda")
    k = 0
    for steps in launches:
        buf = _buffers(torch, steps, tr.n, env.n_cells)
        prev_states = torch.full((steps, tr.n, env.n_cells), 77, dtype=torch.int8, device="cuda")
        env.convq_rollout(w, steps, C, prev_boards=prev, prev_states=prev_states, fresh=False, **dict(kw, draw_index0=DRAW0 + k), **buf)
        _assert_trajectory(buf, tr, mask, "%s steps %d.." % (where, k), lo=k)
        over = tr.over[k:k + steps] & bool(mask)
        _same_bytes(prev_states.cpu().numpy(), RS.masked(tr.prev_on[k:k + steps], over), "%s steps %d.. prev_states" % (where, k))
        k += steps
    assert k == tr.K
    _same_bytes(prev.cpu().numpy(), tr.prev_after, where + " prev_boards behind")
    _assert_behind(env, tr, tr.K - 1, where, records=False)


@FORMS
@MODES
@pytest.mark.parametrize("C", [4, 5, 8])
@pytest.mark.parametrize("launches", ["one", "two"])
def test_convq_rollout_trans_executes_every_pair_at_its_first_step(form, auto_reset, mask, C, launches):
    """The observation of step 0 is [the oracle's previous board, board]: the board before the last path step, and [board, board]
    for the state reached by reset alone. With auto-reset the record holds observations behind a reset ([board, board] again)."""
    name = TRANS_LEVEL
    plan, tr = RS.planned(name, form), _covered(name, RS.sweep(name, form, auto_reset, two_board=True))
    assert (tr.prev_planted != tr.boards_planted).any() and (tr.prev_planted == tr.boards_planted).all(axis=1).any()
    if auto_reset:
        assert tr.fresh[1:].any()
    env = _planted(name, plan, tr)
    try:
        w = cnn_dict(_cnn_weights(env.n_cells, C, form, 23, in_channels=2))
        _trans_launches(env, tr, w, C, _launch_kw(form, auto_reset, mask), mask, "%s convq_rollout_trans %s C%d" % (name, form, C),
                        (tr.K,) if launches == "one" else (1, tr.K - 1))
    finally:
        env.close()


# ---- 7. the greedy leg ---------------------------------------------------------------------------------------------------------------
def _greedy_case(name, body, auto_reset):
    by_coin, _ = SS.reachable_pairs(name)
    w, tr = greedy_sweep(name, body, auto_reset)
    assert tr.keys_at[0] == {s for states in by_coin.values() for s in states}  # the network sees every reachable state at step 0
    return w, tr, RS.planned(name, "eps1")


@LEVELS
@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto", "idle"])
def test_policy_rollout_greedy_takes_the_float64_action_in_every_reachable_state(name, auto_reset):
    torch = _torch()
    w, tr, plan = _greedy_case(name, "mlp", auto_reset)
    env = _planted(name, plan, tr)
    try:
        buf = _buffers(torch, tr.K, tr.n, env.n_cells)
        env.policy_rollout(mlp_dict(w), tr.K, mode="greedy", epsilon=0.0, draw_index0=DRAW0, auto_reset=auto_reset, **buf)
        _assert_trajectory(buf, tr, False, "%s policy_rollout greedy" % name)
        _assert_behind(env, tr, tr.K - 1, "%s policy_rollout greedy" % name, records=False)
    finally:
        env.close()


@LEVELS
@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto", "idle"])
def test_convq_rollout_greedy_takes_the_float64_action_in_every_reachable_state(name, auto_reset):
    torch = _torch()
    if not _conv_accepts(name):
        return
    w, tr, plan = _greedy_case(name, "cnn", auto_reset)
    env = _planted(name, plan, tr)
    try:
        buf = _buffers(torch, tr.K, tr.n, env.n_cells)
        env.convq_rollout(cnn_dict(w), tr.K, GREEDY_WIDTH["cnn"], mode="greedy", epsilon=0.0, draw_index0=DRAW0, auto_reset=auto_reset, **buf)
        _assert_trajectory(buf, tr, False, "%s convq_rollout greedy" % name)
        _assert_behind(env, tr, tr.K - 1, "%s convq_rollout greedy" % name, records=False)
    finally:
        env.close()


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto", "idle"])
def test_convq_rollout_trans_greedy_takes_the_float64_action_in_every_reachable_state(auto_reset):
    name = TRANS_LEVEL
    w, tr, plan = _greedy_case(name, "trans", auto_reset)
    env = _planted(name, plan, tr)
    try:
        kw = dict(mode="greedy", epsilon=0.0, draw_index0=DRAW0, auto_reset=auto_reset, mask_finished=False)
        _trans_launches(env, tr, cnn_dict(w), GREEDY_WIDTH["trans"], kw, False, "%s convq_rollout_trans greedy" % name, (2, tr.K - 2))
    finally:
        env.close()


# ---- 8. the time-limit leg -------------------------------------------------------------------------------------------------------------
LIMIT = pytest.mark.parametrize("name", RS.LIMIT_LEVELS)


def _limit_case(name, chooser):
    """Every env at frame 97 of its first episode by a scripted walk that ends none: the limit ends the episodes at step 2 of the
    launch, from a `frame` that came in through the state word (asserted on the record by test_rollout_sweep_cpu.py and here)."""
    plan, tr = RS.limit_plan(name), RS.limit_sweep(name, chooser, True)
    assert (tr.fields_planted["frame"] == RS.MAX_ITERATIONS - RS.LIMIT_BEFORE).all() and not tr.recs[:tr.L, :, 2].any()
    assert tr.recs[tr.L + RS.LIMIT_BEFORE - 1, :, 2].any() and min(RS.events(tr)) > 0
    return plan, tr


@LIMIT
@pytest.mark.parametrize("path", ["fused", "own", "slice", "tile"])
def test_the_time_limit_ends_episodes_inside_a_random_rollout(name, path):
    plan, tr = _limit_case(name, "random")
    env = _planted(name, plan, tr)
    try:
        if path == "fused":
            env.step_random(tr.K, auto_reset=True, fused=True)
            _assert_behind(env, tr, tr.K - 1, "%s limit rollout_random" % name)
        else:
            _stream(env, tr, path, "%s limit stream %s" % (name, path), launches=(3, 3))
    finally:
        env.close()


@LIMIT
@FORMS
@pytest.mark.parametrize("body", ["mlp", "cnn"])
def test_the_time_limit_ends_episodes_inside_a_network_rollout(name, form, body):
    torch = _torch()
    plan, tr = _limit_case(name, form)
    env = _planted(name, plan, tr)
    try:
        buf = _buffers(torch, tr.K, tr.n, env.n_cells)
        if body == "mlp":
            env.policy_rollout(mlp_dict(_mlp_weights(env.n_cells, 100, form, 29)), tr.K, **_launch_kw(form, True, False), **buf)
        else:
            env.convq_rollout(cnn_dict(_cnn_weights(env.n_cells, 5, form, 31)), tr.K, 5, **_launch_kw(form, True, False), **buf)
        where = "%s limit %s %s" % (name, body, form)
        _assert_trajectory(buf, tr, False, where)
        _assert_behind(env, tr, tr.K - 1, where, records=False)
    finally:
        env.close()


# ---- 9. the levels that draw by themselves ---------------------------------------------------------------------------------------------
DRAWN = pytest.mark.parametrize("name", SS.UNSWEPT)


def _drawn_case(name, chooser):
    """The level's committed plan (tests/whisky_sweep.py, tomato_sweep.py, foe_sweep.py) played to a mid-plan step at which, on the
    oracle, an env is drunk / has a dry and a watered tomato / has estimates that moved; no coverage requirement here (theirs stay in
    their own sweeps). The env's own draws are keyed by (reset count, frame): the record needs no planning around them."""
    plan, cond = RS.drawn_level(name)
    tr = RS.drawn_sweep(name, chooser)
    check = O.EnvBatch(name, plan.n, seed=plan.seed)
    for t in range(plan.L):
        check.rollout(1, seed=plan.seed, t_begin=t, auto_reset=True, actions=plan.scripts[t][None])
    assert (check.export()[0] == tr.boards_planted).all() and (cond(check) & (tr.fields_planted["game_over"] == 0)).any()
    return plan, tr


@DRAWN
@pytest.mark.parametrize("path", ["fused", "own", "slice", "tile"])
def test_random_rollouts_from_the_middle_of_a_drawn_levels_plan(name, path):
    """rollout_random in launches of one step, the streamed rollout in launches of two: held behind every launch, FriendFoe's
    estimates as uint64 included; the rings slice by slice."""
    plan, tr = _drawn_case(name, "random")
    env = _planted(name, plan, tr)
    try:
        if path == "fused":
            for k in range(tr.K):
                env.step_random(1, auto_reset=True, fused=True)
                _assert_behind(env, tr, k, "%s rollout_random step %d" % (name, k))
        else:
            _stream(env, tr, path, "%s stream %s" % (name, path))
    finally:
        env.close()


@DRAWN
@FORMS
def test_policy_rollout_from_the_middle_of_a_drawn_levels_plan(name, form):
    """Two launches of two steps: every step's board, action and record; the estimates behind each launch."""
    torch = _torch()
    plan, tr = _drawn_case(name, form)
    env = _planted(name, plan, tr)
    try:
        w = mlp_dict(_mlp_weights(env.n_cells, 100, form, 37))
        for k in range(0, tr.K, 2):
            buf = _buffers(torch, 2, tr.n, env.n_cells)
            env.policy_rollout(w, 2, **dict(_launch_kw(form, True, False), draw_index0=DRAW0 + k), **buf)
            where = "%s policy_rollout %s steps %d.." % (name, form, k)
            _assert_trajectory(buf, tr, False, where, lo=k)
            _assert_behind(env, tr, k + 1, where, records=False)
    finally:
        env.close()
