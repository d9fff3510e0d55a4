"""The two-channel conv body on the GPU -- sgk_convq_act_trans, sgk_convq_sample_trans, sgk_convq_rollout_trans (the observation of a
transition env, [previous board, board]; BoatRace's 5 x 5 board, 4 / 5 / 8 channels) -- against tests/transition_reference.py: the
float64 forward and the emulated rollout whose conditions tests/test_transition_cpu.py asserts.

  1. act and sample against float64: N = 40 (passes of 17, 17 and 6 envs; half the envs have stepped, half are fresh), integer weights
     EQUAL, real weights within 8 x torch-float32's own error (learner_reference.bound, the yardstick measured here); prev_boards=None
     is a copy of the boards, byte for byte; a second grid-stride pass.
  2. the greedy rollout with integer weights against the emulation: actions, both state channels, records, the final state words, the
     metrics and the prev_boards left behind.
  3. the sampled rollout against the per-step loop {convq_sample(prev_boards=...), copy boards -> previous, env.step}.
  4. guard bands around every pointer of sgk_convq_transition (GUARD_BAND_TESTS), 5. a recorded rollout, 6. refusals, 7. the
     one-channel paths are what they were."""
import ctypes
import types

import numpy as np
import pytest

import guard_arena as GA
import learner_reference as R
import safe_grid_agents_amd as S
import transition_reference as TR
from safe_grid_agents_amd import _lib

pytestmark = pytest.mark.gpu
NAMES = ("w1", "b1", "w2", "b2", "wb", "bb", "wh", "bh", "wl", "bl")
# sgk_convq_transition's pointer fields -> the tests that carve them from a guard_arena.Arena (tests/test_transition_cpu.py asks for one each)
GUARD_BAND_TESTS = {
    "prev_boards_dev": ("test_the_acting_calls_stay_inside_their_guard_bands", "test_the_rollout_stays_inside_its_guard_bands"),
    "prev_states_out_dev": ("test_the_rollout_stays_inside_its_guard_bands",),
    "states_out_dev": ("test_the_rollout_stays_inside_its_guard_bands",),
    "actions_out_dev": ("test_the_acting_calls_stay_inside_their_guard_bands", "test_the_rollout_stays_inside_its_guard_bands"),
    "recs_out_dev": ("test_the_rollout_stays_inside_its_guard_bands",),
    "scores_out_dev": ("test_the_acting_calls_stay_inside_their_guard_bands",),
}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _dev(torch, arrays, dev="cuda:0"):
    return {k: torch.as_tensor(np.ascontiguousarray(a)).to(dev) for k, a in zip(NAMES, arrays)}


def _env(n, steps=TR.PRE_STEPS):
    env = S.BatchedGridworldEnv(TR.LEVEL, n, seed=TR.ENV_SEED)
    env.step_random(steps, auto_reset=True)
    env.metrics_reset()
    return env


def _handle_state(env):
    v = env._device_views()
    out = {"boards": env.boards_host(), "records": env.step_records_host(), "metrics": env.metrics()}
    out.update({"word " + k: a for k, a in env.episode_state_host().items()})
    out.update({k: v[k].cpu().numpy() for k in ("last_return", "last_performance", "n_episodes")})
    return out


def _same_bytes(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


# ---- 1. act and sample against float64 ------------------------------------------------------------------------------------------------
def _act_case(torch, n, family, C):
    prev, cur = TR.act_inputs(n)
    w = TR.weights(family, C, 7100 + C)
    env = _env(n, TR.PRE_STEPS + 1)
    assert (env.boards_host().reshape(n, -1) == cur).all()
    return env, prev, cur, w, _dev(torch, w), torch.as_tensor(prev).cuda()


@pytest.mark.parametrize("C", TR.CHANNELS)
@pytest.mark.parametrize("family", ["integer", "real"])
def test_act_and_sample_scores_against_float64(family, C):
    torch = _torch()
    env, prev, cur, w, wd, pd = _act_case(torch, TR.N, family, C)
    try:
        s64 = TR.forward(prev, cur, w)
        scores = torch.full((TR.N, 4), 7.0, dtype=torch.float32, device="cuda")
        logits = torch.full((TR.N, 4), 7.0, dtype=torch.float32, device="cuda")
        greedy = env.convq_act(wd, 0.0, 3, C, scores_out=scores, prev_boards=pd).clone()
        drawn = env.convq_sample(wd, 11, C, logits_out=logits, prev_boards=pd).clone()
        got = scores.cpu().numpy().astype(np.float64)
        assert scores.cpu().numpy().tobytes() == logits.cpu().numpy().tobytes()
        if family == "integer":
            assert (got == s64).all(), np.abs(got - s64).max()
            assert (greedy.cpu().numpy() == s64.argmax(1)).all()  # the first maximum
        else:
            err_t = R.rel_err(TR.forward(prev, cur, w, dtype=torch.float32), s64)  # torch-float32's own error: the yardstick
            err_k = R.rel_err(got, s64)
            print("C = %d: err_k %.3g, err_t %.3g, bound %.3g" % (C, err_k, err_t, R.bound(err_t)))
            assert err_k <= R.bound(err_t), (err_k, err_t)
            assert (greedy.cpu().numpy() == got.argmax(1)).all()
        # the draws are the one-channel calls' on the same scores: epsilon-greedy (stream 2), Categorical (stream 3)
        assert (drawn.cpu().numpy() == env.categorical_sample(logits, 11).cpu().numpy()).all()
        for eps, t in ((0.3, 11), (1.0, 0)):
            assert (env.convq_act(wd, eps, t, C, prev_boards=pd).cpu().numpy() == env.epsilon_greedy(scores, eps, t).cpu().numpy()).all()
        # channel 0 is read: fed [current, current] the scores are others
        env.convq_act(wd, 0.0, 3, C, scores_out=logits, prev_boards=torch.as_tensor(cur).cuda())
        assert (logits != scores).any()
    finally:
        env.close()


@pytest.mark.parametrize("C", TR.CHANNELS)
def test_no_previous_boards_means_the_current_ones(C):
    torch = _torch()
    env, prev, cur, w, wd, pd = _act_case(torch, TR.N, "real", C)
    try:
        copy = env.boards().reshape(TR.N, -1).clone().contiguous()
        out = {}
        for key, p in (("none", None), ("copy", copy)):
            s = torch.zeros((TR.N, 4), dtype=torch.float32, device="cuda")
            l = torch.zeros((TR.N, 4), dtype=torch.float32, device="cuda")
            a = env.convq_act(wd, 0.1, 5, C, scores_out=s, prev_boards=p).clone()
            b = env.convq_sample(wd, 6, C, logits_out=l, prev_boards=p).clone()
            out[key] = {"scores": s.cpu().numpy(), "logits": l.cpu().numpy(), "act": a.cpu().numpy(), "sample": b.cpu().numpy()}
        _same_bytes(out["none"], out["copy"], "prev_boards=None")
        assert (out["none"]["scores"].astype(np.float64) != TR.forward(prev, cur, w)).any()  # (and not the stepped envs' scores)
    finally:
        env.close()


def test_a_second_grid_stride_pass_is_exact_and_stops_at_n():
    torch = _torch()
    C = 5
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = TR.second_pass_n(cus)  # more passes than the largest grid the launch code can choose, and a partial last one
    env, prev, cur, w, wd, pd = _act_case(torch, n, "integer", C)
    try:
        tail = 64
        scores = torch.full((n + tail, 4), 7.0, dtype=torch.float32, device="cuda")
        actions = torch.full((n + tail,), 9, dtype=torch.uint8, device="cuda")
        env.convq_act(wd, 0.0, 0, C, out=actions[:n], scores_out=scores[:n], prev_boards=pd)
        s64 = TR.forward(prev, cur, w)
        assert (scores[:n].cpu().numpy().astype(np.float64) == s64).all()
        assert (actions[:n].cpu().numpy() == s64.argmax(1)).all()
        assert (scores[n:] == 7.0).all() and (actions[n:] == 9).all()
    finally:
        env.close()


# ---- 2. the greedy rollout against the emulation ------------------------------------------------------------------------------------
def _buffers(torch, T, n):
    return {"states": torch.full((T, n, TR.CELLS), 77, dtype=torch.int8, device="cuda"),
            "prev_states": torch.full((T, n, TR.CELLS), 77, dtype=torch.int8, device="cuda"),
            "actions": torch.full((T, n), 9, dtype=torch.uint8, device="cuda"),
            "recs": torch.full((T, n, 4), 5, dtype=torch.int8, device="cuda")}


def _check_against(env, bufs, prev_boards, res, steps):
    from oracle import oracle as O

    for k in ("actions", "states", "prev_states", "recs"):
        got = np.concatenate([b[k].cpu().numpy() for b in bufs])
        assert got.shape == res[k].shape
        bad = np.argwhere((got != res[k]).reshape(got.shape[0], got.shape[1], -1).any(2))
        assert not len(bad), (k, "first (step, env):", bad[0].tolist(), "of", len(bad))
    n = env.n_envs
    assert (prev_boards.cpu().numpy() == res["prev_boards"]).all()
    assert (env.boards_host().reshape(n, -1) == res["boards"]).all()
    st, f = env.episode_state_host(), res["fields"]
    for mine, theirs in (("episode_return", "episode_return"), ("hidden_return", "hidden_return"), ("frame", "frame"), ("over", "game_over"),
                         ("agent_cell", "agent_cell")):
        assert (st[mine].astype(np.int64) == f[theirs]).all(), mine
    v = env._device_views()
    assert (v["last_return"].cpu().numpy() == f["last_episode_return"])[f["n_episodes"] > 0].all()
    want = res["metrics"].copy()
    want[O.M_STEPS] = n * steps  # the handle counts the steps it issued
    assert env.metrics().tolist() == want.tolist()


@pytest.mark.parametrize("C", TR.CHANNELS)
@pytest.mark.parametrize("T,auto_reset,mask", [(12, False, False), (103, True, False), (103, False, True)])
def test_the_greedy_rollout_is_the_emulation(T, auto_reset, mask, C):
    torch = _torch()
    res = TR.emulated(C, TR.N, T, auto_reset, mask)
    env = _env(TR.N)
    try:
        wd = _dev(torch, TR.rollout_weights(C))
        b = _buffers(torch, T, TR.N)
        prev = torch.full((TR.N, TR.CELLS), 55, dtype=torch.int8, device="cuda")  # fresh: not read
        env.convq_rollout(wd, T, C, mode="greedy", epsilon=0.0, draw_index0=4, auto_reset=auto_reset, mask_finished=mask, states=b["states"],
                          actions=b["actions"], recs=b["recs"], prev_boards=prev, prev_states=b["prev_states"], fresh=True)
        _check_against(env, [b], prev, res, T)
    finally:
        env.close()


def test_two_launches_with_fresh_on_the_first_are_one():
    torch = _torch()
    C = 5
    res = TR.emulated(C, TR.N, 12, False, False)
    env = _env(TR.N)
    try:
        wd = _dev(torch, TR.rollout_weights(C))
        b1, b2 = _buffers(torch, 7, TR.N), _buffers(torch, 5, TR.N)
        prev = torch.full((TR.N, TR.CELLS), 55, dtype=torch.int8, device="cuda")
        for b, T, fresh in ((b1, 7, True), (b2, 5, False)):
            env.convq_rollout(wd, T, C, mode="greedy", states=b["states"], actions=b["actions"], recs=b["recs"], prev_boards=prev,
                              prev_states=b["prev_states"], fresh=fresh)
        _check_against(env, [b1, b2], prev, res, 12)
    finally:
        env.close()


def test_the_rollouts_second_grid_stride_pass():
    torch = _torch()
    C, T = 5, 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = TR.second_pass_n(cus)
    res = TR.emulate_rollout(TR.rollout_weights(C), n, T, True)
    env = _env(n)
    try:
        wd = _dev(torch, TR.rollout_weights(C))
        b = _buffers(torch, T, n)
        prev = torch.full((n, TR.CELLS), 55, dtype=torch.int8, device="cuda")
        env.convq_rollout(wd, T, C, mode="greedy", auto_reset=True, states=b["states"], actions=b["actions"], recs=b["recs"],
                          prev_boards=prev, prev_states=b["prev_states"], fresh=True)
        _check_against(env, [b], prev, res, T)
    finally:
        env.close()


# ---- 3. the sampled rollout is the per-step loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C", TR.CHANNELS)
def test_the_sampled_rollout_is_the_per_step_loop(C):
    torch = _torch()
    T, n, draw0 = 23, TR.N, 1000
    env_a, env_b = _env(n), _env(n)
    try:
        wd = _dev(torch, TR.weights("real", C, 7300 + C))
        b = _buffers(torch, T, n)
        start = env_a.boards().reshape(n, -1).clone().contiguous()
        prev_a = start.clone()
        prev_a[::3] = 1  # not fresh: some previous boards that are not the current ones
        prev_b = prev_a.clone()
        env_a.convq_rollout(wd, T, C, mode="sample", draw_index0=draw0, auto_reset=False, states=b["states"], actions=b["actions"],
                            recs=b["recs"], prev_boards=prev_a, prev_states=b["prev_states"])
        rec_b = env_b._device_views()["rec"]
        for k in range(T):
            boards = env_b.boards().reshape(n, -1)
            assert (b["states"][k] == boards).all() and (b["prev_states"][k] == prev_b).all(), k
            a = env_b.convq_sample(wd, draw0 + k, C, prev_boards=prev_b).clone()
            assert (b["actions"][k] == a).all(), k
            prev_b.copy_(boards)
            env_b.step(a, auto_reset=False)
            assert (b["recs"][k] == rec_b).all(), k
        assert (prev_a == prev_b).all()
        _same_bytes(_handle_state(env_a), _handle_state(env_b), "sampled rollout")
        assert len(np.unique(b["actions"].cpu().numpy())) >= 2
    finally:
        env_a.close()
        env_b.close()


# ---- 4. guard bands ------------------------------------------------------------------------------------------------------------------
def _arena_weights(torch, arena, C, seed):
    w = {}
    for k, a in zip(NAMES, TR.weights("real", C, seed)):
        w[k] = arena.adopt("w_" + k, torch.as_tensor(a))
        arena.freeze("w_" + k)
    return w


@pytest.mark.parametrize("pattern", GA.PATTERNS)
@pytest.mark.parametrize("C", [5, 8])
def test_the_acting_calls_stay_inside_their_guard_bands(C, pattern):
    """prev_boards (an INPUT of act and sample), the actions and the scores / logits carved from the arena under both patterns: no guard
    byte and no input byte changed, no output entry left holding the pattern, the bytes those of a call on ordinary tensors."""
    torch = _torch()
    n = TR.N
    env = _env(n, TR.PRE_STEPS + 1)
    try:
        arena = GA.Arena("cuda:0", pattern, 1 << 20)
        w = _arena_weights(torch, arena, C, 7400 + C)
        prev = arena.adopt("prev_boards", torch.as_tensor(TR.act_inputs(n)[0]))
        arena.freeze("prev_boards")
        outs = {}
        for call in ("act", "sample"):
            outs[call] = (arena.carve(call + "_actions", (n,), torch.uint8), arena.carve(call + "_scores", (n, 4), torch.float32))
        assert arena.layout_ok() and arena.check() == []
        before = _handle_state(env)
        env.convq_act(w, 0.2, 9, C, out=outs["act"][0], scores_out=outs["act"][1], prev_boards=prev)
        env.convq_sample(w, 9, C, out=outs["sample"][0], logits_out=outs["sample"][1], prev_boards=prev)
        torch.cuda.synchronize()
        assert arena.check() == []
        for name in ("act_actions", "act_scores", "sample_actions", "sample_scores"):
            assert arena.unwritten(name) == 0, name
        plain = {k: v.clone() for k, v in w.items()}
        s = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        a = env.convq_act(plain, 0.2, 9, C, scores_out=s, prev_boards=prev.clone())
        assert a.cpu().numpy().tobytes() == outs["act"][0].cpu().numpy().tobytes()
        assert s.cpu().numpy().tobytes() == outs["act"][1].cpu().numpy().tobytes() == outs["sample"][1].cpu().numpy().tobytes()
        _same_bytes(before, _handle_state(env), "acting leaves the handle alone")
    finally:
        env.close()


@pytest.mark.parametrize("pattern", GA.PATTERNS)
@pytest.mark.parametrize("fresh", [True, False])
def test_the_rollout_stays_inside_its_guard_bands(fresh, pattern):
    """Every pointer of the descriptor the rollout uses -- prev_boards (read unless fresh, written at exit), prev_states, states,
    actions, recs -- carved from the arena; the weights frozen. fresh: prev_boards keeps the pattern until the launch writes it."""
    torch = _torch()
    C, T, n = 5, 9, TR.N
    env, twin = _env(n), _env(n)
    try:
        arena = GA.Arena("cuda:0", pattern, 1 << 20)
        w = _arena_weights(torch, arena, C, 7500)
        prev = arena.carve("prev_boards", (n, TR.CELLS), torch.int8)
        given = twin.boards().reshape(n, -1).clone().contiguous()
        given[::2] = 3
        if not fresh:
            prev.copy_(given)
        b = {"states": arena.carve("states", (T, n, TR.CELLS), torch.int8), "prev_states": arena.carve("prev_states", (T, n, TR.CELLS), torch.int8),
             "actions": arena.carve("actions", (T, n), torch.uint8), "recs": arena.carve("recs", (T, n, 4), torch.int8)}
        assert arena.layout_ok() and arena.check() == []
        kw = dict(mode="sample", draw_index0=77, auto_reset=True, fresh=fresh)
        env.convq_rollout(w, T, C, states=b["states"], actions=b["actions"], recs=b["recs"], prev_boards=prev, prev_states=b["prev_states"], **kw)
        torch.cuda.synchronize()
        assert arena.check() == []
        for name in ("prev_boards", "states", "prev_states", "actions", "recs"):
            assert arena.unwritten(name) == 0, name
        t = _buffers(torch, T, n)
        tprev = given.clone()
        twin.convq_rollout({k: v.clone() for k, v in w.items()}, T, C, states=t["states"], actions=t["actions"], recs=t["recs"],
                           prev_boards=tprev, prev_states=t["prev_states"], **kw)
        for k in b:
            assert b[k].cpu().numpy().tobytes() == t[k].cpu().numpy().tobytes(), k
        assert prev.cpu().numpy().tobytes() == tprev.cpu().numpy().tobytes()
        _same_bytes(_handle_state(env), _handle_state(twin), "rollout")
    finally:
        env.close()
        twin.close()


# ---- 5. a recorded rollout -----------------------------------------------------------------------------------------------------------
def test_a_recorded_rollout_replays_as_the_eager_call():
    torch = _torch()
    C, T, n = 5, 6, TR.N
    env, twin = _env(n), _env(n)
    try:
        wd = _dev(torch, TR.weights("real", C, 7600))
        b, t = _buffers(torch, T, n), _buffers(torch, T, n)
        prev, tprev = (torch.zeros((n, TR.CELLS), dtype=torch.int8, device="cuda") for _ in range(2))

        def launch(e, bufs, p):
            e.convq_rollout(wd, T, C, mode="sample", draw_index0=5, auto_reset=True, states=bufs["states"], actions=bufs["actions"],
                            recs=bufs["recs"], prev_boards=p, prev_states=bufs["prev_states"], fresh=True)

        torch.cuda.synchronize()
        cur, following = torch.cuda.current_stream(), env._mode == "follow"
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            env.bind_torch_stream(torch.cuda.current_stream())  # the capture stream
            launch(env, b, prev)
        env.bind_torch_stream(None if following else cur)
        env.account_steps(-T)  # the recorded (not executed) call bumped the host-side counters
        torch.cuda.synchronize()
        assert (b["actions"] == 9).all()  # the capture ran nothing
        graph.replay()
        env.account_steps(T)
        launch(twin, t, tprev)
        torch.cuda.synchronize()
        for k in b:
            assert b[k].cpu().numpy().tobytes() == t[k].cpu().numpy().tobytes(), k
        assert prev.cpu().numpy().tobytes() == tprev.cpu().numpy().tobytes()
        assert (env.boards() == twin.boards()).all()
    finally:
        env.close()
        twin.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_what_cannot_run_is_refused_and_launches_nothing():
    torch = _torch()
    C, n = 5, TR.N
    env = _env(n)
    other = S.BatchedGridworldEnv("SideEffectsSokoban-v0", n, seed=1)
    try:
        wd = _dev(torch, TR.weights("real", C, 7700))
        one = {k: (v[:, :1].contiguous() if k in ("w1", "wb") else v) for k, v in wd.items()}
        six = _dev(torch, TR.weights("real", 6, 7700))
        prev = env.boards().reshape(n, -1).clone().contiguous()
        actions = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        before, prev_before = _handle_state(env), prev.cpu().numpy().copy()
        sok_w = {k: v for k, v in wd.items()}
        sok_w["wl"] = torch.zeros((4, C * other.n_cells), dtype=torch.float32, device="cuda")
        for call, message in (
            (lambda: env.convq_rollout(wd, 3, C, mode="greedy"), "needs prev_boards"),
            (lambda: env.convq_rollout(one, 3, C, mode="greedy", prev_boards=prev), "one input channel"),
            (lambda: env.convq_rollout(one, 3, C, mode="greedy", fresh=True), "two-channel"),
            (lambda: env.convq_act(one, 0.0, 0, C, out=actions, prev_boards=prev), "one input channel"),
            (lambda: env.convq_sample(six, 0, 6, out=actions, prev_boards=prev), "n_channels"),
            (lambda: env.convq_act(wd, 0.0, 0, C, n_layers=3, out=actions, prev_boards=prev), "n_layers"),
            (lambda: env.convq_act(wd, 0.0, 0, C, out=actions, prev_boards=prev[:, :24].contiguous()), "shape"),
            (lambda: env.convq_act(wd, 0.0, 0, C, out=actions, prev_boards=prev.to(torch.uint8)), "dtype"),
            (lambda: env.convq_rollout(wd, 3, C, mode="both", prev_boards=prev), "mode"),
            (lambda: env.convq_rollout(wd, 3, C, prev_boards=prev, prev_states=torch.zeros((2, n, 25), dtype=torch.int8, device="cuda")), "shape"),
            (lambda: other.convq_act(sok_w, 0.0, 0, C, prev_boards=torch.zeros((n, other.n_cells), dtype=torch.int8, device="cuda")), "5 x 5"),
        ):
            with pytest.raises(ValueError, match=message):
                call()
        # the C entry points themselves: SGK_ERR_INVALID with a message for a NULL descriptor, a NULL prev_boards in the rollout, a
        # board shape without the kernel
        lib = env.lib
        w = env._convq_weights(wd, C, 2, in_channels=2)
        tr = _lib.SgkConvQTransition(None, None, 1, None, ctypes.c_void_p(actions.data_ptr()), None, None)
        env._sync_torch_to_lib()
        for call, message in (
            (lambda: lib.sgk_convq_act_trans(env._h.ptr, ctypes.byref(w), None, 0.0, 0, None, None), b"descriptor"),
            (lambda: lib.sgk_convq_sample_trans(env._h.ptr, ctypes.byref(w), None, 0, None), b"descriptor"),
            (lambda: lib.sgk_convq_rollout_trans(env._h.ptr, ctypes.byref(w), None, 0, 0.0, 0, 3, 0), b"descriptor"),
            (lambda: lib.sgk_convq_rollout_trans(env._h.ptr, ctypes.byref(w), ctypes.byref(tr), 0, 0.0, 0, 3, 0), b"prev_boards_dev"),
            (lambda: lib.sgk_convq_rollout_trans(env._h.ptr, ctypes.byref(w), ctypes.byref(tr), 0, 0.0, 0, 3, 64), b"prev_boards_dev"),
            (lambda: lib.sgk_convq_act_trans(other._h.ptr, ctypes.byref(w), ctypes.byref(tr), 0.0, 0, None, None), b"5 x 5"),
        ):
            assert call() == _lib.ERR_INVALID and message in lib.sgk_last_error(), message
        tr.actions_out_dev = None
        assert lib.sgk_convq_act_trans(env._h.ptr, ctypes.byref(w), ctypes.byref(tr), 0.0, 0, None, None) == _lib.ERR_INVALID
        torch.cuda.synchronize()
        _same_bytes(before, _handle_state(env), "a refused call")
        assert (actions == 9).all() and prev.cpu().numpy().tobytes() == prev_before.tobytes()
    finally:
        env.close()
        other.close()


def test_the_agent_refuses_what_has_no_two_channel_kernel():
    _torch()
    args = types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=8, rollouts=4, epochs=1, clipping=0.2, entropy_bonus=0.01, critic_coeff=1.0,
                                 n_layers=2, n_channels=5, n_hidden=None, device=0, log_gradients=False, cheat=False, seed=1)
    env = S.BatchedGridworldEnv(TR.LEVEL, 4, seed=1)
    sok = S.BatchedGridworldEnv("SideEffectsSokoban-v0", 4, seed=1)
    try:
        for make, message in (
            (lambda: S.BatchedPPOAgent(env, args, body="mlp", transitions=True), "body"),
            (lambda: S.BatchedPPOAgent(env, args, body="cnn", transitions=True, fused_conv_learn=True), "fused_conv_learn"),
            (lambda: S.BatchedPPOAgent(env, args, body="cnn", transitions=True, fused_conv=False), "two-channel"),
            (lambda: S.BatchedPPOAgent(sok, args, body="cnn", transitions=True), "two-channel"),
            (lambda: S.BatchedPPOAgent(env, types.SimpleNamespace(**{**vars(args), "n_channels": 6}), body="cnn", transitions=True), "two-channel"),
            (lambda: S.BatchedPPOAgent(env, types.SimpleNamespace(**{**vars(args), "n_layers": 3}), body="cnn", transitions=True), "two-channel"),
        ):
            with pytest.raises(ValueError, match=message):
                make()
        agent = S.BatchedPPOAgent(env, args, body="cnn", transitions=True)
        assert tuple(agent.net.network[0][0].weight.shape) == (5, 2, 3, 3) and tuple(agent.net.bottleneck.weight.shape) == (5, 2, 1, 1)
        assert tuple(env.observation_space.shape) == (1, 5, 5)
        agent.fused_rollout = False  # the per-step loops would not keep prev_boards: refused, not run on a stale board
        for call in (agent.gather_rollout, lambda: S.batched_default_eval(agent, env, 5)):
            with pytest.raises(ValueError, match="fused rollout alone"):
                call()
    finally:
        env.close()
        sok.close()


# ---- 7. the one-channel paths are what they were ------------------------------------------------------------------------------------
def test_without_the_new_keywords_the_calls_are_the_old_ones():
    torch = _torch()
    C, T, n = 5, 8, TR.N
    env, twin = _env(n), _env(n)
    try:
        arrays = TR.weights("real", C, 7800)
        one = _dev(torch, [a[:, :1].copy() if k in ("w1", "wb") else a for k, a in zip(NAMES, arrays)])
        w = env._convq_weights(one, C, 2)
        t = {"states": torch.zeros((T, n, 25), dtype=torch.int8, device="cuda"), "actions": torch.zeros((T, n), dtype=torch.uint8, device="cuda"),
             "recs": torch.zeros((T, n, 4), dtype=torch.int8, device="cuda")}
        b = {k: v.clone() for k, v in t.items()}
        env.convq_rollout(one, T, C, mode="sample", draw_index0=3, auto_reset=True, states=b["states"], actions=b["actions"], recs=b["recs"])
        twin._sync_torch_to_lib()  # the entry point itself, as the binding called it before the keywords existed
        _lib.check(twin.lib.sgk_convq_rollout(twin._h.ptr, ctypes.byref(w), 1, 0.0, 3, T, _lib.F_AUTO_RESET, ctypes.c_void_p(t["states"].data_ptr()),
                                              ctypes.c_void_p(t["actions"].data_ptr()), ctypes.c_void_p(t["recs"].data_ptr())))
        twin._sync_lib_to_torch()
        torch.cuda.synchronize()
        for k in b:
            assert b[k].cpu().numpy().tobytes() == t[k].cpu().numpy().tobytes(), k
        assert (env.boards() == twin.boards()).all()
    finally:
        env.close()
        twin.close()


def _crmdp_args(n):
    return types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=16, rollouts=n, epochs=2, clipping=0.2, entropy_bonus=0.01, critic_coeff=1.0,
                                 n_layers=2, n_channels=5, n_hidden=None, device=0, log_gradients=False, cheat=False, seed=3, env_alias="trans-boat")


def test_a_default_crmdp_gather_is_the_one_channel_gather_and_the_transition_one_is_not():
    torch = _torch()
    n = 24
    out = {}
    for key, kw in (("default", {}), ("twin", {}), ("transitions", {"transitions": True})):
        env = S.BatchedGridworldEnv(TR.LEVEL, n, seed=7)
        try:
            torch.manual_seed(11)
            agent = S.BatchedPPOCRMDPAgent(env, _crmdp_args(n), on_unbounded="keep", **kw)
            assert agent.transitions == bool(kw)
            ro = agent.gather_rollout()
            torch.cuda.synchronize()
            assert hasattr(ro, "prev_states") == bool(kw) and len(ro) == 5 + bool(kw)
            out[key] = {k: getattr(ro, k).cpu().numpy() for k in ("states", "actions", "rewards", "returns", "lengths")}
            out[key]["boards"] = env.boards_host()
            if kw:
                ps, st, ln = ro.prev_states.cpu().numpy(), out[key]["states"], out[key]["lengths"]
                assert (ps[0] == st[0]).all()  # behind the gather's reset: [board, board]
                for e in range(n):
                    assert (ps[1:ln[e], e] == st[:ln[e] - 1, e]).all()  # then the board of the step before
                assert (agent.prev_boards == env.boards().reshape(n, -1)).all()
                agent.learn(ro)  # the torch path on [B, 2, H, W]
                agent.sync()
                torch.cuda.synchronize()
                assert all(bool(torch.isfinite(p).all()) for p in agent.net.parameters())
        finally:
            env.close()
    _same_bytes(out["default"], out["twin"], "the default gather")
