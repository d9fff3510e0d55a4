"""Counters past 2^32. The lockstep counter `t` and the draw index are uint64 in the ABI and each goes into ONE 32-bit Philox word
-- (uint32_t)(t >> 6) for the random actions (64 two-bit actions per block), (uint32_t)draw for the epsilon-greedy and the
categorical draw (sgk_draws.h: ctr = {env_lo, env_hi, draw, stream}) -- so a 32-bit temporary in any random-action path, or a
counter layout that differs between the device, the host helper and the oracle, shows only at these edges. 2^32 lockstep steps
are 25 minutes of rollout at 0.35 us a step: a normal run gets there. sgk_account_steps moves `t` there for free.

Lockstep counter: handles of 257 envs (BoatRace, and WhiskyGold whose own draws must NOT move with t) with a non-zero seed and
env_index_base are accounted to T0 = 2^32 - 5 and 2^38 - 5 and cross the edge eagerly (step_random(3)), through the graph replay
with the device counter (step_random(64)), in the fused rollout and in the streamed rollout into rings of both layouts with the
crossing inside one launch: state, records and every ring slice against the oracle from t_begin = T0, the actions against
sgk_random_action. At 2^38 the Philox word wraps: device == oracle == host helper there, and step 2^38 + k draws what step k draws.
No DeepQ / PPO agent reads `t`: their draws are keyed by draw indices of their own (checked: the package reads lockstep_t nowhere,
and step_one uses `t` for the random action alone), so there is no agent.step() to cross with.

Draw index: 2^32 - 1, 2^32, 2^32 + 5 and 2^63 as a host scalar and as the device scalar through env.epsilon_greedy,
env.categorical_sample, policy_act / policy_sample, convq_act / convq_sample, and policy_rollout / convq_rollout from draw_index0 =
2^32 - 3 over 8 steps, against the oracle's draw functions. Every case is exact, no margin excuses one: epsilon-greedy is an argmax
of float32 scores with clear gaps plus integer draws, and the categorical cases use logits that are exactly equal (e_i = 1,
partial sums 1, 2, 3, 4: the inverse CDF is floor(4 u) without a rounding), which the fused kernels get from a zero actor head.
Draw 2^32 + 5 is draw 5: the period include/sgk.h states (the oracle's half of that pin needs no device:
tests/test_state_sweep_cpu.py, test_the_oracles_draws_have_period_2_to_the_32).

Not reachable without new entry points (none is added here): the tabular agent's step counter `t` (sgk_tabq_* only advance it by
stepping), and the per-env reset counter n_resets, whose (uint32_t)epi << 7 wraps after 2^25 episodes of one env."""
import numpy as np
import pytest

import hostlib
import safe_grid_agents_amd as S
import state_sweep as SS
from oracle import oracle as O
from test_gpu_state_sweep import _assert_state, _same_bytes

pytestmark = pytest.mark.gpu

N, SEED, BASE, K = 257, 0xBEEF, (1 << 33) + 12345, 64
HORIZONS = {"2^32": 2**32 - 5, "2^38": 2**38 - 5}
LEVELS = ["BoatRace-v0", "WhiskyGold-v0"]
_TRACES = {}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _trace(name, T0):
    """The oracle's K steps from lockstep step T0, under the actions orc_random_action names; its own random rollout
    (orc.rollout(t_begin = T0)) ends in the same state, and the host helper names the same actions."""
    if (name, T0) not in _TRACES:
        tr = SS.trace(name, SEED, N, schedule=True, T=K, env_begin=BASE, t_begin=T0)
        own = O.EnvBatch(name, N, seed=SEED, env_begin=BASE)
        m = O.metrics_new()
        rec = own.rollout(K, seed=SEED, env_begin=BASE, t_begin=T0, auto_reset=True, metrics=m)
        assert (rec == tr.recs[K - 1]).all() and (own.boards() == tr.boards[K - 1]).all()
        assert m[:O.M_STEPS].tolist() == tr.metrics[:O.M_STEPS].tolist()
        L = hostlib.load()
        host = np.array([[L.sgk_random_action(SEED, BASE + i, T0 + k) for i in range(N)] for k in range(K)], dtype=np.uint8)
        assert (host == tr.actions).all()
        _TRACES[(name, T0)] = tr
    return _TRACES[(name, T0)]


def _env_at(name, T0, **kw):
    env = S.BatchedGridworldEnv(name, N, seed=SEED, env_index_base=BASE, **kw)
    env.account_steps(T0 - env.lockstep_t)
    assert env.lockstep_t == T0
    return env


def _assert_after(env, tr, k, T0, where):
    """The env after k + 1 steps from T0: records, boards, every state field, the counter and the metrics' episode sums."""
    _same_bytes(env.step_records_host(), tr.recs[k], where + " records")
    _assert_state(env, tr.boards[k], {key: v[k] for key, v in tr.fields.items()}, where)
    assert env.lockstep_t == T0 + k + 1, where
    if env.name == "BoatRace-v0":  # nothing replaces an action here: the record names the action the counter RNG drew
        assert (env.step_records_host()[:, 3].astype(np.uint8) == tr.actions[k]).all(), where


@pytest.mark.parametrize("name", LEVELS)
@pytest.mark.parametrize("horizon", sorted(HORIZONS))
def test_step_random_crosses_the_edge_eagerly_and_through_the_graph(name, horizon):
    _torch()
    T0 = HORIZONS[horizon]
    tr = _trace(name, T0)
    env = _env_at(name, T0)
    for call in range(4):  # fewer than 4 steps run eagerly: steps T0 .. T0 + 11, the edge in the second call
        env.step_random(3, auto_reset=True)
        _assert_after(env, tr, 3 * call + 2, T0, "%s %s eager call %d" % (name, horizon, call))
    env.close()
    env = _env_at(name, T0, layout="pitched")
    env.step_random(K, auto_reset=True)  # one graph replay of 64 launches that read the counter from the device
    _assert_after(env, tr, K - 1, T0, "%s %s graph" % (name, horizon))
    want = tr.metrics.copy()
    want[O.M_STEPS] = N * (T0 + K)  # sgk_account_steps books the steps it is told about: n_envs per lockstep step
    assert env.metrics().tolist() == want.tolist()
    env.close()


@pytest.mark.parametrize("name", LEVELS)
@pytest.mark.parametrize("horizon", sorted(HORIZONS))
def test_fused_rollout_crosses_the_edge_inside_one_launch(name, horizon):
    _torch()
    T0 = HORIZONS[horizon]
    tr = _trace(name, T0)
    env = _env_at(name, T0)
    env.step_random(10, auto_reset=True, fused=True)
    _assert_after(env, tr, 9, T0, "%s %s fused" % (name, horizon))
    env.step_random(K - 10, auto_reset=True, fused=True)
    _assert_after(env, tr, K - 1, T0, "%s %s fused, second launch" % (name, horizon))
    env.close()


@pytest.mark.parametrize("name", LEVELS)
@pytest.mark.parametrize("horizon", sorted(HORIZONS))
@pytest.mark.parametrize("layout", ["slice", "tile"])
def test_streamed_rollout_crosses_the_edge_inside_one_launch(name, horizon, layout):
    torch = _torch()
    T0 = HORIZONS[horizon]
    tr = _trace(name, T0)
    env = _env_at(name, T0)
    steps, ring = 12, 12
    n_tiles = (N + 63) // 64
    shape = (lambda x: (n_tiles, ring, 64, x)) if layout == "tile" else (lambda x: (ring, N, x))
    boards = torch.full(shape(env.n_cells), -7, dtype=torch.int8, device="cuda")
    recs = torch.full(shape(4), -7, dtype=torch.int8, device="cuda")
    env.rollout_random_stream(steps, boards=boards, recs=recs, first_slice=0, layout=layout)
    got_b = (env.ring_slices(boards) if layout == "tile" else boards).cpu().numpy()
    got_r = (env.ring_slices(recs) if layout == "tile" else recs).cpu().numpy()
    for k in range(steps):
        _same_bytes(got_b[k], tr.boards[k], "%s %s %s slice %d boards" % (name, horizon, layout, k))
        _same_bytes(got_r[k], tr.recs[k], "%s %s %s slice %d records" % (name, horizon, layout, k))
    _assert_after(env, tr, steps - 1, T0, "%s %s stream %s" % (name, horizon, layout))
    env.step_random(3, auto_reset=True, fused="stream")  # into the env's own buffers
    _assert_after(env, tr, steps + 2, T0, "%s %s stream, own buffers" % (name, horizon))
    env.close()


@pytest.mark.parametrize("name", LEVELS)
def test_the_random_actions_repeat_after_2_to_the_38_steps(name):
    """(uint32_t)(t >> 6) wraps at t = 2^38: step 2^38 + k draws what step k draws (the period sgk_step_random documents), on the
    device, in the oracle and in the host helper; the envs' own draws are keyed by episode and frame and do not move with t."""
    _torch()
    L = hostlib.load()
    for k in (0, 1, 63, 64, 12345):
        for i in (0, 7, N - 1):
            assert L.sgk_random_action(SEED, BASE + i, 2**38 + k) == L.sgk_random_action(SEED, BASE + i, k) == O.random_action(SEED, BASE + i, k)
    tr = _trace(name, HORIZONS["2^38"])
    first = SS.trace(name, SEED, N, schedule=True, T=K - 5, env_begin=BASE, t_begin=0)
    assert (tr.actions[5:] == first.actions).all()
    late, early = _env_at(name, 2**38), _env_at(name, 0)
    for k in range(8):
        late.step_random(1, auto_reset=True)
        early.step_random(1, auto_reset=True)
        _same_bytes(late.step_records_host(), early.step_records_host(), "%s step %d" % (name, k))
        _same_bytes(early.step_records_host(), first.recs[k], "%s step %d against the oracle" % (name, k))
        _same_bytes(late.boards_host(), early.boards_host(), "%s step %d boards" % (name, k))
    late.close(); early.close()


# ---- the draw index ----------------------------------------------------------------------------------------------------------------
DRAWS = [2**32 - 1, 2**32, 2**32 + 5, 2**63]
N_DRAW = 1000 + 37


def _device_scalar(torch, draw):
    """The 1-element int64 device tensor the launch reads the draw index from: the same 64 bits."""
    return torch.tensor([draw - 2**64 if draw >= 2**63 else draw], dtype=torch.int64, device="cuda")


def _clear_scores(rng, n):
    """float32 [n, 4]: a permutation of 0, 1, 2, 3 in every row (gaps of 1: the argmax is beyond doubt)."""
    return np.stack([rng.permutation(4) for _ in range(n)]).astype(np.float32)


def _mlp_weights(torch, env, zero_head, hidden=100):
    g = torch.Generator().manual_seed(3)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.3).to("cuda").contiguous()  # noqa: E731
    w = {"w1t": r(env.n_cells, hidden), "b1": r(hidden), "w2": r(hidden, hidden), "b2": r(hidden), "w3t": r(hidden, 4), "b3": r(4)}
    if zero_head:
        w["w3t"].zero_(); w["b3"].zero_()
    return w


def _conv_weights(torch, env, zero_head, C=5):
    g = torch.Generator().manual_seed(4)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.3).to("cuda").contiguous()  # noqa: E731
    w = {"w1": r(C, 1, 3, 3), "b1": r(C), "w2": r(C, C, 3, 3), "b2": r(C), "wb": r(C, 1, 1, 1), "bb": r(C), "wh": r(C, C, 3, 3), "bh": r(C),
         "wl": r(4, C * env.n_cells), "bl": r(4)}
    if zero_head:
        w["wl"].zero_(); w["bl"].zero_()
    return w


@pytest.mark.parametrize("draw", DRAWS)
def test_epsilon_greedy_and_categorical_sample_at_the_draw_index_edges(draw):
    torch = _torch()
    n = N_DRAW
    env = S.BatchedGridworldEnv("BoatRace-v0", n, seed=SEED, env_index_base=BASE)
    sc = _clear_scores(np.random.RandomState(1), n)
    scores = torch.as_tensor(sc, device="cuda")
    want = O.eps_greedy(sc, 0.5, SEED, BASE, draw)
    assert 0.25 < (want != sc.argmax(1)).mean() < 0.5  # about 3 / 8 of the envs explore away from the greedy action
    _same_bytes(env.epsilon_greedy(scores, 0.5, draw).cpu().numpy(), want, "epsilon_greedy, host scalar")
    eps_dev = torch.tensor([0.5], dtype=torch.float64, device="cuda")
    _same_bytes(env.epsilon_greedy(scores, eps_dev, _device_scalar(torch, draw)).cpu().numpy(), want, "epsilon_greedy, device scalar")
    zeros = np.zeros((n, 4), dtype=np.float32)
    logits = torch.as_tensor(zeros, device="cuda")
    want_c, _ = O.categorical_sample(zeros, SEED, BASE, draw)
    assert np.bincount(want_c, minlength=4).min() > n // 8
    _same_bytes(env.categorical_sample(logits, draw).cpu().numpy(), want_c, "categorical_sample, host scalar")
    _same_bytes(env.categorical_sample(logits, _device_scalar(torch, draw)).cpu().numpy(), want_c, "categorical_sample, device scalar")
    # the period: only the low 32 bits of the draw index reach the counter (ctr = {env_lo, env_hi, draw, stream})
    low = draw & 0xFFFFFFFF
    _same_bytes(env.epsilon_greedy(scores, 0.5, low).cpu().numpy(), want, "epsilon_greedy, draw mod 2^32")
    _same_bytes(env.categorical_sample(logits, low).cpu().numpy(), want_c, "categorical_sample, draw mod 2^32")
    env.close()


@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("body", ["mlp", "conv"])
def test_fused_forwards_draw_at_the_draw_index_edges(body, draw):
    """policy_act / convq_act: the oracle's epsilon-greedy on the kernel's own scores; policy_sample / convq_sample with a zero
    actor head: the kernel's logits are exactly 0 and the oracle's categorical draw on them is exact."""
    torch = _torch()
    n = N_DRAW
    env = S.BatchedGridworldEnv("IslandNavigation-v0", n, seed=SEED, env_index_base=BASE)
    env.step_random(9, auto_reset=True)
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    weights = _mlp_weights if body == "mlp" else _conv_weights
    act = (lambda w, e, d: env.policy_act(w, e, d, scores_out=out)) if body == "mlp" else (lambda w, e, d: env.convq_act(w, e, d, 5, scores_out=out))
    sample = (lambda w, d: env.policy_sample(w, d, logits_out=out)) if body == "mlp" else (lambda w, d: env.convq_sample(w, d, 5, logits_out=out))
    eps_dev = torch.tensor([0.5], dtype=torch.float64, device="cuda")
    for d, e, form in ((draw, 0.5, "host scalar"), (_device_scalar(torch, draw), eps_dev, "device scalar")):
        got = act(weights(torch, env, False), e, d).cpu().numpy()
        sc = out.cpu().numpy()
        srt = np.sort(sc, axis=1)
        assert (srt[:, 3] > srt[:, 2]).all()  # no ties: the greedy action is the kernel's own argmax, beyond doubt
        _same_bytes(got, O.eps_greedy(sc, 0.5, SEED, BASE, draw), "%s act, %s" % (body, form))
        got = sample(weights(torch, env, True), d).cpu().numpy()
        assert not out.cpu().numpy().any()
        _same_bytes(got, O.categorical_sample(np.zeros((n, 4), dtype=np.float32), SEED, BASE, draw)[0], "%s sample, %s" % (body, form))
    env.close()


@pytest.mark.parametrize("body", ["mlp", "conv"])
@pytest.mark.parametrize("mode", ["sample", "greedy"])
def test_fused_rollouts_cross_the_draw_index_edge(body, mode):
    """policy_rollout / convq_rollout from draw_index0 = 2^32 - 3 over 8 steps: step k draws with index 2^32 - 3 + k. "sample" with a
    zero actor head (logits exactly 0) and "greedy" at epsilon 1 (every env explores: the action is the draw's, whatever the
    scores) make every action the oracle's draw alone, exactly; the env then follows the oracle under those actions."""
    torch = _torch()
    n, T, draw0 = N_DRAW, 8, 2**32 - 3
    name = "IslandNavigation-v0"
    env = S.BatchedGridworldEnv(name, n, seed=SEED, env_index_base=BASE)
    w = (_mlp_weights if body == "mlp" else _conv_weights)(torch, env, mode == "sample")
    actions = torch.full((T, n), 9, dtype=torch.uint8, device="cuda")
    recs = torch.full((T, n, 4), 5, dtype=torch.int8, device="cuda")
    kw = dict(mode=mode, epsilon=1.0, draw_index0=draw0, auto_reset=True, actions=actions, recs=recs)
    if body == "mlp":
        env.policy_rollout(w, T, **kw)
    else:
        env.convq_rollout(w, T, 5, **kw)
    flat = np.zeros((n, 4), dtype=np.float32)
    want = np.stack([O.categorical_sample(flat, SEED, BASE, draw0 + k)[0] if mode == "sample" else O.eps_greedy(flat, 1.0, SEED, BASE, draw0 + k)
                     for k in range(T)])
    _same_bytes(actions.cpu().numpy(), want, "%s rollout %s actions" % (body, mode))
    assert (want[3:] == np.stack([O.categorical_sample(flat, SEED, BASE, k)[0] if mode == "sample" else O.eps_greedy(flat, 1.0, SEED, BASE, k)
                                  for k in range(T - 3)])).all()  # past the edge the draws are those of index 0, 1, ...
    tr = SS.trace(name, SEED, n, actions=want, schedule=True, env_begin=BASE)
    _same_bytes(recs.cpu().numpy(), tr.recs, "%s rollout %s records" % (body, mode))
    _assert_state(env, tr.boards[T - 1], {key: v[T - 1] for key, v in tr.fields.items()}, "%s rollout %s" % (body, mode))
    env.close()
