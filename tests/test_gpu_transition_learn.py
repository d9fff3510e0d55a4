"""The fused learner of the two-board conv body (sgk_ppo_cnn_epochs_trans: the CIN = 2 instantiations of ppo_cnn_forward_kernel,
ppo_cnn_backward_kernel and ppo_cnn_adam_kernel; BatchedPPOAgent(transitions=True, fused_transition_learn=True)).

(a) one epoch from zero Adam state against the float64 reference of tests/transition_learner_reference.py, with the bounds of
    tests/test_gpu_ppo_cnn_gradients.py quantity by quantity: m / (1 - beta1) is the kernel's gradient, per tensor err_k =
    max|g_k - g64| / max|g64| <= max(8 err_t, 16 x 2^-23) and <= 1e-5 (err_t: torch-float32 autograd's error on the same inputs), every
    element of all 14 tensors counted; the three statistics by the same rule; v = (1 - beta2) g_k^2; step == 1; nothing NaN; the old
    policy's bytes unchanged.
(b) Adam from an injected state at step 4 999 fed the kernel's own gradient, against adam64.
(c) two epochs in one call equal two calls of one epoch bit for bit, rows_out included; a call recorded in a graph replays to the eager
    call's bytes.
(d) the in-kernel draws on a ragged rollout are valid rows, and for the same seed, step and lengths they are the rows
    sgk_ppo_cnn_epochs draws on a one-channel agent.
(e) the reference's own `ppo-crmdp -r 6` run (tests/golden/batched_ppo_crmdp_transboat.npz) with this learner in the loop: every gather
    exact -- from iteration 1 on under the weights this learner produced --, losses and weights to rtol 2e-3 / atol 2e-5, the evaluation's
    episodes booked exactly.
(f) against torch autograd on the same two-channel agent over two learn() calls of 3 epochs, with _assert_adam_close's rule of
    tests/test_gpu_ppo_cnn_learn.py (restated here: importing that file's rule would be fine, but the rule is part of this test).
(g) guard bands (tests/guard_arena.py) around every writable field of the learner struct, the workspace of exactly the advertised size.
(h) refusals leave parameters, Adam state and the step counter unchanged as bytes.

Inputs of (a)-(d): transition_learner_reference.trans_inputs -- 3 steps x 37 trajectories, both planes seeded integers 0..5 drawn
independently, so that a swapped, dropped or duplicated plane changes w1's and wb's gradients. Each figure of (a) and (b) is printed
before it is asserted (TRANS_LEARN lines).

Measured on an MI355X: over the 98 gradient tensors of the seven cases the median err_k / err_t is 1.06, the worst 7.6; of the gradients
and statistics the closest to its limit is trans-BoatRace-c5-b64 'grad ba' at 0.28 of it (6.7e-7 against 2.3e-6); of everything,
step B's update of 'w2' at trans-BoatRace-c8-b64, 0.47 of its allowance. profiles/transition_learn/mutations.log: three one-line mutants
of csrc/sgk_ppo_cnn.hip, each caught by (a) -- plane 0 staged from the current board in the backward kernel only on 'grad w1' and
'grad wb' alone, with every forward-only quantity passing."""
import ctypes
import types

import numpy as np
import pytest

import batched_golden as BG
import learner_child as LC
import learner_reference as R
import safe_grid_agents_amd as S
import test_gpu_guard_bands as GB
import test_gpu_learner_gradients as G
import test_gpu_ppo_cnn_gradients as PG
import transition_learner_reference as TL
from safe_grid_agents_amd import _lib

pytestmark = pytest.mark.gpu

F64 = np.float64
RAGGED_STEP = PG.RAGGED_STEP
GOLDEN = "batched_ppo_crmdp_transboat.npz"


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _args(case, epochs):
    return types.SimpleNamespace(discount=0.99, batch_size=case.batch, rollouts=1, epochs=epochs, n_layers=2, n_hidden=None,
                                 n_channels=case.channels, device=0, log_gradients=False, cheat=False, **R.ppo_cnn_hyper(case))


def make_agent(case, env, epochs):
    """A two-channel BatchedPPOAgent on the fused learner whose own and old-policy parameters are the case's seeded tensors."""
    agent = S.BatchedPPOAgent(env, _args(case, epochs), body="cnn", transitions=True, fused_transition_learn=True)
    assert agent.fused_learn and agent.fused_conv and agent.transitions
    d = TL.yardstick(case)[0]
    PG._put(PG._old(agent), d["old"])
    PG._put(PG._own(agent), d["cur"])
    return agent


def rollout(agent, d, lengths=None, prev=True):
    torch = _torch()
    ro = {k: torch.as_tensor(d[k]).to(agent.device) for k in ("states", "actions", "returns") + (("prev_states",) if prev else ())}
    ro["lengths"] = torch.as_tensor(d["lengths"] if lengths is None else lengths).to(agent.device)
    return types.SimpleNamespace(**ro)


def _open_env():
    env = S.BatchedGridworldEnv(TL.ENV, R.N_ENVS, seed=3)
    env.bind_torch_stream()
    return env


def run_case(case):
    """Step A (zero Adam state) and step B (injected state, step 4 999) on the case's seeded rollout."""
    torch = _torch()
    d = TL.yardstick(case)[0]
    env = _open_env()
    try:
        agent = make_agent(case, env, 1)
        ro = rollout(agent, d)
        out = {"old_before": PG._cpu(PG._old(agent))}
        agent.learn(ro, None, rows=[d["rows"]])  # (every (t, trajectory) pair is valid: the index into the valid pairs is the flat row)
        pl = agent._pl
        out["stats"] = [agent._stats.cpu().numpy()[0].copy()]
        out["m_a"], out["v_a"], out["w_a"] = PG._cpu(pl["m"]), PG._cpu(pl["v"]), PG._cpu(PG._own(agent))
        out["step_a"] = [pl["step"].cpu().numpy().copy()]
        out["old_after"] = PG._cpu(PG._old(agent))
        g_c = [m.astype(F64) / R.one_minus_beta1() for m in out["m_a"]]
        ms, vs, _ = R.inject_adam_state(g_c, LC.STATE_SEED + case.seed, False)
        PG.set_state(agent, ro, d["cur"], ms, vs, LC.STEP_BEFORE_B)
        agent.learn(ro, None, rows=[d["rows"]])
        out["m_b"], out["v_b"], out["w_b"] = PG._cpu(pl["m"]), PG._cpu(pl["v"]), PG._cpu(PG._own(agent))
        out["step_b"] = [pl["step"].cpu().numpy().copy()]
        torch.cuda.synchronize()
    finally:
        env.close()
    return out


def result(case):
    return G._once(("ppo-cnn-trans", case), lambda: run_case(case))


def figures_a(case, out):
    d, r64, err_t = TL.yardstick(case)
    stats = out["stats"][0]
    return G._figures_a(TL.TENSORS, out, r64["grads"], err_t, [(k,) + R.cnn_stat_pair(case, r64, i, stats[i]) for i, k in enumerate(TL.STATS)])


def figures_b(case, out):
    state = R.inject_adam_state(G._clipped_gradient(out), LC.STATE_SEED + case.seed, False)
    return G._figures_b(TL.TENSORS, TL.yardstick(case)[0]["cur"], out, state, R.ppo_cnn_hyper(case)["lr"])


def _show(case, step, figs):
    for f in figs:
        print("TRANS_LEARN %s %s %-18s measured=%.3e limit=%.3e err_t=%s" % (
            TL.case_id(case), step, f[0], f[1], f[2], "-" if f[3] is None else "%.3e" % f[3]), flush=True)


# ---- (a), (b) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TL.CASES, ids=TL.case_id)
def test_gradients_and_statistics_against_float64(case):
    out = result(case)
    figs = figures_a(case, out)
    _show(case, "A", figs)
    G._finite(out, ("m_a", "v_a", "w_a", "stats"))
    assert int(out["step_a"][0][0]) == 1
    d = TL.yardstick(case)[0]
    assert len(out["m_a"]) == 14 and [tuple(m.shape) for m in out["m_a"]] == TL.param_shapes(case.channels)
    for k, a, b in zip(TL.TENSORS, out["old_before"], out["old_after"]):
        assert a.tobytes() == b.tobytes(), k  # the old policy, bit for bit
    for k, a, b in zip(TL.TENSORS, out["old_before"], d["old"]):
        assert (a.reshape(b.shape) == b).all(), k
    assert len(figs) == 2 * 14 + 3
    G._check(figs)


@pytest.mark.parametrize("case", TL.CASES, ids=TL.case_id)
def test_adam_from_injected_state(case):
    out = result(case)
    figs = figures_b(case, out)
    _show(case, "B", figs)
    G._finite(out, ("m_b", "v_b", "w_b"))
    assert int(out["step_b"][0][0]) == LC.STEP_BEFORE_B + 1
    G._check(figs)


# ---- (c), (d) -------------------------------------------------------------------------------------------------------------------------
def _restore(agent, snap):
    PG._put(PG._own(agent), snap["w"])
    PG._put(agent._pl["m"], snap["m"])
    PG._put(agent._pl["v"], snap["v"])
    agent._pl["step"].fill_(int(snap["step"][0][0]))


def run_plumbing_case(case):
    torch = _torch()
    d, r64, _ = TL.yardstick(case)
    env = _open_env()
    try:
        two, one = make_agent(case, env, 2), make_agent(case, env, 1)
        ro = rollout(one, d)
        ms, vs, _ = R.inject_adam_state(r64["grads"], LC.STATE_SEED + case.seed, False)
        start = (d["cur"], ms, vs, LC.STEP_BEFORE_B)
        out = {}
        rows_out = torch.full((2, case.batch), -1, dtype=torch.int64, device=two.device)
        PG.set_state(two, ro, *start)
        two._learn_fused_cnn(ro, rows=[d["rows"], d["rows2"]], rows_out=rows_out)
        out["two"] = dict(PG._snapshot(two), stats=two._stats.cpu().numpy().copy(), rows_out=rows_out.cpu().numpy().copy())
        PG.set_state(one, ro, *start)
        stats, used = [], []
        for rows in (d["rows"], d["rows2"]):
            got = torch.full((1, case.batch), -1, dtype=torch.int64, device=one.device)
            one._learn_fused_cnn(ro, rows=[rows], rows_out=got)
            stats.append(one._stats.cpu().numpy()[0].copy())
            used.append(got.cpu().numpy()[0].copy())
        out["one"] = dict(PG._snapshot(one), stats=np.stack(stats), rows_out=np.stack(used))
        # the graph: the two-epoch agent drawing its own rows on the ragged rollout, eager, then recorded and replayed from the same state
        ragged = rollout(two, d, d["ragged_lengths"])
        drawn = torch.full((2, case.batch), -1, dtype=torch.int64, device=two.device)
        PG.set_state(two, ragged, *start)
        before = PG._snapshot(two)
        two._learn_fused_cnn(ragged, rows_out=drawn)
        torch.cuda.synchronize()
        out["eager"] = dict(PG._snapshot(two), stats=two._stats.cpu().numpy().copy(), rows_out=drawn.cpu().numpy().copy())
        _restore(two, before)
        drawn.fill_(-1)
        two._stats.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            two._learn_fused_cnn(ragged, rows_out=drawn)
        _restore(two, before)
        drawn.fill_(-1)
        two._stats.zero_()
        graph.replay()
        torch.cuda.synchronize()
        out["replay"] = dict(PG._snapshot(two), stats=two._stats.cpu().numpy().copy(), rows_out=drawn.cpu().numpy().copy())
        # (d): the kernel's own draws, and a one-channel agent's on the same handle, step, lengths and batch
        zeros = [np.zeros_like(p) for p in d["cur"]]
        got = torch.full((1, case.batch), -1, dtype=torch.int64, device=one.device)
        PG.set_state(one, ragged, d["cur"], zeros, zeros, RAGGED_STEP)
        one._learn_fused_cnn(ragged, rows_out=got)
        out["ragged"] = {"rows": got.cpu().numpy()[0].copy(), "stats": one._stats.cpu().numpy()[0].copy(), "step": int(one._pl["step"].item())}
        plain = S.BatchedPPOAgent(env, _args(case, 1), body="cnn", fused_conv_learn=True)
        assert plain.fused_learn and not plain.transitions
        ro1 = rollout(plain, d, d["ragged_lengths"], prev=False)
        plain._cnn_learner(ro1)
        plain._pl["step"].fill_(RAGGED_STEP)
        got1 = torch.full((1, case.batch), -1, dtype=torch.int64, device=plain.device)
        plain._learn_fused_cnn(ro1, rows_out=got1)
        out["ragged_one_channel"] = got1.cpu().numpy()[0].copy()
        torch.cuda.synchronize()
    finally:
        env.close()
    return out


def plumbing_result(case):
    return G._once(("ppo-cnn-trans plumbing", case), lambda: run_plumbing_case(case))


def _same_bytes(a, b):
    for key in ("w", "m", "v", "step"):
        for k, x, y in zip(TL.TENSORS, a[key], b[key]):
            assert np.isfinite(x).all() and x.tobytes() == y.tobytes(), (key, k)
    assert np.isfinite(a["stats"]).all() and a["stats"].tobytes() == b["stats"].tobytes()
    assert a["rows_out"].tobytes() == b["rows_out"].tobytes()


@pytest.mark.parametrize("case", TL.PLUMBING_CASES, ids=TL.case_id)
def test_two_epochs_in_one_call_equal_two_calls_of_one_epoch_bit_for_bit(case):
    d = TL.yardstick(case)[0]
    res = plumbing_result(case)
    two, one = res["two"], res["one"]
    _same_bytes(two, one)
    assert int(two["step"][0][0]) == LC.STEP_BEFORE_B + 2
    assert not (two["stats"][0] == two["stats"][1]).all()  # (two different epochs)
    want = np.stack([d["rows"], d["rows2"]])
    assert (two["rows_out"] == want).all() and (one["rows_out"] == want).all()
    assert any((a != b).any() for a, b in zip(two["w"], d["cur"]))


@pytest.mark.parametrize("case", TL.PLUMBING_CASES, ids=TL.case_id)
def test_a_recorded_call_replays_to_the_eager_calls_bytes(case):
    d = TL.yardstick(case)[0]
    res = plumbing_result(case)
    _same_bytes(res["replay"], res["eager"])
    assert int(res["replay"]["step"][0][0]) == LC.STEP_BEFORE_B + 2
    assert (res["eager"]["rows_out"] >= 0).all()
    assert any((a != b).any() for a, b in zip(res["eager"]["w"], d["cur"]))


@pytest.mark.parametrize("case", TL.PLUMBING_CASES, ids=TL.case_id)
def test_in_kernel_draws_are_valid_and_do_not_depend_on_the_channel_count(case):
    d = TL.yardstick(case)[0]
    res = plumbing_result(case)
    lengths = d["ragged_lengths"]
    assert (lengths == 0).any() and 3 * int(lengths.sum()) >= TL.T * TL.N
    rows = res["ragged"]["rows"]
    assert rows.shape == (case.batch,) and (rows >= 0).all() and (rows < TL.T * TL.N).all()
    t, n = rows // TL.N, rows % TL.N
    assert (t < lengths[n]).all()
    assert len(np.unique(rows)) > case.batch // 4  # (draws, not a constant)
    assert res["ragged"]["step"] == RAGGED_STEP + 1 and np.isfinite(res["ragged"]["stats"]).all()
    assert (res["ragged_one_channel"] == rows).all()
    # the graph run drew on the same lengths at steps 4 999 and 5 000: valid rows too
    for r in res["eager"]["rows_out"]:
        assert ((r // TL.N) < lengths[r % TL.N]).all()


# ---- (e) the reference's own run --------------------------------------------------------------------------------------------------------
def test_the_reference_run_with_the_fused_transition_learner():
    """tests/test_gpu_transition_golden.py::test_the_transition_agent_reproduces_the_reference_run with learn() on the device. Nothing is
    excluded: every gather element, every loss and every weight is compared."""
    from oracle import oracle as O

    import test_gpu_transition_golden as TG

    torch = _torch()
    fx = BG.PpoFixture(GOLDEN)
    m, n = fx.meta, fx.n
    env = S.BatchedGridworldEnv(fx.env, n, seed=fx.seed, env_index_base=fx.base)
    env.bind_torch_stream()
    agent = S.BatchedPPOCRMDPAgent(env, TG._args(fx), transitions=True, fused_transition_learn=True)
    try:
        assert agent.transitions and agent.fused_conv and agent.fused_rollout and agent.fused_learn
        agent.net.load_state_dict({k: torch.as_tensor(v).to(agent.device) for k, v in fx.weights(0).items()}, strict=False)
        agent.sync()
        env.reset()
        for k in range(fx.iterations):
            env.metrics_reset()
            ro = agent.gather_rollout(cheat=fx.cheat)
            assert (ro.lengths.cpu().numpy() == fx.it(k, "lengths")).all(), k
            bad = np.argwhere(ro.actions.cpu().numpy().T != fx.it(k, "actions"))
            assert bad.size == 0, (k, bad[:4], [float(fx.it(k, "margins")[i, t]) for i, t in bad[:4]])
            assert (ro.states.cpu().numpy().transpose(1, 0, 2) == fx.it(k, "states")).all(), k
            assert (ro.prev_states.cpu().numpy().transpose(1, 0, 2) == fx.it(k, "prev_states")).all(), k
            assert (agent._buffers["rewards"].cpu().numpy() == fx.it(k, "raw_rewards")).all(), k
            assert (ro.rewards.cpu().numpy() == fx.it(k, "rewards")).all(), k
            assert ro.returns.cpu().numpy().tobytes() == fx.it(k, "returns").tobytes(), k
            stats = agent.stats()
            assert stats["replaced_rewards"] == m["replaced_rewards"][k] and stats["first_unbounded"] == -1
            for mine, theirs in ((agent.memory.flag, "mem_flag"), (agent.memory.reward, "mem_reward"), (agent.memory.bound, "mem_rllb")):
                want = fx.it(k, theirs)
                got = mine[0].cpu().numpy()
                known = fx.it(k, "mem_flag") != 0 if theirs == "mem_reward" else np.ones_like(want, dtype=bool)
                assert (got[known] == want[known]).all(), (k, theirs)
            TG._metrics_agree(env.metrics(), fx.gather_metrics(k), O)
            w = S.RecordingWriter()
            step = 0 if agent._pl is None else int(agent._pl["step"].item())
            agent.learn(ro, {"writer": w, "t": 0, "t_learn": 0}, rows=list(fx.it(k, "rows")))
            assert int(agent._pl["step"].item()) == step + m["epochs"]  # (the fused path ran)
            got = np.array([float.fromhex(c[2]) for c in w.calls]).reshape(m["epochs"], 3)
            np.testing.assert_allclose(got, fx.losses(k), rtol=2e-3, atol=2e-5)
            sd = agent.net.state_dict()
            for key, v in fx.weights(k + 1).items():
                np.testing.assert_allclose(sd[key].cpu().numpy(), v, rtol=2e-3, atol=2e-5, err_msg="%s after iteration %d" % (key, k))
            agent.sync()
        bm = S.batched_default_eval(agent, env, fx.eval_timesteps)
        BG.assert_eval_metrics(bm.vec, fx, O)
        assert bm.episodes == sum(len(a["eval_episodes"]) for a in fx.agents)
    finally:
        env.close()


# ---- (f) against torch autograd ---------------------------------------------------------------------------------------------------------
def _assert_adam_close(got, want, steps, lr, what):
    """tests/test_gpu_ppo_cnn_learn.py's rule as it stands: parameters after Adam steps within rtol 2e-3 / atol 2e-5; an element whose
    gradient in some epoch is ~0 moves by lr g / (|g| + eps) in a direction set by fp32 rounding in either implementation -- such
    elements, at most 5 % of a tensor, only have to stay within Adam's largest possible move."""
    got, want = got.cpu().numpy(), want.cpu().numpy()
    off = ~np.isclose(got, want, rtol=2e-3, atol=2e-5)
    assert off.mean() <= 0.05, (what, off.mean(), np.abs(got - want).max())
    assert (np.abs(got - want)[off] <= 2 * lr * steps + 2e-5).all(), what


def _trans_agent(env, C, batch, fused, epochs=3):
    torch = _torch()
    torch.manual_seed(3)
    args = types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=batch, rollouts=1, epochs=epochs, clipping=0.2, entropy_bonus=0.01,
                                 critic_coeff=1.0, n_layers=2, n_hidden=None, n_channels=C, device=0, log_gradients=False, cheat=False)
    return S.BatchedPPOAgent(env, args, body="cnn", transitions=True, fused_transition_learn=fused)


@pytest.mark.parametrize("C,batch", [(5, 64), (8, 2)])
def test_fused_transition_learner_equals_torch_autograd(C, batch):
    """A seeded init, one gathered rollout, the same rows: two learn() calls of 3 epochs (Adam's step counter crosses the calls) by
    sgk_ppo_cnn_epochs_trans and by torch autograd + torch.optim.Adam on the same two-channel network: the same statistics (the
    tolerances of test_fused_cnn_learner_equals_torch_autograd) and, by _assert_adam_close, the same 14 tensors."""
    torch = _torch()
    env = S.BatchedGridworldEnv(TL.ENV, 64, seed=11)
    env.bind_torch_stream()
    try:
        fused, ref = _trans_agent(env, C, batch, True), _trans_agent(env, C, batch, False)
        assert fused.fused_learn and not ref.fused_learn
        ref.net.load_state_dict(fused.net.state_dict())
        ro = fused.gather_rollout()
        assert ro.prev_states.shape == ro.states.shape and not torch.equal(ro.prev_states, ro.states)
        gen = torch.Generator().manual_seed(7)
        n_valid = int(ro.lengths.sum().item())
        own = lambda a: {k: v.data for k, v in a.net.named_parameters() if k in a.CNN_PARAMS}  # noqa: E731
        for call in range(2):
            rows = [torch.randint(n_valid, (batch,), generator=gen) for _ in range(3)]
            fused.learn(ro, rows=rows)
            w = S.RecordingWriter()
            ref.learn(ro, {"writer": w, "t": 0, "t_learn": 0}, rows=rows)
            want = np.array([float.fromhex(c[2]) for c in w.calls]).reshape(3, 3)
            got = fused._stats.cpu().numpy().astype(np.float64)
            np.testing.assert_allclose(got[:, 1:], want[:, 1:], rtol=1e-4, atol=1e-6, err_msg="value loss / entropy of call %d" % call)
            np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-4, atol=1e-5, err_msg="policy loss of call %d" % call)
            a, b = own(fused), own(ref)
            assert len(a) == 14
            for k in fused.CNN_PARAMS:
                _assert_adam_close(a[k], b[k], 3 * (call + 1), 1e-3, "%s after call %d" % (k, call))
        assert int(fused._pl["step"].item()) == 6
    finally:
        env.close()


# ---- (g) guard bands --------------------------------------------------------------------------------------------------------------------
def trans_body(C, batch, rows_mode, epochs=2):
    """sgk_ppo_cnn_epochs_trans with every pointer of sgk_ppo_cnn_learner and prev_states carved; w1 / wb (and their moments and old
    copies) have the two-plane sizes, the workspace exactly sgk_ppo_cnn_trans_workspace_bytes bytes."""
    torch = _torch()
    T = 5

    def body(env, A):
        lib, cells, n = env.lib, env.n_cells, env.n_envs
        rng = np.random.default_rng(cells * 1000 + C + batch)
        L = _lib.SgkPpoCnnLearner()
        lengths = np.array([(5, 1, 2, 0)[(i + i // 4) % 4] for i in range(n)], dtype=np.int32)
        L.states = A.inp("states", torch.as_tensor(rng.integers(0, 5, (T, n, cells)).astype(np.int8))).data_ptr()
        prev = A.inp("prev_states", torch.as_tensor(rng.integers(0, 5, (T, n, cells)).astype(np.int8)))
        L.actions = A.inp("actions", torch.as_tensor(rng.integers(0, 4, (T, n)).astype(np.uint8))).data_ptr()
        L.returns = A.inp("returns", GB._f32(torch, rng, (n, T), 1.0)).data_ptr()
        L.lengths = A.inp("lengths", torch.as_tensor(lengths)).data_ptr()
        L.horizon, L.n_channels, L.batch, L.n_epochs, L.n_trajectories = T, C, batch, epochs, n
        shapes = dict(zip(GB.CNN_PARAMS, TL.param_shapes(C, cells)))
        assert shapes[GB.CNN_PARAMS[0]] == (C, 2, 3, 3) and shapes[GB.CNN_PARAMS[4]] == (C, 2, 1, 1)
        for i, k in enumerate(GB.CNN_PARAMS):
            L.params[i] = A.state(k, GB._f32(torch, rng, shapes[k], 0.2)).data_ptr()
            for name, arr, t in zip(("m", "v"), (L.m, L.v), GB._adam_state(torch, rng, shapes[k], False)):
                arr[i] = A.state("%s_%s" % (name, k), t).data_ptr()
        for i, k in enumerate(GB.CNN_PARAMS[:10]):
            L.old_params[i] = A.inp("old_" + k, GB._f32(torch, rng, shapes[k], 0.2)).data_ptr()
        step = A.state("step", torch.full((1,), 300, dtype=torch.int64))
        L.step = step.data_ptr()
        L.stats_out = A.out("stats_out", (epochs, 3), torch.float32).data_ptr()
        rows_out = A.out("rows_out", (epochs, batch), torch.int64)
        L.rows_out = rows_out.data_ptr()
        L.lr, L.beta1, L.beta2, L.eps, L.clipping, L.critic_coeff, L.entropy_bonus = 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.5, 0.02
        if rows_mode == "given":
            rows = rng.choice(np.flatnonzero(lengths > 0), (epochs, batch))
            rows = A.inp("rows", torch.as_tensor(rows.astype(np.int64)))
            L.rows = rows.data_ptr()
        need = env.ppo_cnn_trans_workspace_bytes(C, batch)
        assert need == TL.workspace_bytes(C, batch) and need > env.ppo_cnn_workspace_bytes(C, batch)
        L.workspace = A.scratch("workspace", need).data_ptr()
        GB._call(env, lib.sgk_ppo_cnn_epochs_trans, ctypes.byref(L), GB._ptr(prev))
        torch.cuda.synchronize()
        assert bool((step == 300 + epochs).all())
        r = rows_out.reshape(epochs * batch).cpu().numpy()
        if rows_mode == "given":
            assert torch.equal(rows_out, rows)
        else:
            assert ((r // n) < lengths[r % n]).all()

    return body


@pytest.mark.parametrize("pattern", GB.PATTERNS)
@pytest.mark.parametrize("C,batch,rows_mode", [(4, 2, "null"), (5, 37, "null"), (8, 37, "null"), (8, 64, "null"), (5, 37, "given")])
def test_guard_bands_around_the_transition_learner(C, batch, rows_mode, pattern):
    GB.check_case("ppo_cnn/trans/5x5/C%d/B%d/rows_%s" % (C, batch, rows_mode), pattern, GB._env(GB.BOAT, 8), trans_body(C, batch, rows_mode),
                  arena_bytes=16 << 20)


# ---- (h) refusals, the workspace and the Python surface --------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 5, 8])
@pytest.mark.parametrize("batch", [2, 64])
def test_the_workspace_size_is_the_headers_formula(C, batch):
    env = S.BatchedGridworldEnv(TL.ENV, 8, seed=2)
    try:
        assert env.ppo_cnn_trans_workspace_bytes(C, batch) == TL.workspace_bytes(C, batch)
        assert env.ppo_cnn_trans_workspace_bytes(C, batch) - env.ppo_cnn_workspace_bytes(C, batch) == 4 * batch * 10 * C
    finally:
        env.close()


def _state_bytes(agent):
    pl = agent._pl
    return [t.cpu().numpy().tobytes() for t in list(PG._own(agent)) + list(pl["m"]) + list(pl["v"]) + [pl["step"]]]


def test_refusals_raise_and_touch_nothing():
    """A NULL prev_states, a Sokoban handle, C = 6, batch 1 and 65 raise the library's SGK_ERR_INVALID, a wrong-sized network.0.0.weight
    the binding's ValueError; parameters, Adam state and the step counter keep their bytes; the workspace query refuses the same shapes."""
    torch = _torch()
    case = TL.CASES[1]
    d = TL.yardstick(case)[0]
    env = _open_env()
    sokoban = S.BatchedGridworldEnv("SideEffectsSokoban-v0", 8, seed=2)
    sokoban.bind_torch_stream()
    try:
        agent = make_agent(case, env, 1)
        ro = rollout(agent, d)
        agent.learn(ro, None, rows=[d["rows"]])
        torch.cuda.synchronize()
        before = _state_bytes(agent)

        def refused(env_, L, prev, code=_lib.ERR_INVALID):
            with pytest.raises(_lib.SgkError) as ei:
                env_.ppo_cnn_epochs_trans(L, prev)
            assert ei.value.code == code

        L, _ = agent._cnn_learner(ro)
        refused(env, L, None)
        with pytest.raises(_lib.SgkError):  # the raw symbol with a NULL pointer
            _lib.check(env.lib.sgk_ppo_cnn_epochs_trans(env.handle, ctypes.byref(L), None))
        # a Sokoban handle (6 x 6): the one-board call's shape, not this one's (prev_states sized for that board)
        prev6 = torch.zeros((TL.T, TL.N, sokoban.n_cells), dtype=torch.int8, device=agent.device)
        refused(sokoban, L, prev6)
        for field, value in (("n_channels", 6), ("batch", 1), ("batch", 65)):
            L, _ = agent._cnn_learner(ro)
            setattr(L, field, value)
            refused(env, L, ro.prev_states)
        # a wrong-sized network.0.0.weight: the one-channel tensor where 18 C floats are read
        own = dict(agent.net.named_parameters())
        conv1 = own["network.0.0.weight"]
        keep = conv1.data
        conv1.data = keep[:, 1:2].contiguous()
        with pytest.raises(ValueError, match="network.0.0.weight"):
            agent.learn(ro, None, rows=[d["rows"]])
        conv1.data = keep
        with pytest.raises(ValueError, match="prev_states"):
            env.ppo_cnn_epochs_trans(agent._cnn_learner(ro)[0], ro.prev_states[:, :, :24])
        torch.cuda.synchronize()
        assert _state_bytes(agent) == before
        for e, C, batch in ((env, 6, 16), (env, 5, 65), (env, 5, 1), (sokoban, 5, 16)):
            with pytest.raises(_lib.SgkError):
                e.ppo_cnn_trans_workspace_bytes(C, batch)
        assert sokoban.ppo_cnn_workspace_bytes(5, 16) > 0  # (the one-board learner does run there)
    finally:
        sokoban.close()
        env.close()


def test_the_keyword_chooses_the_path():
    env = S.BatchedGridworldEnv(TL.ENV, 8, seed=2)
    env.bind_torch_stream()
    try:
        case = TL.CASES[1]
        with pytest.raises(ValueError, match="fused_transition_learn"):
            S.BatchedPPOAgent(env, _args(case, 1), body="cnn", fused_transition_learn=True)
        with pytest.raises(ValueError, match="fused_conv_learn"):
            S.BatchedPPOAgent(env, _args(case, 1), body="cnn", transitions=True, fused_conv_learn=True)
        assert not S.BatchedPPOAgent(env, _args(case, 1), body="cnn", transitions=True).fused_learn
        assert S.BatchedPPOAgent(env, _args(case, 1), body="cnn", transitions=True, fused_transition_learn=True).fused_learn
        big = S.BatchedPPOAgent(env, _args(case._replace(batch=128), 1), body="cnn", transitions=True, fused_transition_learn=True)
        assert not big.fused_learn  # (outside 2 .. 64: the torch path, as fused_conv_learn)
        one = S.BatchedPPOAgent(env, _args(case._replace(batch=1), 1), body="cnn", transitions=True, fused_transition_learn=True)
        assert not one.fused_learn
    finally:
        env.close()
