"""A population of independent PPO-CNN agents -- sgk_convq_rollout_members / sgk_ppo_cnn_epochs_members, BatchedPPOCNNPopulation -- on the
GPU. The rollout kernel's pass holds ENVS = 512 / (H * (W + 1)) envs (17 on BoatRace, 12 on Sokoban, 9 on the 6x8 boards, 7 on
DistributionalShift); the shapes below are chosen around it.

1. one member leaves the bytes of the existing calls: the members entry points with n_members = 1 against sgk_convq_rollout /
   sgk_ppo_cnn_epochs;
2. a member is a separate run, bit for bit: member m of a population == a BatchedPPOAgent(body="cnn", fused_conv_learn=True) on a handle
   of E envs created at env_index_base + m * E with member m's weights;
3. more members than resident workgroups (1 100 members of 3 envs);
4. a member reproduces the REFERENCE's own run (tests/golden/batched_ppo_cnn_*.npz) while its neighbours run something else;
5. learn() recorded in a graph as the first call on a fresh handle == the eager calls;
6. what cannot run is refused with the reason and touches nothing;
7. a caller's row that is not the member's own trains on the member's first row.

Run on the GPU box:  python -m pytest tests/test_gpu_ppo_cnn_members.py -m gpu -q
"""
import ctypes
import types

import numpy as np
import pytest

import batched_golden as BG
import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib
from safe_grid_agents_amd import ppo_cnn_population as PC

pytestmark = pytest.mark.gpu

SUMS = [_lib.M_SUM_RETURN, _lib.M_SUM_SAFETY, _lib.M_SUM_MARGIN, _lib.M_SUM_MARGIN_POS, _lib.M_EPISODES, _lib.M_MARGIN_POS_COUNT]
MAXS = [_lib.M_MAX_RETURN, _lib.M_MAX_SAFETY, _lib.M_MAX_MARGIN, _lib.M_MAX_MARGIN_POS]


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _args(C=5, batch=64, epochs=3, rollouts=8, layers=2, seed=5, **hyper):
    kw = dict(lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01)
    kw.update(hyper)
    return types.SimpleNamespace(discount=0.99, batch_size=batch, rollouts=rollouts, epochs=epochs, n_layers=layers, n_hidden=None,
                                 n_channels=C, device=0, log_gradients=False, cheat=False, seed=seed, **kw)


def _handle_state(env):
    """Everything a rollout leaves in the handle: boards, last step records, the decoded state words, the episode arrays, the metrics."""
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


def _rollout_bytes(ro):
    return {k: getattr(ro, k).cpu().numpy() for k in ("states", "actions", "rewards", "returns", "lengths")}


def _random_weights(torch, rng, members, cells, C, dev):
    """The rollout kernel's ten tensors stacked [M, ...], seeded (scale: logits that are neither flat nor saturated)."""
    shapes = {"w1": (C, 1, 3, 3), "b1": (C,), "w2": (C, C, 3, 3), "b2": (C,), "wb": (C, 1, 1, 1), "bb": (C,), "wh": (C, C, 3, 3), "bh": (C,),
              "wl": (4, C * cells), "bl": (4,)}
    return {k: torch.as_tensor(rng.normal(0.0, 0.05 if k == "wl" else 0.3, (members,) + s).astype(np.float32)).to(dev)
            for k, s in shapes.items()}


def _sentinel_buffers(torch, steps, n, cells, dev):
    return {"states": torch.full((steps, n, cells), 77, dtype=torch.int8, device=dev),
            "actions": torch.full((steps, n), 77, dtype=torch.uint8, device=dev),
            "recs": torch.full((steps, n, 4), 77, dtype=torch.int8, device=dev)}


def _agent(env, args, state_dict=None):
    agent = S.BatchedPPOAgent(env, args, body="cnn", fused_conv_learn=True)
    assert agent.fused_conv and agent.fused_learn and agent.fused_rollout
    if state_dict is not None:
        agent.net.load_state_dict(state_dict)
        agent.sync()
    return agent


def _agent_learner_state(agent):
    named, pl = dict(agent.net.named_parameters()), agent._pl
    out = {"stats": agent._stats.cpu().numpy(), "step": pl["step"].cpu().numpy()[0]}
    for i, (key, k) in enumerate(zip(agent.CNN_PARAMS, PC.PARAMS)):
        out.update({k: named[key].data.cpu().numpy(), "m_" + k: pl["m"][i].cpu().numpy(), "v_" + k: pl["v"][i].cpu().numpy()})
    return out


def _member_learner_state(pop, m):
    out = {"stats": pop.stats[m].cpu().numpy(), "step": pop.step.cpu().numpy()[m]}
    for i, k in enumerate(PC.PARAMS):
        out.update({k: pop.cur[k][m].cpu().numpy(), "m_" + k: pop.adam_m[i][m].cpu().numpy(), "v_" + k: pop.adam_v[i][m].cpu().numpy()})
    return out


ONE_MEMBER_LEVELS = [("BoatRace-v0", 5), ("SideEffectsSokoban-v0", 8), ("WhiskyGold-v0", 4)]  # WhiskyGold: per-env draws of its own


# ---- 1. one member leaves the bytes of the existing calls ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sample", "greedy"])
@pytest.mark.parametrize("name,C", ONE_MEMBER_LEVELS)
def test_one_member_rollout_leaves_the_bytes_of_the_existing_call(name, C, mode):
    """N = 37 (more than one pass, the last partial), 12 steps from a state max_iterations - 7 random steps into the episodes (so that
    episodes end inside the 12 steps and the metrics and episode arrays move), auto-reset: sgk_convq_rollout_members(n_members = 1),
    the member instantiation of the kernel, == sgk_convq_rollout in every output (sentinel-filled buffers) and the handle."""
    torch = _torch()
    n, steps = 37, 12
    envs = [S.BatchedGridworldEnv(name, n, seed=21, env_index_base=300) for _ in range(2)]
    try:
        dev = "cuda:%d" % envs[0].device
        w = _random_weights(torch, np.random.default_rng(C), 1, envs[0].n_cells, C, dev)
        single = {k: v[0] for k, v in w.items()}
        got = []
        for i, env in enumerate(envs):
            env.step_random(int(env.info.max_iterations) - 7, auto_reset=True)
            buf = _sentinel_buffers(torch, steps, n, env.n_cells, dev)
            kw = dict(mode=mode, epsilon=0.25, draw_index0=1000, auto_reset=True, mask_finished=mode == "sample", **buf)
            if i == 0:
                env.convq_rollout(single, steps, C, **kw)
            else:
                env.convq_rollout_members(w, 1, steps, C, **kw)
            snap = _handle_state(env)
            snap.update({k: v.cpu().numpy() for k, v in buf.items()})
            got.append(snap)
        assert got[0]["metrics"][_lib.M_EPISODES] > 0  # episodes did end inside the launch
        assert (got[0]["states"] != 77).all() and len(np.unique(got[0]["actions"])) > 1
        _same_bytes(got[0], got[1], (name, mode, C))
    finally:
        for env in envs:
            env.close()


@pytest.mark.parametrize("name,C", ONE_MEMBER_LEVELS)
def test_one_member_learner_leaves_the_bytes_of_the_existing_call(name, C):
    """N = 37: a BatchedPPOAgent's gather + sgk_ppo_cnn_epochs against a population of ONE member with the same weights and member_keys
    NULL (the handle's seed), two iterations: rollout, the 14 tensors, Adam's state, step, statistics and drawn rows bit for bit."""
    torch = _torch()
    n, args = 37, _args(C=C, batch=33, epochs=3, rollouts=37)
    e1, e2 = (S.BatchedGridworldEnv(name, n, seed=21, env_index_base=300) for _ in range(2))
    try:
        torch.manual_seed(4)
        agent = _agent(e1, args)
        pop = S.BatchedPPOCNNPopulation(e2, args, 1)
        pop.load_member(0, agent.net.state_dict())
        pop.member_keys = None  # NULL: the handle's seed
        rows1 = torch.zeros((3, 33), dtype=torch.int64, device=agent.device)
        rows2 = torch.zeros((1, 3, 33), dtype=torch.int64, device=agent.device)
        for it in range(2):
            r1, r2 = agent.gather_rollout(), pop.gather_rollout()
            _same_bytes(_rollout_bytes(r1), _rollout_bytes(r2), ("rollout", it))
            agent._learn_fused_cnn(r1, rows_out=rows1)
            pop.learn(r2, rows_out=rows2)
            a, b = _agent_learner_state(agent), _member_learner_state(pop, 0)
            a["rows"], b["rows"] = rows1.cpu().numpy(), rows2[0].cpu().numpy()
            assert int(a["step"]) == 3 * (it + 1) and np.abs(a["m_w1"]).max() > 0 and np.isfinite(a["stats"]).all()
            _same_bytes(a, b, ("learn", it))
            agent.sync(); pop.sync()
    finally:
        e1.close(); e2.close()


# ---- 2. a member is a separate run, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,members,E,C,batch,epochs", [
    ("BoatRace-v0", 3, 5, 5, 7, 3),             # a member smaller than a pass; rows of 25 bytes: members 1 and 2 start unaligned
    ("BoatRace-v0", 2, 19, 5, 64, 2),           # one full pass of 17 plus a partial pass of 2
    ("SideEffectsSokoban-v0", 2, 14, 8, 2, 3),  # the second sprite; batch 2: B - 1 = 1; 12 + 2 envs
    ("WhiskyGold-v0", 3, 5, 4, 37, 2),          # the level with draws of its own per env, keyed by the global env index
])
def test_a_member_is_a_separate_run_bit_for_bit(name, members, E, C, batch, epochs):
    """Two PPO iterations (gather, learn, sync; the second gather under the learned weights) of a population against one
    BatchedPPOAgent(body="cnn", fused_conv_learn=True) per member on a handle of its own: BatchedGridworldEnv(level, E, seed,
    env_index_base = base + m * E), member m's weights, member_keys = [seed] * M (the key the agent's handle draws its rows with)."""
    torch = _torch()
    seed, base = 9, 1000
    args = _args(C=C, batch=batch, epochs=epochs, rollouts=E)
    env = S.BatchedGridworldEnv(name, members * E, seed=seed, env_index_base=base)
    singles = [S.BatchedGridworldEnv(name, E, seed=seed, env_index_base=base + m * E) for m in range(members)]
    try:
        pop = S.BatchedPPOCNNPopulation(env, args, members, member_seeds=[31 + m for m in range(members)], member_keys=[seed] * members)
        agents = [_agent(e, args, pop.member(m).state_dict()) for m, e in enumerate(singles)]
        assert not torch.equal(pop.cur["w2"][0], pop.cur["w2"][1])  # the members did start from different weights
        N, dev = members * E, pop.device
        used = torch.zeros((members, epochs, batch), dtype=torch.int64, device=dev)
        used_m = torch.zeros((epochs, batch), dtype=torch.int64, device=dev)
        for it in range(2):
            env.metrics_reset()
            pop.reset_member_metrics()
            ro = pop.gather_rollout()
            gained = env.metrics()
            per_member = pop.member_metrics.cpu().numpy()
            assert gained[_lib.M_EPISODES] == N
            assert (per_member[:, SUMS].sum(0) == gained[SUMS]).all(), (per_member, gained)
            assert (per_member[:, MAXS].max(0) == gained[MAXS]).all(), (per_member, gained)
            pop.learn(ro, rows_out=used)
            for m, (e, agent) in enumerate(zip(singles, agents)):
                e.metrics_reset()
                rm = agent.gather_rollout()
                sl = slice(m * E, (m + 1) * E)
                mine = {"states": ro.states[:, sl], "actions": ro.actions[:, sl], "rewards": ro.rewards[sl], "returns": ro.returns[sl],
                        "lengths": ro.lengths[sl]}
                _same_bytes(_rollout_bytes(rm), {k: v.contiguous().cpu().numpy() for k, v in mine.items()}, ("rollout", it, m))
                alone = e.metrics()
                assert (per_member[m, SUMS] == alone[SUMS]).all() and (per_member[m, MAXS] == alone[MAXS]).all(), (it, m)
                agent._learn_fused_cnn(rm, rows_out=used_m)
                rows = used[m].cpu().numpy()
                t, col = rows // N, rows % N
                assert ((col >= m * E) & (col < (m + 1) * E)).all(), (it, m)  # a member draws from its own trajectories
                assert (t * E + (col - m * E) == used_m.cpu().numpy()).all(), (it, m)
                a, b = _agent_learner_state(agent), _member_learner_state(pop, m)
                assert int(a["step"]) == epochs * (it + 1) and np.isfinite(a["stats"]).all()
                _same_bytes(a, b, ("learn", it, m))
                agent.sync()
            pop.sync()
    finally:
        env.close()
        for e in singles:
            e.close()


# ---- 3. more members than resident workgroups ---------------------------------------------------------------------------------------
def test_more_members_than_resident_workgroups():
    """1 100 members of 3 envs (a grid of 1 100 workgroups: more than the chip holds at once), 12 steps, WhiskyGold with 5 channels,
    sampling with auto-reset from a handle max_iterations - 7 steps into its episodes. All members carry the SAME weights, so the
    launch must leave what sgk_convq_rollout leaves with those weights, byte for byte."""
    torch = _torch()
    members, E, steps, C = 1100, 3, 12, 5
    envs = [S.BatchedGridworldEnv("WhiskyGold-v0", members * E, seed=4) for _ in range(2)]
    try:
        dev, n = "cuda:%d" % envs[0].device, members * E
        single = {k: v[0].contiguous() for k, v in _random_weights(torch, np.random.default_rng(1), 1, envs[0].n_cells, C, dev).items()}
        stacked = {k: v.unsqueeze(0).repeat((members,) + (1,) * v.dim()).contiguous() for k, v in single.items()}
        got = []
        for i, env in enumerate(envs):
            env.step_random(int(env.info.max_iterations) - 7, auto_reset=True)
            buf = _sentinel_buffers(torch, steps, n, env.n_cells, dev)
            kw = dict(mode="sample", draw_index0=5, auto_reset=True, **buf)
            if i == 0:
                env.convq_rollout(single, steps, C, **kw)
            else:
                env.convq_rollout_members(stacked, members, steps, C, **kw)
            snap = _handle_state(env)
            snap.update({k: v.cpu().numpy() for k, v in buf.items()})
            got.append(snap)
        assert got[0]["metrics"][_lib.M_EPISODES] > 0  # at least one episode ended
        assert (got[1]["states"] != 77).all()
        _same_bytes(got[0], got[1], "1 100 members")
    finally:
        for env in envs:
            env.close()


# ---- 4. a member reproduces the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BG.PPO_CNN_FIXTURES)
def test_a_member_reproduces_the_reference_ppo_cnn_run(name, members=3, index=1):
    """tests/golden/batched_ppo_cnn_*.npz (the reference's train() with PPOCNNAgent, rollout r = env index base + r) as member 1 of a
    population of 3 whose handle starts at base - n: lengths, actions, states, rewards exact, returns bit for bit; with the
    reference's minibatch rows (fixture row t * n + r = population row t * N + index * n + r), losses and the 14 tensors after each
    iteration to rtol 2e-3 / atol 2e-5 -- the tolerance test_fused_cnn_learner_reproduces_the_reference_ppo_cnn_run holds the single
    learner to --, then its greedy evaluation books the fixture's episodes; while the other members, the fixture's initial weights plus
    a seeded perturbation, run beside it. The two *_gather fixtures hold gathers only."""
    from oracle import oracle as O

    torch = _torch()
    fx = BG.PpoFixture(name)
    meta, T, n = fx.meta, fx.horizon, fx.n
    assert meta["agent"] == "ppo-cnn"
    N = members * n
    assert fx.base - index * n >= 0
    env = S.BatchedGridworldEnv(fx.env, N, seed=fx.seed, env_index_base=fx.base - index * n)
    try:
        args = fx.args(0)
        args.seed = fx.seed
        pop = S.BatchedPPOCNNPopulation(env, args, members, member_keys=[fx.seed + 1000 * m for m in range(members)])
        rng = np.random.default_rng(17)
        for m in range(members):
            sd = {k: torch.as_tensor(v if m == index else (v + 0.02 * rng.standard_normal(v.shape)).astype(np.float32))
                  for k, v in fx.weights(0).items() if not k.startswith("old_policy.")}
            pop.load_member(m, sd)
        pop.sync()
        sl = slice(index * n, (index + 1) * n)
        epochs, batch = meta["epochs"], meta["batch_size"]
        used = torch.zeros((members, epochs, batch), dtype=torch.int64, device=pop.device)
        for k in range(fx.iterations):
            env.metrics_reset()
            pop.reset_member_metrics()
            ro = pop.gather_rollout(cheat=fx.cheat)
            assert tuple(ro.actions.shape) == (T, N)
            lengths = ro.lengths[sl].cpu().numpy()
            assert (lengths == fx.it(k, "lengths")).all(), (k, lengths, fx.it(k, "lengths"))
            got_actions = ro.actions[:, sl].cpu().numpy().T
            bad = np.argwhere(got_actions != fx.it(k, "actions"))
            assert bad.size == 0, (k, bad[:4], [float(fx.it(k, "margins")[i, t]) for i, t in bad[:4]])
            assert (ro.states[:, sl].cpu().numpy().transpose(1, 0, 2) == fx.it(k, "states")).all(), k
            assert (ro.rewards[sl].cpu().numpy() == fx.it(k, "rewards")).all(), k
            assert ro.returns[sl].contiguous().cpu().numpy().tobytes() == fx.it(k, "returns").tobytes(), k
            want = fx.gather_metrics(k)
            vec = pop.member_metrics[index].cpu().numpy()
            for key, col in (("sum_return", O.M_SUM_RETURN), ("sum_safety", O.M_SUM_SAFETY), ("sum_margin", O.M_SUM_MARGIN),
                             ("sum_margin_pos", O.M_SUM_MARGIN_POS), ("episodes", O.M_EPISODES), ("margin_pos_count", O.M_MARGIN_POS_COUNT)):
                assert int(vec[col]) == want[key], (k, key, int(vec[col]), want[key])
            if fx.learn:
                # the reference's rows index the valid (step, rollout) pairs in step-major order; every member takes them in its own columns
                valid_t, valid_r = np.nonzero(np.arange(T)[:, None] < fx.it(k, "lengths")[None, :])
                ref = np.asarray(fx.it(k, "rows")).astype(np.int64)
                assert ref.shape == (epochs, batch)
                own_lengths = ro.lengths.cpu().numpy().reshape(members, n)
                rows = np.zeros((members, epochs, batch), dtype=np.int64)
                for m in range(members):
                    t, r = valid_t[ref], valid_r[ref]
                    if m != index:  # (a neighbour's episodes have other lengths: keep its rows inside them)
                        t = np.minimum(t, own_lengths[m][r] - 1)
                    rows[m] = t * N + m * n + r
                pop.learn(ro, rows=torch.as_tensor(rows).to(pop.device), rows_out=used)
                assert (used.cpu().numpy() == rows).all(), k
                stats = pop.stats.cpu().numpy().astype(np.float64)
                np.testing.assert_allclose(stats[index], fx.losses(k), rtol=2e-3, atol=2e-5)
                sd = PC.unstack_state_dict(pop.cur, index)
                for key, v in fx.weights(k + 1).items():
                    np.testing.assert_allclose(sd[key].cpu().numpy(), v, rtol=2e-3, atol=2e-5, err_msg="%s after iteration %d" % (key, k))
                for m in range(members):  # the neighbours learned something else
                    assert m == index or not np.array_equal(stats[m], stats[index])
            pop.sync()
        per_member, total = pop.evaluate(fx.eval_timesteps)
        BG.assert_eval_metrics(per_member[index].vec, fx, O)
        assert per_member[index].episodes == sum(len(a["eval_episodes"]) for a in fx.agents)
        assert total.episodes == sum(bm.episodes for bm in per_member)
    finally:
        env.close()


# ---- 5. capture ---------------------------------------------------------------------------------------------------------------------
def test_learn_captured_as_the_first_call_on_a_fresh_handle_equals_the_eager_calls():
    """Two populations with the same seeds on two handles. The first gathers a rollout and learns on it twice, eagerly. On the second
    handle nothing has run when pop.learn is recorded under torch.cuda.graph (one stream, the default queue setting); the graph is
    replayed twice from the restored initial state: after each replay every output is bit-identical to the eager calls'."""
    torch = _torch()
    members, E, args = 3, 5, _args(C=5, batch=7, epochs=3, rollouts=5)
    env, fresh = (S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=6) for _ in range(2))
    try:
        pop = S.BatchedPPOCNNPopulation(env, args, members)
        ro = pop.gather_rollout()
        used = torch.zeros((members, 3, 7), dtype=torch.int64, device=pop.device)

        def outputs(p, rows):
            out = {k: t.cpu().numpy() for k, t in p.tensors().items()}
            out.update(rows=rows.cpu().numpy(), stats=p.stats.cpu().numpy())
            return out

        eager = []
        for call in range(2):
            pop.learn(ro, rows_out=used)
            eager.append(outputs(pop, used))
        assert (eager[0]["step"] == 3).all() and (eager[1]["step"] == 6).all()
        assert np.abs(eager[0]["m_w1"]).max() > 0 and eager[0]["rows"].any() and not np.array_equal(eager[0]["rows"], eager[1]["rows"])

        pop2 = S.BatchedPPOCNNPopulation(fresh, args, members)  # (the constructor asks the handle for the workspace size: no launch)
        used2 = torch.zeros_like(used)
        start = {k: t.clone() for k, t in pop2.tensors().items()}
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            pop2.learn(ro, rows_out=used2)
        for k, t in pop2.tensors().items():  # (recording ran nothing)
            assert torch.equal(t, start[k]), k
            t.copy_(start[k])
        used2.zero_(); pop2.stats.zero_()
        for replay in range(2):
            graph.replay()
            torch.cuda.synchronize()
            _same_bytes(eager[replay], outputs(pop2, used2), ("replay", replay))
    finally:
        env.close(); fresh.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_what_cannot_run_is_refused_with_the_reason_and_touches_nothing():
    """n_envs % n_members != 0 and n_members < 1 (the C entry points, the env methods, the constructor), 6 channels, a batch of 65 and
    of 1, three layers, a NULL workspace, a rows tensor of the wrong shape: an SgkError / ValueError that says why, and nothing
    launched (weights, step counters, metrics and the handle untouched)."""
    torch = _torch()
    env = S.BatchedGridworldEnv("BoatRace-v0", 15, seed=6)
    try:
        base = dict(C=5, batch=7, epochs=2, rollouts=5)
        pop = S.BatchedPPOCNNPopulation(env, _args(**base), 3)
        ro = pop.gather_rollout()
        before = {k: t.clone() for k, t in pop.tensors().items()}
        metrics_before = pop.member_metrics.clone()
        handle = _handle_state(env)
        lib, dev = env.lib, pop.device
        acting = pop._acting_weights(pop.old)
        w = env._member_convq_weights(acting, 3, 5, 2)
        for bad in (2, 4, 0, -1):
            rc = lib.sgk_convq_rollout_members(env._h.ptr, ctypes.byref(w), bad, 1, 0.0, 0, 5, 0, None, None, None, None)
            assert rc == _lib.ERR_INVALID and b"n_members" in lib.sgk_last_error(), (bad, lib.sgk_last_error())
            with pytest.raises((_lib.SgkError, ValueError), match="n_members"):
                env.convq_rollout_members(acting, bad, 5, 5)
            with pytest.raises(ValueError, match="n_members"):
                S.BatchedPPOCNNPopulation(env, _args(**base), bad)
        w3 = env._member_convq_weights(acting, 3, 5, 3)  # what sgk_convq_rollout refuses is refused too
        rc = lib.sgk_convq_rollout_members(env._h.ptr, ctypes.byref(w3), 3, 1, 0.0, 0, 5, 0, None, None, None, None)
        assert rc == _lib.ERR_INVALID and b"n_layers" in lib.sgk_last_error()
        rc = lib.sgk_convq_rollout_members(env._h.ptr, ctypes.byref(w), 3, 2, 0.0, 0, 5, 0, None, None, None, None)
        assert rc == _lib.ERR_INVALID and b"mode" in lib.sgk_last_error()
        with pytest.raises(ValueError, match="weights"):  # a stack of the wrong member count never reaches the kernel
            env.convq_rollout_members(acting, 5, 5, 5)

        # the learner: a filled sgk_ppo_cnn_learner the library would accept, then one thing wrong at a time
        C, cells, M = 5, env.n_cells, 4
        sizes = (9 * C, C, 9 * C * C, C, C, C, 9 * C * C, C, 4 * C * cells, 4, 9 * C * C, C, C * cells, 1)
        keep = [torch.zeros((M, s), dtype=torch.float32, device=dev) for s in sizes]
        step = torch.zeros(M, dtype=torch.int64, device=dev)
        ws = torch.zeros(env.ppo_cnn_members_workspace_bytes(5, 64, M), dtype=torch.uint8, device=dev)
        assert env.ppo_cnn_members_workspace_bytes(5, 7, 3) >= 3 * env.ppo_cnn_workspace_bytes(5, 7)

        def learner(channels=5, batch=7, workspace=True):
            L = _lib.SgkPpoCnnLearner()
            L.states, L.actions, L.returns, L.lengths = (ro.states.data_ptr(), ro.actions.data_ptr(), ro.returns.data_ptr(), ro.lengths.data_ptr())
            L.horizon, L.n_channels, L.batch, L.n_epochs, L.n_trajectories = ro.actions.shape[0], channels, batch, 2, 15
            for i, t in enumerate(keep):
                L.params[i], L.m[i], L.v[i] = t.data_ptr(), t.data_ptr(), t.data_ptr()
            for i in range(10):
                L.old_params[i] = keep[i].data_ptr()
            L.step = step.data_ptr()
            if workspace:
                L.workspace = ws.data_ptr()
            L.lr, L.beta1, L.beta2, L.eps, L.clipping, L.critic_coeff, L.entropy_bonus = 1e-3, 0.9, 0.999, 1e-8, 0.2, 1.0, 0.01
            return L

        for L, members, reason in ((learner(), 2, b"n_members"), (learner(), 4, b"n_members"), (learner(), 0, b"n_members"),
                                   (learner(), -1, b"n_members"), (learner(channels=6), 3, b"n_channels"), (learner(batch=65), 3, b"batch"),
                                   (learner(batch=1), 3, b"batch"), (learner(workspace=False), 3, b"workspace")):
            rc = lib.sgk_ppo_cnn_epochs_members(env._h.ptr, ctypes.byref(L), members, None)
            assert rc == _lib.ERR_INVALID and reason in lib.sgk_last_error(), (members, lib.sgk_last_error())
        for bad in (2, 4, 0, -1):
            with pytest.raises((_lib.SgkError, ValueError), match="n_members"):
                env.ppo_cnn_epochs_members(learner(), bad)
        for channels, batch, members in ((6, 7, 3), (5, 65, 3), (5, 1, 3), (5, 7, 0)):
            assert lib.sgk_ppo_cnn_members_workspace_bytes(env._h.ptr, channels, batch, members) == -1 and lib.sgk_last_error()
            with pytest.raises(_lib.SgkError):
                env.ppo_cnn_members_workspace_bytes(channels, batch, members)
        for kw, reason in ((dict(C=6), "n_channels"), (dict(batch=65), "batch_size"), (dict(batch=1), "batch_size"), (dict(layers=3), "n_layers")):
            with pytest.raises(ValueError, match=reason):
                S.BatchedPPOCNNPopulation(env, _args(**dict(base, **kw)), 3)
        with pytest.raises(ValueError, match="rows"):  # a tensor argument of the wrong shape never reaches the kernels
            pop.learn(ro, rows=torch.zeros((3, 2, 6), dtype=torch.int64, device=dev))
        with pytest.raises(ValueError, match="rollout.states"):
            pop.learn(ro._replace(states=ro.states.to(torch.float32)))
        torch.cuda.synchronize()
        assert int(step.abs().sum()) == 0 and all(int((t != 0).sum()) == 0 for t in keep) and int((ws != 0).sum()) == 0
        for k, t in pop.tensors().items():
            assert torch.equal(t, before[k]), k
        assert torch.equal(pop.member_metrics, metrics_before)
        _same_bytes(handle, _handle_state(env), "after the refusals")
    finally:
        env.close()


# ---- 7. a foreign or out-of-range caller's row ----------------------------------------------------------------------------------------
def test_a_row_that_is_not_the_members_own_trains_on_the_members_first_row():
    """Caller's rows with entries below zero, at and beyond the rollout's end, far outside int32 and in other members' trajectories:
    learn() leaves the bytes of the same call with each such entry replaced by the member's first row, 0 * N + m * E (which
    rows_out reports)."""
    torch = _torch()
    members, E, epochs, batch = 3, 5, 2, 7
    env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=6)
    try:
        pop = S.BatchedPPOCNNPopulation(env, _args(C=5, batch=batch, epochs=epochs, rollouts=E), members)
        ro = pop.gather_rollout()
        T, N = ro.actions.shape
        lengths = ro.lengths.cpu().numpy()
        rng = np.random.default_rng(3)
        clean = np.zeros((members, epochs, batch), dtype=np.int64)
        for m in range(members):
            col = m * E + rng.integers(0, E, (epochs, batch))
            clean[m] = rng.integers(0, lengths[col]) * N + col
        dirty = clean.copy()
        foreign = lambda m, t: t * N + ((m + 1) % members) * E + 2  # noqa: E731  (a valid row of the NEXT member's)
        bad = {(0, 0, 0): -1, (0, 1, 3): T * N, (1, 0, 2): T * N + 5, (1, 1, 6): 2 ** 62, (2, 0, 1): foreign(2, 1), (0, 0, 5): foreign(0, 0),
               (1, 0, 0): -(2 ** 40), (2, 1, 4): 1 * N + 2 * E - 1}  # (the last: member 1's last trajectory, handed to member 2)
        for (m, e, b), row in bad.items():
            dirty[m, e, b] = row
            clean[m, e, b] = m * E
        start = {k: t.clone() for k, t in pop.tensors().items()}
        got = []
        for rows in (clean, dirty):
            for k, t in pop.tensors().items():
                t.copy_(start[k])
            used = torch.full((members, epochs, batch), -7, dtype=torch.int64, device=pop.device)
            pop.learn(ro, rows=torch.as_tensor(rows).to(pop.device), rows_out=used)
            out = {k: t.cpu().numpy() for k, t in pop.tensors().items()}
            out.update(rows=used.cpu().numpy(), stats=pop.stats.cpu().numpy())
            got.append(out)
        assert (got[0]["rows"] == clean).all() and (got[0]["step"] == epochs).all() and np.isfinite(got[0]["stats"]).all()
        _same_bytes(got[0], got[1], "foreign rows")
    finally:
        env.close()


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def test_the_trainer_runs_a_ppo_cnn_population():
    """`boat ppo-cnn -r 5 -e 2 -b 7 --members 3`: two training periods and the evaluations of a BatchedPPOCNNPopulation over N = 15 envs;
    every member learned (2 periods x 2 epochs), the aggregate meters and the per-member histograms are written."""
    torch = _torch()
    args = S.prepare_parser().parse_args(["-S", "3", "-E", "2", "-EE", "2", "-V", "120", "boat", "ppo-cnn", "-l", "0.001", "-r", "5", "-e", "2",
                                          "-b", "7", "--members", "3"])
    writers = []

    def wf(d):
        writers.append(S.RecordingWriter(d))
        return writers[-1]

    agent, env = S.train_batched(args, writer_factory=wf)
    try:
        assert isinstance(agent, S.BatchedPPOCNNPopulation) and env.n_envs == 15 and agent.n_members == 3
        assert (agent.step.cpu().numpy() == 4).all() and torch.isfinite(agent.stats).all()
        tags = {c[1] for c in writers[0].calls}
        assert {"Train/policy_loss", "Train/member_return", "Train/member_safety"} <= tags and any(t.startswith("Evaluation/") for t in tags), tags
    finally:
        env.close()
