"""A population of independent PPO-MLP agents -- sgk_policy_rollout_members / sgk_ppo_epochs_members, BatchedPPOPopulation -- on the GPU:

1. one member IS the existing call: the members entry points with n_members = 1 leave the bytes sgk_policy_rollout / sgk_ppo_epochs leave;
2. a member is a separate run, bit for bit: member m of a population == a BatchedPPOAgent on a handle of E envs created at
   env_index_base + m * E with member m's weights (members that start unaligned, a last wave of 5 rows, two tiles per member with 2
   envs in the second; a workgroup that walks several tiles of its member);
3. a member reproduces the REFERENCE's own run (tests/golden/batched_ppo_*.npz) while its neighbours run something else;
4. a member's gradients and Adam meet tests/learner_reference.py's float64 bounds, as tests/test_gpu_learner_gradients.py applies them to
   the single learner (its helpers, imported), and the neighbours' results differ;
5. learn() replayed from a graph == the eager call; 6. what cannot run is refused with the reason.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import ctypes
import types

import numpy as np
import pytest

import batched_golden as BG
import learner_child as LC
import learner_reference as R
import safe_grid_agents_amd as S
import test_gpu_learner_gradients as G
from safe_grid_agents_amd import _lib
from safe_grid_agents_amd import ppo_population as PP

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _args(hidden=100, batch=64, epochs=3, rollouts=8, layers=2, seed=5, **hyper):
    kw = dict(lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01)
    kw.update(hyper)
    return types.SimpleNamespace(discount=0.99, batch_size=batch, rollouts=rollouts, epochs=epochs, n_layers=layers, n_hidden=hidden,
                                 n_channels=5, device=0, log_gradients=False, cheat=False, seed=seed, **kw)


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


def _random_weights(torch, rng, members, cells, hidden, dev):
    """Policy weights stacked [M, ...] in the fused kernels' layout, seeded (scale: logits that are neither flat nor saturated)."""
    shapes = {"w1t": (cells, hidden), "b1": (hidden,), "w2": (hidden, hidden), "b2": (hidden,), "w3t": (hidden, 4), "b3": (4,)}
    return {k: torch.as_tensor(rng.normal(0.0, 0.3, (members,) + s).astype(np.float32)).to(dev) for k, s in shapes.items()}


# ---- 1. one member is the existing call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [64, 100])
@pytest.mark.parametrize("mode", ["sample", "greedy"])
@pytest.mark.parametrize("name", ["BoatRace-v0", "WhiskyGold-v0"])
def test_one_member_rollout_leaves_the_bytes_of_the_existing_call(name, mode, hidden):
    """N = 37, 12 steps from a state max_iterations - 7 random steps into the episodes (so that episodes end inside the 12 steps and the
    metrics and episode arrays move): sgk_policy_rollout_members(n_members = 1) == sgk_policy_rollout in every output and the handle."""
    torch = _torch()
    n, steps = 37, 12
    envs = [S.BatchedGridworldEnv(name, n, seed=21, env_index_base=300) for _ in range(2)]
    try:
        dev = "cuda:%d" % envs[0].device
        w = _random_weights(torch, np.random.default_rng(hidden), 1, envs[0].n_cells, hidden, dev)
        single = {k: v[0] for k, v in w.items()}
        got = []
        for i, env in enumerate(envs):
            env.step_random(int(env.info.max_iterations) - 7, auto_reset=True)
            buf = {"states": torch.full((steps, n, env.n_cells), 77, dtype=torch.int8, device=dev),
                   "actions": torch.full((steps, n), 77, dtype=torch.uint8, device=dev),
                   "recs": torch.full((steps, n, 4), 77, dtype=torch.int8, device=dev)}
            kw = dict(mode=mode, epsilon=0.25, draw_index0=1000, auto_reset=mode == "greedy", mask_finished=mode == "sample", **buf)
            if i == 0:
                env.policy_rollout(single, steps, **kw)
            else:
                env.policy_rollout_members(w, 1, steps, **kw)
            snap = _handle_state(env)
            snap.update({k: v.cpu().numpy() for k, v in buf.items()})
            got.append(snap)
        assert got[0]["metrics"][_lib.M_EPISODES] > 0  # episodes did end inside the launch
        assert (got[0]["states"] != 77).any()
        _same_bytes(got[0], got[1], (name, mode, hidden))
    finally:
        for env in envs:
            env.close()


@pytest.mark.parametrize("hidden", [64, 100])
@pytest.mark.parametrize("name", ["BoatRace-v0", "WhiskyGold-v0"])
def test_one_member_learner_leaves_the_bytes_of_the_existing_call(name, hidden):
    """N = 37: a BatchedPPOAgent's gather + sgk_ppo_epochs against a population of ONE member with the same weights and member_keys
    NULL (the handle's seed): rollout, weights, transposed copies, Adam state, step, statistics and drawn rows bit for bit."""
    torch = _torch()
    n, args = 37, _args(hidden=hidden, batch=33, epochs=3, rollouts=37)
    e1, e2 = (S.BatchedGridworldEnv(name, n, seed=21, env_index_base=300) for _ in range(2))
    try:
        torch.manual_seed(4)
        agent = S.BatchedPPOAgent(e1, args)
        pop = S.BatchedPPOPopulation(e2, args, 1)
        pop.load_member(0, agent.net.state_dict())
        pop.member_keys = None  # NULL: the handle's seed
        rows1 = torch.zeros((3, 33), dtype=torch.int64, device=agent.device)
        rows2 = torch.zeros((1, 3, 33), dtype=torch.int64, device=agent.device)
        for it in range(2):
            r1, r2 = agent.gather_rollout(), pop.gather_rollout()
            _same_bytes(_rollout_bytes(r1), _rollout_bytes(r2), ("rollout", it))
            agent._learn_fused(r1, rows_out=rows1)
            pop.learn(r2, rows_out=rows2)
            pl = agent._pl
            a = {"rows": rows1.cpu().numpy(), "stats": agent._stats.cpu().numpy(), "step": pl["step"].cpu().numpy(),
                 "w1t": pl["w1t"].cpu().numpy(), "w2t": pl["w2t"].cpu().numpy()}
            b = {"rows": rows2[0].cpu().numpy(), "stats": pop.stats[0].cpu().numpy(), "step": pop.step.cpu().numpy(),
                 "w1t": pop.cur_t["w1t"][0].cpu().numpy(), "w2t": pop.cur_t["w2t"][0].cpu().numpy()}
            for i, k in enumerate(PP.PARAMS):
                a.update({k: agent._own_tensors()[i].cpu().numpy(), "m_" + k: pl["m"][i].cpu().numpy(), "v_" + k: pl["v"][i].cpu().numpy()})
                b.update({k: pop.cur[k][0].cpu().numpy(), "m_" + k: pop.adam_m[i][0].cpu().numpy(), "v_" + k: pop.adam_v[i][0].cpu().numpy()})
            assert int(a["step"][0]) == 3 * (it + 1) and np.abs(a["m_w1"]).max() > 0
            _same_bytes(a, b, ("learn", it))
            agent.sync(); pop.sync()
    finally:
        e1.close(); e2.close()


# ---- 2. a member is a separate run, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,members,E,batch,epochs,hidden", [
    ("WhiskyGold-v0", 3, 5, 7, 3, 64),      # the level with draws of its own per env (replaced actions), keyed by the global env index
    ("BoatRace-v0", 3, 5, 7, 3, 64),        # rows of 25 bytes: members 1 and 2 start unaligned, the last wave holds 5 rows
    ("BoatRace-v0", 2, 130, 64, 3, 100),    # two tiles per member, the second with 2 envs
])
def test_a_member_is_a_separate_run_bit_for_bit(name, members, E, batch, epochs, hidden):
    """Two PPO iterations (gather, learn, sync; the second gather under the learned weights) of a population against one BatchedPPOAgent
    per member on a handle of its own: BatchedGridworldEnv(level, E, seed, env_index_base = base + m * E), member m's weights,
    member_keys = [seed] * M (the key the agent's handle draws its rows with)."""
    torch = _torch()
    seed, base = 9, 1000
    args = _args(hidden=hidden, batch=batch, epochs=epochs, rollouts=E)
    env = S.BatchedGridworldEnv(name, members * E, seed=seed, env_index_base=base)
    singles = [S.BatchedGridworldEnv(name, E, seed=seed, env_index_base=base + m * E) for m in range(members)]
    try:
        pop = S.BatchedPPOPopulation(env, args, members, member_seeds=[31 + m for m in range(members)], member_keys=[seed] * members)
        agents = []
        for m, e in enumerate(singles):
            agent = S.BatchedPPOAgent(e, args)
            agent.net.load_state_dict(pop.member(m).state_dict())
            agent.sync()
            agents.append(agent)
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
            sums = [_lib.M_SUM_RETURN, _lib.M_SUM_SAFETY, _lib.M_SUM_MARGIN, _lib.M_SUM_MARGIN_POS, _lib.M_EPISODES, _lib.M_MARGIN_POS_COUNT]
            maxs = [_lib.M_MAX_RETURN, _lib.M_MAX_SAFETY, _lib.M_MAX_MARGIN, _lib.M_MAX_MARGIN_POS]
            assert gained[_lib.M_EPISODES] == N
            assert (per_member[:, sums].sum(0) == gained[sums]).all(), (per_member, gained)
            assert (per_member[:, maxs].max(0) == gained[maxs]).all(), (per_member, gained)
            pop.learn(ro, rows_out=used)
            for m, (e, agent) in enumerate(zip(singles, agents)):
                e.metrics_reset()
                rm = agent.gather_rollout()
                sl = slice(m * E, (m + 1) * E)
                mine = {"states": ro.states[:, sl], "actions": ro.actions[:, sl], "rewards": ro.rewards[sl], "returns": ro.returns[sl],
                        "lengths": ro.lengths[sl]}
                _same_bytes(_rollout_bytes(rm), {k: v.contiguous().cpu().numpy() for k, v in mine.items()}, ("rollout", it, m))
                alone = e.metrics()
                assert (per_member[m, sums] == alone[sums]).all() and (per_member[m, maxs] == alone[maxs]).all(), (it, m)
                agent._learn_fused(rm, rows_out=used_m)
                rows = used[m].cpu().numpy()
                t, col = rows // N, rows % N
                assert ((col >= m * E) & (col < (m + 1) * E)).all(), (it, m)  # a member draws from its own trajectories
                assert (t * E + (col - m * E) == used_m.cpu().numpy()).all(), (it, m)
                pl = agent._pl
                a = {"stats": agent._stats.cpu().numpy(), "step": pl["step"].cpu().numpy()[0]}
                b = {"stats": pop.stats[m].cpu().numpy(), "step": pop.step.cpu().numpy()[m]}
                for i, k in enumerate(PP.PARAMS):
                    a.update({k: agent._own_tensors()[i].cpu().numpy(), "m_" + k: pl["m"][i].cpu().numpy(), "v_" + k: pl["v"][i].cpu().numpy()})
                    b.update({k: pop.cur[k][m].cpu().numpy(), "m_" + k: pop.adam_m[i][m].cpu().numpy(), "v_" + k: pop.adam_v[i][m].cpu().numpy()})
                _same_bytes(a, b, ("learn", it, m))
                agent.sync()
            pop.sync()
    finally:
        env.close()
        for e in singles:
            e.close()


def test_a_workgroup_walks_all_tiles_of_its_member():
    """More members than compute units (300) with two tiles each (E = 130): every workgroup loops over its member's tiles. All members
    carry the SAME weights, so the launch must leave what the shared-policy kernel leaves with those weights."""
    torch = _torch()
    members, E, steps, hidden = 300, 130, 12, 64
    envs = [S.BatchedGridworldEnv("WhiskyGold-v0", members * E, seed=4) for _ in range(2)]
    try:
        dev, n = "cuda:%d" % envs[0].device, members * E
        single = {k: v[0].contiguous() for k, v in _random_weights(torch, np.random.default_rng(1), 1, envs[0].n_cells, hidden, dev).items()}
        stacked = {k: v.unsqueeze(0).repeat((members,) + (1,) * v.dim()).contiguous() for k, v in single.items()}
        got = []
        for i, env in enumerate(envs):
            env.step_random(int(env.info.max_iterations) - 7, auto_reset=True)
            buf = {"states": torch.full((steps, n, env.n_cells), 77, dtype=torch.int8, device=dev),
                   "actions": torch.full((steps, n), 77, dtype=torch.uint8, device=dev),
                   "recs": torch.full((steps, n, 4), 77, dtype=torch.int8, device=dev)}
            kw = dict(mode="sample", draw_index0=5, auto_reset=True, **buf)
            if i == 0:
                env.policy_rollout(single, steps, **kw)
            else:
                env.policy_rollout_members(stacked, members, steps, **kw)
            snap = _handle_state(env)
            snap.update({k: v.cpu().numpy() for k, v in buf.items()})
            got.append(snap)
        assert got[0]["metrics"][_lib.M_EPISODES] > 0
        _same_bytes(got[0], got[1], "300 members")
    finally:
        for env in envs:
            env.close()


# ---- 3. a member reproduces the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,members,index", [("batched_ppo_boat.npz", 3, 1), ("batched_ppo_boat_cheat.npz", 2, 0),
                                                ("batched_ppo_whisky_cheat_gather.npz", 3, 2)])
def test_a_member_reproduces_the_reference_ppo_run(name, members, index):
    """tests/golden/batched_ppo_*.npz (the reference's train() with PPOMLPAgent, rollout r = env index base + r) as member `index` of a
    population whose handle starts at base - index * n: the assertions of
    test_gpu_batched_golden.py::test_batched_ppo_reproduces_the_reference_ppo_run[fused] on that member's slice -- lengths, actions,
    states, rewards exact, returns bit for bit, the reference's minibatch rows (fixture row t * n + r = population row
    t * N + index * n + r), losses and weights to rtol 2e-3 / atol 2e-5, then its greedy evaluation books the fixture's episodes --
    while the other members, the fixture's initial weights plus a seeded perturbation, run beside it."""
    from oracle import oracle as O

    torch = _torch()
    fx = BG.PpoFixture(name)
    meta, T, n = fx.meta, fx.horizon, fx.n
    N = members * n
    assert fx.base - index * n >= 0
    env = S.BatchedGridworldEnv(fx.env, N, seed=fx.seed, env_index_base=fx.base - index * n)
    try:
        args = fx.args(0)
        args.seed = fx.seed
        keys = [fx.seed if m == index else fx.seed + 1000 + m for m in range(members)]
        pop = S.BatchedPPOPopulation(env, args, members, member_keys=keys)
        rng = np.random.default_rng(17)
        for m in range(members):
            sd = {k: torch.as_tensor(v if m == index else (v + 0.02 * rng.standard_normal(v.shape)).astype(np.float32))
                  for k, v in fx.weights(0).items() if not k.startswith("old_policy.")}
            pop.load_member(m, sd)
        pop.sync()
        sl = slice(index * n, (index + 1) * n)
        used = torch.zeros((members, meta["epochs"], meta["batch_size"]), dtype=torch.int64, device=pop.device)
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
                pop.learn(ro, rows_out=used)
                ref = fx.it(k, "rows")
                assert (used[index].cpu().numpy() == (ref // n) * N + index * n + ref % n).all(), k
                stats = pop.stats.cpu().numpy().astype(np.float64)
                np.testing.assert_allclose(stats[index], fx.losses(k), rtol=2e-3, atol=2e-5)
                sd = PP.unstack_state_dict(pop.cur, index)
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


# ---- 4. float64 ---------------------------------------------------------------------------------------------------------------------
FLOAT64_CASES = [next(c for c in R.PPO_CASES if c[:3] == ("SideEffectsSokoban-v0", 100, 64)),
                 next(c for c in R.PPO_CASES if c[:3] == ("BoatRace-v0", 100, 33))]


def run_members_case(case, members=3, index=1):
    """tests/test_gpu_learner_gradients.py::run_ppo_case for member `index` of a population: the case's rollout, weights and rows in that
    member's slice of every tensor, seeded other data in the neighbours'. Returns (that member's results in run_ppo_case's form, the
    neighbours' first moments after step A)."""
    torch = _torch()
    d = R.ppo_yardstick(case)[0]
    n, N = R.N_ENVS, members * R.N_ENVS
    env = S.BatchedGridworldEnv(case.env, N, seed=3)
    try:
        assert env.n_cells == R.ENV_CELLS[case.env]
        args = _args(hidden=case.hidden, batch=case.batch, epochs=1, rollouts=n, **R.PPO_HYPER)
        pop = S.BatchedPPOPopulation(env, args, members)
        dev, rng = pop.device, np.random.default_rng(case.seed + 77)
        noise = lambda a: (a + np.float32(0.05) * rng.standard_normal(a.shape).astype(np.float32)).astype(np.float32)  # noqa: E731
        cur = [d["cur"] if m == index else [noise(a) for a in d["cur"]] for m in range(members)]
        old = [d["old"] if m == index else [noise(a) for a in d["old"]] for m in range(members)]

        def load():
            for m in range(members):
                sd = {k: torch.as_tensor(a) for k, a in zip(PP.MEMBER_KEYS, cur[m])}
                sd.update({"old_policy." + k: torch.as_tensor(a) for k, a in zip(PP.MEMBER_KEYS, old[m])})
                pop.load_member(m, sd)

        def column_block(own, shape, make, axis):
            parts = [own if m == index else make(shape) for m in range(members)]
            return torch.as_tensor(np.ascontiguousarray(np.concatenate(parts, axis=axis))).to(dev)

        ro = types.SimpleNamespace(
            states=column_block(d["states"], d["states"].shape, lambda s: rng.integers(0, 6, s).astype(np.int8), 1),
            actions=column_block(d["actions"], d["actions"].shape, lambda s: rng.integers(0, 4, s).astype(np.uint8), 1),
            returns=column_block(d["returns"], d["returns"].shape, lambda s: rng.uniform(-5.0, 5.0, s).astype(np.float32), 0),
            lengths=torch.full((N,), R.SLICES, dtype=torch.int32, device=dev))
        t, col = d["rows"] // n, d["rows"] % n
        rows = torch.as_tensor(np.stack([t * N + m * n + col for m in range(members)])[:, None, :].astype(np.int64)).to(dev)
        cpu = lambda ts: [x[index].detach().cpu().numpy().copy() for x in ts]  # noqa: E731
        own = [pop.cur[k] for k in PP.PARAMS]
        out = {}
        load()
        pop.learn(ro, rows=rows)
        out["stats"] = [pop.stats[index, 0].cpu().numpy().copy()]
        out["m_a"], out["v_a"], out["w_a"] = cpu(pop.adam_m), cpu(pop.adam_v), cpu(own)
        out["step_a"] = [pop.step[index:index + 1].cpu().numpy().copy()]
        others = {m: [x[m].cpu().numpy().copy() for x in pop.adam_m] for m in range(members) if m != index}
        g_c = [m.astype(np.float64) / R.one_minus_beta1() for m in out["m_a"]]
        ms, vs, _ = R.inject_adam_state(g_c, LC.STATE_SEED + case.seed, False)
        load()
        with torch.no_grad():
            for i in range(8):
                pop.adam_m[i][index].copy_(torch.as_tensor(np.ascontiguousarray(ms[i])).to(dev))
                pop.adam_v[i][index].copy_(torch.as_tensor(np.ascontiguousarray(vs[i])).to(dev))
        pop.step.fill_(LC.STEP_BEFORE_B)
        pop.learn(ro, rows=rows)
        out["m_b"], out["v_b"], out["w_b"] = cpu(pop.adam_m), cpu(pop.adam_v), cpu(own)
        out["step_b"] = [pop.step[index:index + 1].cpu().numpy().copy()]
        out["w1t"], out["w2t"] = cpu([pop.cur_t["w1t"]]), cpu([pop.cur_t["w2t"]])
        torch.cuda.synchronize()
        return out, others
    finally:
        env.close()


def members_result(case):
    return G._once(("ppo members", case), lambda: run_members_case(case))


@pytest.mark.parametrize("case", FLOAT64_CASES, ids=R.case_id)
def test_a_member_meets_the_float64_bounds_of_the_single_learner(case):
    """Member 1 of 3 on a learner_reference case: step A's gradients (out of Adam's first moment), second moments and the three
    statistics, and step B's Adam from the injected state at step 4999, within learner_reference's own bounds exactly as
    test_ppo_learner_gradients_and_statistics_against_float64 / test_ppo_learner_adam_from_injected_state check the single learner;
    the neighbours, on other weights and other data, end somewhere else (a member stride that trained everybody on member 0's slice
    fails the first, one that gave everybody the same slice fails the second)."""
    out, others = members_result(case)
    G._finite(out, ("m_a", "v_a", "w_a", "stats", "m_b", "v_b", "w_b"))
    assert int(out["step_a"][0][0]) == 1
    G._check(G.ppo_figures_a(case, out))
    assert int(out["step_b"][0][0]) == LC.STEP_BEFORE_B + 1
    G._check(G.ppo_figures_b(case, out))
    assert (out["w1t"][0] == out["w_b"][0].T).all() and (out["w2t"][0] == out["w_b"][2].T).all()
    for m, ms in others.items():
        for k, a, b in zip(PP.PARAMS, ms, out["m_a"]):
            assert np.isfinite(a).all() and not np.array_equal(a, b), (m, k)
    assert not np.array_equal(others[0][0], others[2][0])


# ---- 5. capture ---------------------------------------------------------------------------------------------------------------------
def test_learn_replayed_from_a_graph_equals_the_eager_call():
    """pop.learn recorded once under torch.cuda.graph (one stream, no parallel branches) after a warm-up call, replayed twice from the
    same inputs: every output of each replay is bit-identical to the eager call's."""
    torch = _torch()
    members, E = 3, 5
    env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=6)
    try:
        pop = S.BatchedPPOPopulation(env, _args(hidden=64, batch=7, epochs=3, rollouts=E), members)
        ro = pop.gather_rollout()
        used = torch.zeros((members, 3, 7), dtype=torch.int64, device=pop.device)
        start = {k: t.clone() for k, t in pop.tensors().items()}

        def restore():
            for k, t in pop.tensors().items():
                t.copy_(start[k])
            used.zero_(); pop.stats.zero_()

        def outputs():
            out = {k: t.cpu().numpy() for k, t in pop.tensors().items()}
            out.update(rows=used.cpu().numpy(), stats=pop.stats.cpu().numpy())
            return out

        pop.learn(ro, rows_out=used)  # eager (also the warm-up: the kernel's attributes are set)
        eager = outputs()
        assert (eager["step"] == 3).all() and np.abs(eager["m_w1"]).max() > 0 and eager["rows"].any()
        restore()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            pop.learn(ro, rows_out=used)
        for replay in range(2):
            restore()
            graph.replay()
            torch.cuda.synchronize()
            _same_bytes(eager, outputs(), ("replay", replay))
    finally:
        env.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_what_cannot_run_is_refused_with_the_reason():
    """n_envs % n_members != 0 (the C entry points and the Python layer), 128 hidden units with learn, a batch of 65, three layers: an
    SgkError / ValueError that says why, and nothing launched (weights, step counters, metrics and the env untouched)."""
    torch = _torch()
    env = S.BatchedGridworldEnv("BoatRace-v0", 15, seed=6)
    try:
        pop = S.BatchedPPOPopulation(env, _args(hidden=64, batch=7, epochs=2, rollouts=5), 3)
        ro = pop.gather_rollout()
        before = {k: t.clone() for k, t in pop.tensors().items()}
        handle = _handle_state(env)
        lib, dev = env.lib, pop.device
        w = env._member_weights_arg(pop._old_weights(), 3)
        for bad in (2, 4, 0, -1):
            rc = lib.sgk_policy_rollout_members(env._h.ptr, ctypes.byref(w), bad, 1, 0.0, 0, 5, 0, None, None, None, None)
            assert rc == _lib.ERR_INVALID and b"n_members" in lib.sgk_last_error(), (bad, lib.sgk_last_error())
            with pytest.raises((_lib.SgkError, ValueError), match="n_members"):
                env.policy_rollout_members(pop._old_weights(), bad, 5)
            with pytest.raises(ValueError, match="n_members"):
                S.BatchedPPOPopulation(env, _args(hidden=64, batch=7, epochs=2, rollouts=5), bad)
        # the learner: a filled sgk_ppo_learner the library would accept, then one thing wrong at a time
        H, K0 = 64, env.n_cells
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        keep = {"w1": f(4, H, K0), "b1": f(4, H), "w2": f(4, H, H), "b2": f(4, H), "wa": f(4, 4, H), "ba": f(4, 4), "wc": f(4, 1, H),
                "bc": f(4, 1), "w1t": f(4, K0, H), "w2t": f(4, H, H), "ow1t": f(4, K0, H), "ob1": f(4, H), "ow2t": f(4, H, H), "ob2": f(4, H),
                "owa": f(4, 4, H), "oba": f(4, 4)}
        step = torch.zeros(4, dtype=torch.int64, device=dev)

        def learner(hidden=64, batch=7):
            L = _lib.SgkPpoLearner()
            L.states, L.actions, L.returns, L.lengths = (ro.states.data_ptr(), ro.actions.data_ptr(), ro.returns.data_ptr(), ro.lengths.data_ptr())
            L.horizon, L.n_hidden, L.batch, L.n_epochs, L.n_trajectories = ro.actions.shape[0], hidden, batch, 2, 15
            for k, t in keep.items():
                setattr(L, k, t.data_ptr())
            for i, k in enumerate(PP.PARAMS):
                L.m[i], L.v[i] = keep[k].data_ptr(), keep[k].data_ptr()
            L.step = step.data_ptr()
            L.lr, L.beta1, L.beta2, L.eps, L.clipping, L.critic_coeff, L.entropy_bonus = 1e-3, 0.9, 0.999, 1e-8, 0.2, 1.0, 0.01
            return L

        for L, members, reason in ((learner(), 2, b"n_members"), (learner(), 4, b"n_members"), (learner(), 0, b"n_members"),
                                   (learner(hidden=128), 3, b"n_hidden"), (learner(batch=65), 3, b"batch")):
            rc = lib.sgk_ppo_epochs_members(env._h.ptr, ctypes.byref(L), members, None)
            assert rc == _lib.ERR_INVALID and reason in lib.sgk_last_error(), (members, lib.sgk_last_error())
        for kw, reason in ((dict(hidden=128), "n_hidden"), (dict(batch=65), "batch_size"), (dict(layers=3), "n_layers"), (dict(batch=1), "batch_size")):
            with pytest.raises(ValueError, match=reason):
                S.BatchedPPOPopulation(env, _args(**dict(dict(hidden=64, batch=7, epochs=2, rollouts=5), **kw)), 3)
        with pytest.raises(ValueError, match="rows"):  # a tensor argument of the wrong shape never reaches the kernel
            pop.learn(ro, rows=torch.zeros((3, 2, 6), dtype=torch.int64, device=dev))
        with pytest.raises(ValueError, match="rollout.states"):
            pop.learn(ro._replace(states=ro.states.to(torch.float32)))
        torch.cuda.synchronize()
        assert int(step.abs().sum()) == 0 and all(int((t != 0).sum()) == 0 for t in keep.values())
        for k, t in pop.tensors().items():
            assert torch.equal(t, before[k]), k
        _same_bytes(handle, _handle_state(env), "after the refusals")
    finally:
        env.close()
