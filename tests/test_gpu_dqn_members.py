"""A population of independent Deep-Q agents -- sgk_dqn_sgd_step_members (dqn_sgd_kernel / dqn_adam_kernel with a member axis),
BatchedDeepQPopulation -- on the GPU:

1. one member IS the existing call: n_members = 1, keys NULL and a workspace leave the bytes sgk_dqn_sgd_step leaves;
2. a member is a separate run, bit for bit: member m of a population == a BatchedDeepQAgent on a handle of E envs created at
   env_index_base + m * E with member m's weights, step by step through a warm-up and 12 learning steps across a target sync;
3. more members than compute units (300): every member, given the same weights and the same transitions, ends where the single call ends;
4. a caller's row outside a member's own columns trains on the member's first transition;
5. a member's gradients and Adam meet tests/learner_reference.py's float64 bounds, as tests/test_gpu_learner_gradients.py applies them to
   the single learner (its helpers, imported), and the neighbours' results differ;
6. a member reproduces the REFERENCE's own run (tests/golden/batched_dqn_*.npz) while its neighbours run something else;
7. learn_batch recorded in a graph as the first learner call on its handle == the eager calls; 8. what cannot run is refused with the
   reason.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import ctypes
import functools
import types

import numpy as np
import pytest

import batched_golden as BG
import learner_child as LC
import learner_reference as R
import safe_grid_agents_amd as S
import test_gpu_learner_gradients as G
from safe_grid_agents_amd import _lib
from safe_grid_agents_amd import deepq_population as DP
from test_gpu_batched_golden import DQN_ATOL, DQN_LOSS_RTOL, DQN_RTOL
from test_gpu_ppo_members import _handle_state, _same_bytes

pytestmark = pytest.mark.gpu

RING = ("states", "successors", "actions", "rewards", "terminals")


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _args(hidden=100, batch=64, sync_every=20, layers=2, seed=5, lr=R.DQN_LR, discount=R.DQN_DISCOUNT):
    return types.SimpleNamespace(discount=discount, lr=lr, batch_size=batch, sync_every=sync_every, epsilon=0.05, epsilon_anneal=200,
                                 n_layers=layers, n_hidden=hidden, seed=seed)


def _sd(torch, arrays):
    return {k: torch.as_tensor(np.ascontiguousarray(a)) for k, a in zip(DP.MEMBER_KEYS, arrays)}


def _load_agent(torch, agent, q_state, t_state):
    """A BatchedDeepQAgent's two networks <- state dicts, the fused kernels' transposed copies refreshed."""
    dev = agent.device
    agent.Q.load_state_dict({k: torch.as_tensor(v).to(dev) for k, v in q_state.items()})
    agent.target_Q.load_state_dict({k: torch.as_tensor(v).to(dev) for k, v in t_state.items()})
    agent._refresh_fused_weights()
    agent._fl["w2t"].copy_(agent.Q[1][0][0].weight.data.t())
    agent._refresh_target_transposes()


def _fill_ring(torch, rp, d, filled):
    for key in RING:
        getattr(rp, key).copy_(torch.as_tensor(np.ascontiguousarray(d[key])).to(rp.device))
    rp.filled = filled


def _agent_learner(agent):
    """Everything sgk_dqn_sgd_step reads and updates of a BatchedDeepQAgent, under the population's tensor names."""
    fl, fw = agent._fl, agent._fw
    out = {"w1t": fw["w1t"], "w2t": fl["w2t"], "w3t": fw["w3t"], "step": fl["step"][0], "loss": fl["loss"][0],
           "target_w1t": fl["tw1t"], "target_w2t": fl["tw2t"]}
    for i, (k, p, tp) in enumerate(zip(DP.PARAMS, agent.Q.parameters(), agent.target_Q.parameters())):
        out.update({k: p.data, "m_" + k: fl["m"][i], "v_" + k: fl["v"][i], "vmax_" + k: fl["vmax"][i], "target_" + k: tp.data})
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def _member_learner(pop, m):
    return {k: v[m].detach().cpu().numpy() for k, v in pop.tensors().items()}


def _case(env, hidden, batch):
    return next(c for c in R.DQN_CASES if c[:3] == (env, hidden, batch) and c.clipped and c.broadcast)


# ---- 1. one member is the existing call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [64, 100])
@pytest.mark.parametrize("name", ["BoatRace-v0", "DistributionalShift-v0"])
def test_one_member_leaves_the_bytes_of_the_existing_call(name, hidden):
    """learner_reference.dqn_inputs' synthetic ring (2 slices x 64 envs; BoatRace: rows of 25 bytes, every second one unaligned; the
    63-cell level) on two handles: sgk_dqn_sgd_step against sgk_dqn_sgd_step_members(n_members = 1, keys NULL, a workspace) -- two steps
    on the kernel's own draws and one on the caller's rows: weights, transposes, m / v / vmax, step, loss and rows_out as bytes."""
    torch = _torch()
    case = _case(name, hidden, 64)
    d = R.dqn_inputs(case)
    e1, e2 = (S.BatchedGridworldEnv(name, R.N_ENVS, seed=21, env_index_base=300) for _ in range(2))
    try:
        args = _args(hidden=hidden, batch=case.batch)
        agent = S.BatchedDeepQAgent(e1, args, replay_slices=R.SLICES)
        pop = S.BatchedDeepQPopulation(e2, args, 1, replay_slices=R.SLICES)
        assert agent.fused_learn
        _load_agent(torch, agent, _sd(torch, d["q"]), _sd(torch, d["t"]))
        pop.load_member(0, _sd(torch, d["q"]), _sd(torch, d["t"]))
        pop.member_keys = None  # NULL: the handle's seed
        _fill_ring(torch, agent.replay, d, R.SLICES)
        _fill_ring(torch, pop.replay, d, R.SLICES)
        dev = agent.device
        used1 = torch.zeros(case.batch, dtype=torch.int64, device=dev)
        used2 = torch.zeros((1, case.batch), dtype=torch.int64, device=dev)
        rows = torch.as_tensor(d["rows"]).to(dev)
        drawn = []
        for it in range(3):
            r = rows if it == 2 else None
            agent._learn_batch_fused(rows=r, rows_out=used1)
            pop.learn_batch(rows=None if r is None else r[None].contiguous(), rows_out=used2)
            a, b = _agent_learner(agent), _member_learner(pop, 0)
            a["rows"], b["rows"] = used1.cpu().numpy(), used2[0].cpu().numpy()
            assert int(a["step"]) == it + 1 and np.abs(a["m_w1"]).max() > 0 and np.isfinite(a["loss"])
            _same_bytes(a, b, (name, hidden, it))
            drawn.append(a["rows"].copy())
        assert not np.array_equal(drawn[0], drawn[1]) and np.array_equal(drawn[2], d["rows"])
        assert ((drawn[0] >= 0) & (drawn[0] < R.SLICES * R.N_ENVS)).all() and len(set(drawn[0].tolist())) > 8
    finally:
        e1.close(); e2.close()


# ---- 2. a member is a separate run, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,members,E,batch,hidden", [
    ("WhiskyGold-v0", 3, 5, 7, 64),      # the level with draws of its own per env (replaced actions), keyed by the global env index
    ("BoatRace-v0", 3, 5, 7, 64),        # rows of 25 bytes: members 1 and 2 start unaligned
    ("BoatRace-v0", 2, 130, 64, 100),    # two acting tiles per member
])
def test_a_member_is_a_separate_run_bit_for_bit(name, members, E, batch, hidden):
    """A warm-up of the whole ring, then 12 lockstep learning steps (sync_every = 8: one target sync inside) of a population against one
    BatchedDeepQAgent(sgd_steps=1, fused_learn=True, fuse_reset=False) per member on a handle of its own: BatchedGridworldEnv(level, E,
    seed, env_index_base = base + m * E), member m's Q and target weights, member_keys = [seed] * M (the key the agent's handle draws its
    minibatch with). After every step: actions, the handle's state, the ring columns, the minibatch rows, the loss and every learner
    tensor as bytes."""
    torch = _torch()
    seed, base, slices, steps = 9, 1000, 4, 12
    args = _args(hidden=hidden, batch=batch, sync_every=8, lr=1e-3)
    N = members * E
    env = S.BatchedGridworldEnv(name, N, seed=seed, env_index_base=base)
    singles = [S.BatchedGridworldEnv(name, E, seed=seed, env_index_base=base + m * E) for m in range(members)]
    try:
        pop = S.BatchedDeepQPopulation(env, args, members, member_seeds=[31 + m for m in range(members)], member_keys=[seed] * members,
                                       replay_slices=slices)
        dev = pop.device
        used = torch.zeros((members, batch), dtype=torch.int64, device=dev)
        used_m = torch.zeros(batch, dtype=torch.int64, device=dev)
        pop.learn_batch = functools.partial(pop.learn_batch, rows_out=used)  # (step() calls self.learn_batch())
        agents = []
        for m, e in enumerate(singles):
            agent = S.BatchedDeepQAgent(e, args, sgd_steps=1, replay_slices=slices, fused_learn=True)
            assert agent.fused_learn
            agent.fuse_reset = False
            st = pop.member_state(m)
            _load_agent(torch, agent, st["Q"], st["target_Q"])
            agent.learn_batch = functools.partial(agent._learn_batch_fused, rows_out=used_m)
            agents.append(agent)
        assert not torch.equal(pop.cur["w2"][0], pop.cur["w2"][1])  # the members did start from different weights
        assert not torch.equal(pop.target["w2"][0], pop.cur["w2"][0])  # Q and the target are initialised independently

        def compare(what):
            state = _handle_state(env)
            ring = {k: getattr(pop.replay, k).cpu().numpy() for k in RING}
            for m, (e, agent) in enumerate(zip(singles, agents)):
                sl = slice(m * E, (m + 1) * E)
                mine = {k: v[sl] for k, v in state.items() if k != "metrics"}
                alone = {k: v for k, v in _handle_state(e).items() if k != "metrics"}
                _same_bytes(mine, alone, (what, "handle", m))
                _same_bytes({k: np.ascontiguousarray(v[:, sl]) for k, v in ring.items()},
                            {k: getattr(agent.replay, k).cpu().numpy() for k in RING}, (what, "ring", m))
                assert (pop.replay.head, pop.replay.filled) == (agent.replay.head, agent.replay.filled)
                _same_bytes(_member_learner(pop, m), _agent_learner(agent), (what, "learner", m))

        pop.warmup(slices)
        for agent in agents:
            agent.warmup(slices)
        for e in [env] + singles:
            e.reset()
            e.metrics_reset()
        pop.reset_member_metrics()
        compare("warm-up")
        losses = []
        for t in range(steps):
            a = pop.step(learn=True).cpu().numpy()
            rows = used.cpu().numpy()
            for m, agent in enumerate(agents):
                am = agent.step(learn=True).cpu().numpy()
                assert a[m * E:(m + 1) * E].tobytes() == am.tobytes(), (t, m)
                sl_, col = rows[m] // N, rows[m] % N
                assert ((col >= m * E) & (col < (m + 1) * E)).all(), (t, m)  # a member draws from its own columns
                assert (sl_ * E + (col - m * E) == used_m.cpu().numpy()).all(), (t, m)
                assert agent.t == pop.t and agent.epsilon == pop.epsilon
            compare("step %d" % t)
            losses.append(pop.loss.cpu().numpy().copy())
        assert int(pop.step_count[0]) == steps
        assert torch.equal(pop.target["w2"], pop.cur["w2"]) is False and pop.t == steps  # (four steps past the sync at t = 7)
        assert len({float(x) for x in losses[-1]}) == members  # the members ended with different losses
        sums = [_lib.M_SUM_RETURN, _lib.M_SUM_SAFETY, _lib.M_EPISODES]
        per_member = pop.member_metrics.cpu().numpy()
        for m, e in enumerate(singles):
            assert (per_member[m, sums] == e.metrics()[sums]).all(), m
    finally:
        env.close()
        for e in singles:
            e.close()


# ---- 3. more members than compute units ---------------------------------------------------------------------------------------------
def test_more_members_than_compute_units_each_end_where_the_single_call_ends():
    """M = 300, E = 1, 64 units on BoatRace: every member gets the same weights and Adam state, every column of the ring the same 8
    transitions, and member m's rows name its own column -- one launch (the grid mapping, not a stress run) must leave every member's
    tensors equal to member 0's and to what sgk_dqn_sgd_step leaves on a handle of one env."""
    torch = _torch()
    members, slices, batch, hidden = 300, 8, 17, 64
    case = _case("BoatRace-v0", hidden, 64)
    d = R.dqn_inputs(case)
    column = {k: d[k][0, :slices] for k in RING}  # 8 transitions
    picks = np.random.default_rng(3).integers(0, slices, batch)
    env = S.BatchedGridworldEnv("BoatRace-v0", members, seed=4)
    one = S.BatchedGridworldEnv("BoatRace-v0", 1, seed=4)
    try:
        args = _args(hidden=hidden, batch=batch)
        pop = S.BatchedDeepQPopulation(env, args, members, replay_slices=slices)
        agent = S.BatchedDeepQAgent(one, args, replay_slices=slices)
        dev = pop.device
        _load_agent(torch, agent, _sd(torch, d["q"]), _sd(torch, d["t"]))
        rng = np.random.default_rng(8)
        state = [[np.abs(rng.normal(0, 1e-3, p.shape)).astype(np.float32) for p in d["q"]] for _ in range(2)]
        for i in range(6):
            agent._fl["m"][i].copy_(torch.as_tensor(state[0][i]).to(dev))
            for dst in (agent._fl["v"][i], agent._fl["vmax"][i]):
                dst.copy_(torch.as_tensor(state[1][i]).to(dev))
            pop.adam_m[i].copy_(torch.as_tensor(state[0][i]).to(dev).expand_as(pop.adam_m[i]))
            for dst in (pop.adam_v[i], pop.adam_vmax[i]):
                dst.copy_(torch.as_tensor(state[1][i]).to(dev).expand_as(dst))
        agent._fl["step"].fill_(41)
        pop.step_count.fill_(41)
        for m in range(members):
            pop.load_member(m, _sd(torch, d["q"]), _sd(torch, d["t"]))
        _fill_ring(torch, agent.replay, {k: v[:, None] for k, v in column.items()}, slices)
        _fill_ring(torch, pop.replay, {k: np.repeat(v[:, None], members, axis=1) for k, v in column.items()}, slices)
        rows = torch.as_tensor(picks[None, :] * members + np.arange(members)[:, None]).to(dev)
        used = torch.zeros((members, batch), dtype=torch.int64, device=dev)
        agent._learn_batch_fused(rows=torch.as_tensor(picks).to(dev))
        pop.learn_batch(rows=rows, rows_out=used)
        torch.cuda.synchronize()
        assert torch.equal(used, rows)
        want = _agent_learner(agent)
        assert int(want["step"]) == 42 and np.isfinite(want["loss"]) and not np.array_equal(want["w2"], d["q"][2])
        for k, t in pop.tensors().items():
            t = t.cpu().numpy()
            assert (t == t[:1]).all(), k  # every member equals member 0
            assert t[0].tobytes() == want[k].tobytes(), k
    finally:
        env.close(); one.close()


# ---- 4. a caller's rows outside a member's columns ----------------------------------------------------------------------------------
def test_a_callers_row_outside_a_members_columns_trains_on_its_first_transition():
    """M = 3, E = 5, a warmed-up ring of 4 slices: rows past the stored transitions, negative ones and rows naming another member's env
    (in range for the ring) leave what a call leaves whose rows name the member's first transition (slice 0, env m * E) in their place;
    rows_out reports that transition."""
    torch = _torch()
    members, E, slices, batch = 3, 5, 4, 7
    N = members * E
    env = S.BatchedGridworldEnv("BoatRace-v0", N, seed=6)
    try:
        pop = S.BatchedDeepQPopulation(env, _args(hidden=64, batch=batch), members, replay_slices=slices)
        pop.warmup(slices)
        dev = pop.device
        own = lambda m, sl, e: sl * N + m * E + e  # noqa: E731
        good = np.array([[own(m, (m + b) % slices, (2 * b + m) % E) for b in range(batch)] for m in range(members)], dtype=np.int64)
        bad = good.copy()
        bad[0, 1] = slices * N + 3              # past the stored transitions
        bad[0, 4] = -2
        bad[1, 0] = own(0, 1, 2)                # member 0's env
        bad[1, 5] = own(2, 3, 4)                # member 2's env
        bad[1, 6] = 2 ** 40
        bad[2, 3] = own(1, 0, 0)                # the env just below its own
        first = good.copy()
        for m, b in ((0, 1), (0, 4), (1, 0), (1, 5), (1, 6), (2, 3)):
            first[m, b] = m * E
        start = {k: t.clone() for k, t in pop.tensors().items()}
        got = []
        for rows in (bad, first):
            for k, t in pop.tensors().items():
                t.copy_(start[k])
            used = torch.full((members, batch), -1, dtype=torch.int64, device=dev)
            pop.learn_batch(rows=torch.as_tensor(rows).to(dev), rows_out=used)
            out = {k: t.cpu().numpy() for k, t in pop.tensors().items()}
            out["rows"] = used.cpu().numpy()
            got.append(out)
        assert (got[0]["rows"] == first).all() and (got[0]["step"] == 1).all()
        _same_bytes(got[0], got[1], "rows outside")
    finally:
        env.close()


# ---- 5. float64 ---------------------------------------------------------------------------------------------------------------------
def run_members_case(case, members=3, index=1):
    """tests/learner_child.py::run_dqn_case for member `index` of a population: the case's ring, weights and rows in that member's
    columns / slice, seeded other data in the neighbours'. Returns (that member's results in run_dqn_case's form, the neighbours' first
    moments after step A)."""
    torch = _torch()
    d = R.dqn_inputs(case)
    n, N = R.N_ENVS, members * R.N_ENVS
    env = S.BatchedGridworldEnv(case.env, N, seed=3)
    try:
        assert env.n_cells == R.ENV_CELLS[case.env] and float(env.reward_scale) == d["reward_scale"]
        pop = S.BatchedDeepQPopulation(env, _args(hidden=case.hidden, batch=case.batch), members, replay_slices=R.SLICES,
                                       reference_loss_broadcast=case.broadcast)
        dev, rng = pop.device, np.random.default_rng(case.seed + 77)
        noise = lambda a: (a + np.float32(0.05) * rng.standard_normal(a.shape).astype(np.float32)).astype(np.float32)  # noqa: E731
        q = [d["q"] if m == index else [noise(a) for a in d["q"]] for m in range(members)]
        t = [d["t"] if m == index else [noise(a) for a in d["t"]] for m in range(members)]
        make = {"states": lambda s: rng.integers(0, 6, s).astype(np.int8), "successors": lambda s: rng.integers(0, 6, s).astype(np.int8),
                "actions": lambda s: rng.integers(0, 4, s).astype(np.uint8), "rewards": lambda s: rng.integers(-50, 51, s).astype(np.int8),
                "terminals": lambda s: rng.random(s) < 0.3}
        ring = {k: np.concatenate([d[k] if m == index else make[k](d[k].shape) for m in range(members)], axis=1) for k in RING}
        _fill_ring(torch, pop.replay, ring, R.SLICES)
        sl, col = d["rows"] // n, d["rows"] % n
        rows = torch.as_tensor(np.stack([sl * N + m * n + col for m in range(members)]).astype(np.int64)).to(dev)
        used = torch.zeros((members, case.batch), dtype=torch.int64, device=dev)
        own = [pop.cur[k] for k in DP.PARAMS]
        cpu = lambda ts: [x[index].detach().cpu().numpy().copy() for x in ts]  # noqa: E731

        def set_state(ms, vs, xs, step):
            for m in range(members):
                pop.load_member(m, _sd(torch, q[m]), _sd(torch, t[m]))
            for i in range(6):
                for dst, src in ((pop.adam_m[i], ms[i]), (pop.adam_v[i], vs[i]), (pop.adam_vmax[i], xs[i])):
                    dst.zero_()
                    dst[index].copy_(torch.as_tensor(np.ascontiguousarray(src)).to(dev))
            pop.step_count.fill_(step)

        zeros = [np.zeros_like(p) for p in d["q"]]
        out = {}
        set_state(zeros, zeros, zeros, 0)
        pop.learn_batch(rows=rows, rows_out=used)
        assert torch.equal(used, rows)
        out["loss"] = [pop.loss[index:index + 1].cpu().numpy().copy()]
        out["m_a"], out["v_a"], out["x_a"], out["w_a"] = cpu(pop.adam_m), cpu(pop.adam_v), cpu(pop.adam_vmax), cpu(own)
        out["step_a"] = [pop.step_count[index:index + 1].cpu().numpy().copy()]
        others = {m: [x[m].cpu().numpy().copy() for x in pop.adam_m] for m in range(members) if m != index}
        g_c = [m.astype(np.float64) / R.one_minus_beta1() for m in out["m_a"]]
        set_state(*R.inject_adam_state(g_c, LC.STATE_SEED + case.seed, True), LC.STEP_BEFORE_B)
        pop.learn_batch(rows=rows)
        out["m_b"], out["v_b"], out["x_b"], out["w_b"] = cpu(pop.adam_m), cpu(pop.adam_v), cpu(pop.adam_vmax), cpu(own)
        out["step_b"] = [pop.step_count[index:index + 1].cpu().numpy().copy()]
        out["w1t"], out["w2t"], out["w3t"] = cpu([pop.cur_t["w1t"]]), cpu([pop.cur_t["w2t"]]), cpu([pop.cur_t["w3t"]])
        torch.cuda.synchronize()
        return out, others
    finally:
        env.close()


@pytest.mark.parametrize("case", R.CHILD_CASES, ids=R.case_id)
def test_a_member_meets_the_float64_bounds_of_the_single_learner(case):
    """Member 1 of 3 on learner_reference's CHILD_KEYS cases (clipped, broadcast): step A's gradients (out of Adam's first moment), second
    moments and loss, and step B's Adam(amsgrad) from the injected state at step 4999, within learner_reference's own bounds exactly as
    test_dqn_learner_gradients_and_loss_against_float64 / test_dqn_learner_adam_amsgrad_from_injected_state check the single learner
    (dqn_checks_a / dqn_checks_b, imported: no tolerance of this file's); the neighbours, on other weights and other data, end
    somewhere else."""
    out, others = G._once(("dqn members", case), lambda: run_members_case(case))
    G.dqn_checks_a(case, out)
    G.dqn_checks_b(case, out)
    for m, ms in others.items():
        for k, a, b in zip(DP.PARAMS, ms, out["m_a"]):
            assert np.isfinite(a).all() and not np.array_equal(a, b), (m, k)
    assert not np.array_equal(others[0][0], others[2][0])


# ---- 6. a member reproduces the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["batched_dqn_sokoban.npz", "batched_dqn_boat_cheat.npz"])
def test_a_member_reproduces_the_reference_dqn_run(name):
    """tests/golden/batched_dqn_*.npz (the reference's train() with DeepQAgent + dqn_warmup + dqn_learn on env index fx.index) as one
    member of a population of M = 3, E = 1 whose handle starts at fx.index - index: the assertions of
    test_gpu_batched_golden.py::test_batched_deepq_n1_reproduces_the_reference_dqn_run on that member -- the warm-up ring exact, every
    action exact, losses and the weights at the three syncs and at the end within that file's DQN_RTOL / DQN_ATOL / DQN_LOSS_RTOL, then
    its greedy evaluation books the fixture's episodes -- while the other members, the fixture's initial weights plus a seeded 0.02
    perturbation and keys of their own, run beside it and see other losses."""
    from oracle import oracle as O

    torch = _torch()
    fx = BG.DqnFixture(name)
    members = 3
    index = 1 if fx.index >= 1 else 0
    env = S.BatchedGridworldEnv(fx.env, members, seed=fx.seed, env_index_base=fx.index - index)
    try:
        keys = [fx.seed if m == index else fx.seed + 1000 + m for m in range(members)]
        pop = S.BatchedDeepQPopulation(env, fx.args(), members, member_keys=keys, replay_slices=fx.capacity)
        assert pop.reference_loss_broadcast and pop.sgd_steps == 1
        rng = np.random.default_rng(17)
        for m in range(members):
            sds = [{k: torch.as_tensor(v if m == index else (v + 0.02 * rng.standard_normal(v.shape)).astype(np.float32))
                    for k, v in fx.weights(tag).items()} for tag in ("init_Q", "init_T")]
            pop.load_member(m, *sds)
        reset_board = env.boards_host()[index].reshape(-1).copy()
        # ---- dqn_warmup ----
        pop.warmup(fx.capacity)
        rp = pop.replay
        assert rp.filled == fx.capacity and rp.head == 0
        term = fx.warm("terminals") != 0
        assert (rp.states[:, index].cpu().numpy() == fx.warm("states")).all()
        want_succ = np.where(term[:, None], reset_board[None], fx.warm("successors"))  # (the ring's convention at an episode's last step)
        assert (rp.successors[:, index].cpu().numpy() == want_succ).all()
        assert (rp.actions[:, index].cpu().numpy() == fx.warm("actions")).all()
        assert (rp.rewards[:, index].cpu().numpy().astype(np.int32) == fx.warm("rewards")).all()
        assert (rp.terminals[:, index].cpu().numpy() == term).all()
        # ---- dqn_learn, step by step ----
        env.reset()
        env.metrics_reset()
        pop.reset_member_metrics()
        losses, syncs = [], 0
        for t in range(fx.steps):
            assert pop.epsilon == fx.epsilon_used[t], (t, pop.epsilon, fx.epsilon_used[t])
            a = pop.step(learn=True, cheat=fx.cheat)
            losses.append(pop.loss.cpu().numpy().copy())
            assert int(a[index]) == int(fx.actions[t]), (t, int(a[index]), int(fx.actions[t]), float(fx.gaps[t]), bool(fx.explored[t]))
            if t % fx.sync_every == fx.sync_every - 1:  # the reference's Q at this sync_target_Q
                got = pop.member_state(index)["target_Q"]
                for key, v in fx.weights("sync%d_Q" % syncs).items():
                    np.testing.assert_allclose(got[key].cpu().numpy(), v, rtol=DQN_RTOL, atol=DQN_ATOL, err_msg="%s at sync %d" % (key, syncs))
                syncs += 1
        assert syncs == len(fx.meta["syncs_at"]) >= 1
        losses = np.array(losses)
        np.testing.assert_allclose(losses[:, index], fx.losses, rtol=DQN_LOSS_RTOL, atol=1e-6)
        final = pop.member_state(index)
        for tag, sd in (("final_Q", final["Q"]), ("final_T", final["target_Q"])):
            for key, v in fx.weights(tag).items():
                np.testing.assert_allclose(sd[key].cpu().numpy(), v, rtol=DQN_RTOL, atol=DQN_ATOL, err_msg="%s %s" % (tag, key))
        assert (pop.step_count.cpu().numpy() == fx.steps).all() and pop.t == fx.steps
        assert (env.boards_host()[index].reshape(-1) == np.array(fx.meta["final_board"], dtype=np.int8)).all()
        assert int(env.episode_state_host()["episode_return"][index]) == fx.units(fx.meta["episode_return_at_stop"])
        vec, want = pop.member_metrics[index].cpu().numpy(), fx.episode_metrics()
        assert int(vec[O.M_EPISODES]) == want["episodes"] and int(vec[O.M_SUM_RETURN]) == want["sum_return"]
        assert int(vec[O.M_SUM_SAFETY]) == want["sum_safety"]
        for m in range(members):  # the neighbours learned something else
            assert m == index or not np.array_equal(losses[:, m], losses[:, index])
        # ---- default_eval, greedy ----
        per_member, total = pop.evaluate(fx.eval_timesteps)
        BG.assert_eval_metrics(per_member[index].vec, fx, O)
        assert total.episodes == sum(bm.episodes for bm in per_member)
    finally:
        env.close()


# ---- 7. capture ---------------------------------------------------------------------------------------------------------------------
def test_learn_batch_recorded_as_the_first_call_on_its_handle_equals_the_eager_calls():
    """The workspace is the caller's, so nothing has to be allocated on a first call: learn_batch is recorded under torch.cuda.graph (one
    stream, no parallel branches) as the FIRST learner call ever made on the handle; three replays in a row leave, replay by replay,
    the bytes three eager calls leave from the same start."""
    torch = _torch()
    members, E, slices, batch = 3, 5, 4, 7
    env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=6)
    try:
        pop = S.BatchedDeepQPopulation(env, _args(hidden=64, batch=batch), members, replay_slices=slices)
        pop.warmup(slices)
        used = torch.zeros((members, batch), dtype=torch.int64, device=pop.device)
        start = {k: t.clone() for k, t in pop.tensors().items()}

        def restore():
            for k, t in pop.tensors().items():
                t.copy_(start[k])
            used.zero_()

        def outputs():
            out = {k: t.cpu().numpy() for k, t in pop.tensors().items()}
            out["rows"] = used.cpu().numpy()
            return out

        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            pop.learn_batch(rows_out=used)
        torch.cuda.synchronize()
        _same_bytes({k: v.cpu().numpy() for k, v in start.items()}, {k: t.cpu().numpy() for k, t in pop.tensors().items()}, "recording")
        replayed = []
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            replayed.append(outputs())
        restore()
        for i in range(3):
            pop.learn_batch(rows_out=used)
            eager = outputs()
            assert (eager["step"] == i + 1).all() and np.abs(eager["m_w1"]).max() > 0 and eager["rows"].any()
            _same_bytes(eager, replayed[i], ("replay", i))
    finally:
        env.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_what_cannot_run_is_refused_with_the_reason():
    """n_envs % n_members != 0 (the C entry point and the Python layer), 128 hidden units, a batch of 65, three layers, a NULL workspace:
    an SgkError / ValueError that says why, and nothing launched (weights, step counters, the workspace and the env untouched)."""
    torch = _torch()
    env = S.BatchedGridworldEnv("BoatRace-v0", 15, seed=6)
    try:
        pop = S.BatchedDeepQPopulation(env, _args(hidden=64, batch=7), 3, replay_slices=4)
        pop.warmup(4)
        before = {k: t.clone() for k, t in pop.tensors().items()}
        handle = _handle_state(env)
        lib, dev, rp = env.lib, pop.device, pop.replay
        H, K0 = 64, env.n_cells
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        keep = {"w1": f(4, H, K0), "b1": f(4, H), "w2": f(4, H, H), "b2": f(4, H), "w3": f(4, 4, H), "b3": f(4, 4), "w1t": f(4, K0, H),
                "w2t": f(4, H, H), "w3t": f(4, H, 4), "tw1t": f(4, K0, H), "tb1": f(4, H), "tw2t": f(4, H, H), "tb2": f(4, H),
                "tw3": f(4, 4, H), "tb3": f(4, 4)}
        step = torch.zeros(4, dtype=torch.int64, device=dev)
        ws = torch.zeros(env.dqn_members_workspace_bytes(H, 4), dtype=torch.uint8, device=dev)

        def learner(hidden=64, batch=7):
            L = _lib.SgkDqnLearner()
            for k in RING:
                setattr(L, k, getattr(rp, k).data_ptr())
            L.slices_filled, L.n_hidden, L.batch, L.loss_mode = 4, hidden, batch, _lib.DQN_LOSS_REFERENCE
            for k, t in keep.items():
                setattr(L, k, t.data_ptr())
            for i, k in enumerate(DP.PARAMS):
                L.m[i], L.v[i], L.vmax[i] = keep[k].data_ptr(), keep[k].data_ptr(), keep[k].data_ptr()
            L.step = step.data_ptr()
            L.lr, L.beta1, L.beta2, L.eps, L.discount, L.max_grad_norm = 1e-3, 0.9, 0.999, 1e-8, 0.9, 10.0
            return L

        wp = ctypes.c_void_p(ws.data_ptr())
        for L, members, w, reason in ((learner(), 2, wp, b"n_members"), (learner(), 4, wp, b"n_members"), (learner(), 0, wp, b"n_members"),
                                      (learner(hidden=128), 3, wp, b"n_hidden"), (learner(batch=65), 3, wp, b"batch"),
                                      (learner(), 3, None, b"workspace")):
            rc = lib.sgk_dqn_sgd_step_members(env._h.ptr, ctypes.byref(L), members, None, w)
            assert rc == _lib.ERR_INVALID and reason in lib.sgk_last_error(), (members, lib.sgk_last_error())
        assert lib.sgk_dqn_members_workspace_bytes(env._h.ptr, 128, 3) == -1 and b"n_hidden" in lib.sgk_last_error()
        assert lib.sgk_dqn_members_workspace_bytes(env._h.ptr, 64, 0) == -1 and b"n_members" in lib.sgk_last_error()
        with pytest.raises(_lib.SgkError):
            env.dqn_members_workspace_bytes(128, 3)
        for bad in (2, 4, 0, -1):
            with pytest.raises(ValueError, match="n_members"):
                S.BatchedDeepQPopulation(env, _args(hidden=64, batch=7), bad)
        for kw, reason in ((dict(hidden=128), "n_hidden"), (dict(batch=65), "batch_size"), (dict(layers=3), "n_layers"), (dict(batch=0), "batch_size")):
            with pytest.raises(ValueError, match=reason):
                S.BatchedDeepQPopulation(env, _args(**dict(dict(hidden=64, batch=7), **kw)), 3)
        with pytest.raises(ValueError, match="rows"):  # a tensor argument of the wrong shape never reaches the kernel
            pop.learn_batch(rows=torch.zeros((3, 6), dtype=torch.int64, device=dev))
        with pytest.raises(ValueError, match="workspace"):
            env.dqn_sgd_step_members(learner(), 3, None, ws[:-16])
        torch.cuda.synchronize()
        assert int(step.abs().sum()) == 0 and int(ws.sum()) == 0 and all(int((t != 0).sum()) == 0 for t in keep.values())
        for k, t in pop.tensors().items():
            assert torch.equal(t, before[k]), k
        _same_bytes(handle, _handle_state(env), "after the refusals")
    finally:
        env.close()
