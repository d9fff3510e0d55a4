"""Per-member hyper-parameters of the populations on the GPU -- sgk_ppo_epochs_members_hyper, sgk_ppo_cnn_epochs_members_hyper,
sgk_dqn_sgd_step_members_hyper, sgk_policy_rollout_members_eps, sgk_discounted_returns_members; member_hyper / set_member_hyper of
BatchedPPOPopulation, BatchedPPOCNNPopulation, BatchedDeepQPopulation:

1. equal values are the old call: with every member given the `args` value, each new entry point leaves the bytes of its shared-hyper
   counterpart (parameters, transposes, Adam moments, steps, stats, rows_out; actions, step records and env state of the rollout; returns);
2. the invariant: member m with hyper-parameters h_m == the single agent on a handle of E envs created at env_index_base + m * E whose
   args carry h_m, bit for bit (two PPO iterations; 12 lockstep Deep-Q steps past the warm-up);
3. isolation: a change of member 1's lr / epsilon / discount moves member 1 and leaves members 0 and 2 byte-identical;
4. a recorded learn() follows set_member_hyper between replays; 5. refusals launch nothing.

Sizes: BoatRace (25-byte rows, members start unaligned) and SideEffectsSokoban (the second sprite), M = 3 members of E = 4 envs, batch
7, 2 epochs, H in {64, 100}, C = 5, a Deep-Q ring of 4 slices, T = the level's max_iterations; one case each with M = 5, E = 2 (member
strides that are no power of two).

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import ctypes
import functools
import types

import numpy as np
import pytest

import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib
from safe_grid_agents_amd import deepq_population as DP
from safe_grid_agents_amd import ppo_cnn_population as PC
from safe_grid_agents_amd import ppo_population as PP
from safe_grid_agents_amd.member_hyper import annealed_epsilon

pytestmark = pytest.mark.gpu

LEVELS = ["BoatRace-v0", "SideEffectsSokoban-v0"]
RING = ("states", "successors", "actions", "rewards", "terminals")
SEED, BASE, SLICES = 9, 1000, 4
# the values of test 2, member by member (the first three are the issue's; two more for the five-member case)
PPO_HYPER = {"lr": [1e-3, 3e-3, 1e-2, 5e-4, 2e-3], "clipping": [0.1, 0.2, 0.5, 0.3, 0.05], "critic_coeff": [1.0, 0.5, 2.0, 1.5, 0.25],
             "entropy_bonus": [0.0, 0.01, 0.05, 0.02, 0.1], "discount": [0.9, 0.99, 1.0, 0.95, 0.999]}
DQN_HYPER = {"lr": [1e-3, 3e-3, 1e-2, 5e-4, 2e-3], "discount": [0.9, 0.99, 0.995, 0.95, 0.999], "epsilon": [0.01, 0.1, 0.5, 0.05, 0.25]}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ppo_args(hidden=100, C=5, batch=7, epochs=2, rollouts=4, **hyper):
    kw = dict(lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01, discount=0.99)
    kw.update(hyper)
    return types.SimpleNamespace(batch_size=batch, rollouts=rollouts, epochs=epochs, n_layers=2, n_hidden=hidden, n_channels=C, device=0,
                                 log_gradients=False, cheat=False, seed=5, **kw)


def _dqn_args(hidden=100, batch=7, sync_every=8, **hyper):
    kw = dict(lr=1e-3, discount=0.99, epsilon=0.05)
    kw.update(hyper)
    return types.SimpleNamespace(batch_size=batch, sync_every=sync_every, epsilon_anneal=200, n_layers=2, n_hidden=hidden, seed=5, **kw)


def _hyper(table, members):
    return {k: v[:members] for k, v in table.items()}


def _with(args, **values):
    out = types.SimpleNamespace(**vars(args))
    vars(out).update(values)
    return out


def _handle_state(env):
    """Everything a rollout leaves in the handle: boards, last step records, the decoded state words, the episode arrays, the metrics."""
    v = env._device_views()
    out = {"boards": env.boards_host(), "records": env.step_records_host(), "metrics": env.metrics()}
    out.update({"word " + k: a for k, a in env.episode_state_host().items()})
    out.update({k: v[k].cpu().numpy() for k in ("last_return", "last_performance", "n_episodes")})
    return out


def _same_bytes(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def _differs(a, b, keys):
    return any(np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes() for k in keys)


def _rollout_bytes(ro, sl=None):
    if sl is None:
        return {k: getattr(ro, k).cpu().numpy() for k in ("states", "actions", "rewards", "returns", "lengths")}
    mine = {"states": ro.states[:, sl], "actions": ro.actions[:, sl], "rewards": ro.rewards[sl], "returns": ro.returns[sl], "lengths": ro.lengths[sl]}
    return {k: v.contiguous().cpu().numpy() for k, v in mine.items()}


def _pop_tensors(pop, m=None):
    """A population's learner state by name (member m's slice, or everything): tensors() + the stats where it has them."""
    out = dict(pop.tensors())
    if hasattr(pop, "stats"):
        out["stats"] = pop.stats
    return {k: (v if m is None else v[m]).detach().cpu().numpy() for k, v in out.items()}


# -- the two PPO bodies behind one face -------------------------------------------------------------------------------------------------
class _Mlp:
    population, params = S.BatchedPPOPopulation, PP.PARAMS

    @staticmethod
    def args(hidden, **kw):
        return _ppo_args(hidden=hidden, **kw)

    @staticmethod
    def agent(env, args, state_dict):
        agent = S.BatchedPPOAgent(env, args)
        agent.net.load_state_dict(state_dict)
        agent.sync()
        return agent

    @staticmethod
    def learn(agent, rollout, rows_out):
        agent._learn_fused(rollout, rows_out=rows_out)

    @staticmethod
    def agent_state(agent):
        pl = agent._pl
        out = {"stats": agent._stats.cpu().numpy(), "step": pl["step"].cpu().numpy()[0], "w1t": pl["w1t"].cpu().numpy(),
               "w2t": pl["w2t"].cpu().numpy()}
        for i, k in enumerate(PP.PARAMS):
            out.update({k: agent._own_tensors()[i].cpu().numpy(), "m_" + k: pl["m"][i].cpu().numpy(), "v_" + k: pl["v"][i].cpu().numpy()})
        return out


class _Cnn:
    population, params = S.BatchedPPOCNNPopulation, PC.PARAMS

    @staticmethod
    def args(hidden, **kw):  # (`hidden` is the MLP's; the conv body has C = 5 channels)
        return _ppo_args(hidden=None, C=5, **kw)

    @staticmethod
    def agent(env, args, state_dict):
        agent = S.BatchedPPOAgent(env, args, body="cnn", fused_conv_learn=True)
        assert agent.fused_conv and agent.fused_learn and agent.fused_rollout
        agent.net.load_state_dict(state_dict)
        agent.sync()
        return agent

    @staticmethod
    def learn(agent, rollout, rows_out):
        agent._learn_fused_cnn(rollout, rows_out=rows_out)

    @staticmethod
    def agent_state(agent):
        named, pl = dict(agent.net.named_parameters()), agent._pl
        out = {"stats": agent._stats.cpu().numpy(), "step": pl["step"].cpu().numpy()[0]}
        for i, (key, k) in enumerate(zip(agent.CNN_PARAMS, PC.PARAMS)):
            out.update({k: named[key].data.cpu().numpy(), "m_" + k: pl["m"][i].cpu().numpy(), "v_" + k: pl["v"][i].cpu().numpy()})
        return out


PPO_CASES = [(_Mlp, name, 3, 4, hidden) for name in LEVELS for hidden in (64, 100)] + [(_Cnn, name, 3, 4, None) for name in LEVELS]
PPO_IDS = ["%s-%s-M%d-E%d-%s" % (b.__name__[1:], n[:4], m, e, h) for b, n, m, e, h in PPO_CASES + [(_Mlp, "BoatRace-v0", 5, 2, 100), (_Cnn, "BoatRace-v0", 5, 2, None)]]


# ---- 1. equal values are the old call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,name,members,E,hidden", PPO_CASES, ids=PPO_IDS[:len(PPO_CASES)])
def test_ppo_equal_values_leave_the_bytes_of_the_shared_call(body, name, members, E, hidden):
    """Two populations from the same seeds on two handles, one with member_hyper = args' values for every member (the _hyper entry point
    and the per-member returns table), one without (today's calls): two gather / learn / sync iterations leave the same rollout --
    states, actions, rewards, lengths, RETURNS --, handle state, parameters, transposes, Adam moments, steps, stats and rows_out."""
    torch = _torch()
    args = body.args(hidden, rollouts=E)
    envs = [S.BatchedGridworldEnv(name, members * E, seed=SEED, env_index_base=BASE) for _ in range(2)]
    try:
        same = {k: [getattr(args, k)] * members for k in PP.PPO_NAMES}
        pops = [body.population(envs[0], args, members), body.population(envs[1], args, members, member_hyper=same)]
        assert pops[0].hyper is None and tuple(pops[1].hyper["learner"].shape) == (members, 4)
        assert pops[1].hyper["learner"].dtype == torch.float64
        used = [torch.zeros((members, args.epochs, args.batch_size), dtype=torch.int64, device=p.device) for p in pops]
        for it in range(2):
            got = []
            for pop, env, rows in zip(pops, envs, used):
                ro = pop.gather_rollout()
                snap = {"ro " + k: v for k, v in _rollout_bytes(ro).items()}
                snap.update({"env " + k: v for k, v in _handle_state(env).items()})
                pop.learn(ro, rows_out=rows)
                snap.update(_pop_tensors(pop))
                snap["rows"] = rows.cpu().numpy()
                pop.sync()
                got.append(snap)
            assert (got[0]["step"] == args.epochs * (it + 1)).all() and np.abs(got[0]["m_w1"]).max() > 0 and got[0]["rows"].any()
            assert np.abs(got[0]["ro returns"]).max() > 0
            _same_bytes(got[0], got[1], (name, it))
        assert tuple(pops[1].hyper["gamma_pow"].shape) == (members, int(envs[1].info.max_iterations))
    finally:
        for env in envs:
            env.close()


@pytest.mark.parametrize("hidden", [64, 100])
@pytest.mark.parametrize("name", LEVELS)
def test_dqn_equal_values_leave_the_bytes_of_the_shared_call(name, hidden):
    """The same for Deep-Q: a warm-up of the ring and 10 lockstep learning steps (one target sync inside) with member_hyper = args' lr,
    discount and epsilon for every member against the population without it: actions, handle state, ring, minibatch rows and every
    learner tensor after each step. The annealed per-member epsilon is the shared float, bit for bit."""
    torch = _torch()
    members, E = 3, 4
    args = _dqn_args(hidden=hidden)
    envs = [S.BatchedGridworldEnv(name, members * E, seed=SEED, env_index_base=BASE) for _ in range(2)]
    try:
        same = {k: [getattr(args, k)] * members for k in DP.DQN_NAMES}
        pops = [S.BatchedDeepQPopulation(envs[0], args, members, replay_slices=SLICES),
                S.BatchedDeepQPopulation(envs[1], args, members, replay_slices=SLICES, member_hyper=same)]
        assert tuple(pops[1].hyper["learner"].shape) == (members, 2) and pops[1].hyper["learner"].dtype == torch.float64
        used = [torch.zeros((members, args.batch_size), dtype=torch.int64, device=p.device) for p in pops]
        for pop, env, rows in zip(pops, envs, used):
            pop.learn_batch = functools.partial(pop.learn_batch, rows_out=rows)
            pop.warmup(SLICES)
            env.reset()
            env.metrics_reset()
            pop.reset_member_metrics()
        for t in range(10):
            got = []
            for pop, env, rows in zip(pops, envs, used):
                snap = {"actions": pop.step(learn=True).cpu().numpy(), "rows": rows.cpu().numpy()}
                snap.update({"env " + k: v for k, v in _handle_state(env).items()})
                snap.update({"ring " + k: getattr(pop.replay, k).cpu().numpy() for k in RING})
                snap.update(_pop_tensors(pop))
                got.append(snap)
            _same_bytes(got[0], got[1], (name, hidden, t))
            eps = pops[1].epsilon.cpu().numpy()
            assert eps.dtype == np.float64 and (eps == pops[0].epsilon).all() and pops[0].epsilon < 1.0
        assert (got[0]["step"] == 10).all() and len(np.unique(got[0]["actions"])) > 1
    finally:
        for env in envs:
            env.close()


@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("name", LEVELS)
def test_rollout_with_equal_epsilons_leaves_the_bytes_of_the_shared_call(name, mode):
    """sgk_policy_rollout_members_eps with every member's epsilon = 0.25 against sgk_policy_rollout_members(epsilon = 0.25), 12 steps
    from max_iterations - 7 random steps into the episodes (episodes end inside): states, actions, step records (sentinel-filled
    buffers), member metrics and the handle. Mode 1 ignores the array (0.9 there changes nothing)."""
    torch = _torch()
    members, E, steps, hidden = 3, 4, 12, 100
    n = members * E
    envs = [S.BatchedGridworldEnv(name, n, seed=21, env_index_base=300) for _ in range(2)]
    try:
        dev = "cuda:%d" % envs[0].device
        rng = np.random.default_rng(3)
        shapes = {"w1t": (envs[0].n_cells, hidden), "b1": (hidden,), "w2": (hidden, hidden), "b2": (hidden,), "w3t": (hidden, 4), "b3": (4,)}
        w = {k: torch.as_tensor(rng.normal(0.0, 0.3, (members,) + s).astype(np.float32)).to(dev) for k, s in shapes.items()}
        eps = torch.full((members,), 0.25 if mode == "greedy" else 0.9, dtype=torch.float64, device=dev)
        got = []
        for i, env in enumerate(envs):
            env.step_random(int(env.info.max_iterations) - 7, auto_reset=True)
            buf = {"states": torch.full((steps, n, env.n_cells), 77, dtype=torch.int8, device=dev),
                   "actions": torch.full((steps, n), 77, dtype=torch.uint8, device=dev),
                   "recs": torch.full((steps, n, 4), 77, dtype=torch.int8, device=dev)}
            mm = torch.zeros((members, _lib.METRICS_LEN), dtype=torch.int64, device=dev)
            env.policy_rollout_members(w, members, steps, mode=mode, epsilon=0.25, draw_index0=1000, auto_reset=True,
                                       mask_finished=mode == "sample", member_metrics=mm, member_epsilon=eps if i else None, **buf)
            snap = _handle_state(env)
            snap.update({k: v.cpu().numpy() for k, v in buf.items()})
            snap["member_metrics"] = mm.cpu().numpy()
            got.append(snap)
        assert got[0]["metrics"][_lib.M_EPISODES] > 0 and (got[0]["states"] != 77).all() and len(np.unique(got[0]["actions"])) > 1
        _same_bytes(got[0], got[1], (name, mode))
    finally:
        for env in envs:
            env.close()


def test_returns_with_equal_rows_are_the_shared_scan_and_rows_are_read_per_member():
    """sgk_discounted_returns_members on random rewards, 15 trajectories of up to 100 steps (ragged lengths, a tail past one 64-lane
    round): with every row = discount_powers(0.99) the bytes of sgk_discounted_returns(0.99); with three different rows, member m's
    trajectories are the shared scan with ITS discount (5 trajectories per member: rows change at i / 5, no power of two)."""
    torch = _torch()
    env = S.BatchedGridworldEnv("BoatRace-v0", 15, seed=1)
    try:
        dev, T, n = "cuda:%d" % env.device, 100, 15
        rng = np.random.default_rng(7)
        rewards = torch.as_tensor(rng.integers(-3, 4, (n, T)).astype(np.float32)).to(dev)
        lengths = torch.as_tensor(rng.integers(1, T + 1, n).astype(np.int32)).to(dev)
        lengths[3], lengths[4] = T, 1
        table = lambda ds: torch.as_tensor(np.stack([_lib.discount_powers(d, T) for d in ds])).to(dev)  # noqa: E731
        shared = {d: env.discounted_returns(rewards, d, lengths=lengths).cpu().numpy() for d in (0.9, 0.99, 1.0)}
        same = env.discounted_returns_members(rewards, table([0.99] * 3), lengths=lengths).cpu().numpy()
        assert np.abs(same).max() > 0 and same.tobytes() == shared[0.99].tobytes()
        mixed = env.discounted_returns_members(rewards, table([0.9, 0.99, 1.0]), lengths=lengths).cpu().numpy()
        for m, d in enumerate((0.9, 0.99, 1.0)):
            assert mixed[5 * m:5 * m + 5].tobytes() == shared[d][5 * m:5 * m + 5].tobytes(), m
        assert mixed[:5].tobytes() != shared[0.99][:5].tobytes()
        one = env.discounted_returns_members(rewards, table([0.9]), lengths=lengths).cpu().numpy()  # one member: the whole batch
        assert one.tobytes() == shared[0.9].tobytes()
    finally:
        env.close()


# ---- 2. the invariant ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,name,members,E,hidden", PPO_CASES + [(_Mlp, "BoatRace-v0", 5, 2, 100), (_Cnn, "BoatRace-v0", 5, 2, None)],
                         ids=PPO_IDS)
def test_a_ppo_member_with_its_own_hyper_parameters_is_the_single_agent_with_them(body, name, members, E, hidden):
    """Two PPO iterations (gather, learn, sync) of a population whose members differ in lr, clipping, critic_coeff, entropy_bonus and
    discount, against one BatchedPPOAgent per member on a handle of its own -- BatchedGridworldEnv(level, E, seed, env_index_base =
    base + m * E) -- built from args that carry member m's values, with member m's weights and the same minibatch key: rollout
    (returns under the member's discount), rows, stats, step, parameters and Adam moments as bytes."""
    torch = _torch()
    args = body.args(hidden, rollouts=E)
    hyper = _hyper(PPO_HYPER, members)
    env = S.BatchedGridworldEnv(name, members * E, seed=SEED, env_index_base=BASE)
    singles = [S.BatchedGridworldEnv(name, E, seed=SEED, env_index_base=BASE + m * E) for m in range(members)]
    try:
        pop = body.population(env, args, members, member_seeds=[31 + m for m in range(members)], member_keys=[SEED] * members,
                              member_hyper=hyper)
        agents = []
        for m, e in enumerate(singles):
            h_m = {k: v[m] for k, v in hyper.items()}
            assert pop.member_hyper_of(m) == h_m
            handed = pop.member(m)  # the single agent the population hands out is built from member m's values
            assert (handed.discount, handed.clipping, handed.entropy_bonus, handed.critic_coeff) == (
                h_m["discount"], h_m["clipping"], h_m["entropy_bonus"], h_m["critic_coeff"])
            agents.append(body.agent(e, _with(args, **h_m), handed.state_dict()))
        N, dev = members * E, pop.device
        used = torch.zeros((members, args.epochs, args.batch_size), dtype=torch.int64, device=dev)
        used_m = torch.zeros((args.epochs, args.batch_size), dtype=torch.int64, device=dev)
        for it in range(2):
            ro = pop.gather_rollout()
            pop.learn(ro, rows_out=used)
            for m, (e, agent) in enumerate(zip(singles, agents)):
                rm = agent.gather_rollout()
                _same_bytes(_rollout_bytes(rm), _rollout_bytes(ro, slice(m * E, (m + 1) * E)), ("rollout", it, m))
                body.learn(agent, rm, used_m)
                rows = used[m].cpu().numpy()
                t, col = rows // N, rows % N
                assert ((col >= m * E) & (col < (m + 1) * E)).all(), (it, m)  # a member draws from its own trajectories
                assert (t * E + (col - m * E) == used_m.cpu().numpy()).all(), (it, m)
                a = body.agent_state(agent)
                b = {k: v for k, v in _pop_tensors(pop, m).items() if k in a}
                assert int(a["step"]) == args.epochs * (it + 1) and np.isfinite(a["stats"]).all() and np.abs(a["m_w1"]).max() > 0
                _same_bytes(a, b, ("learn", it, m))
                agent.sync()
            pop.sync()
    finally:
        env.close()
        for e in singles:
            e.close()


def _load_dqn_agent(torch, agent, q_state, t_state):
    """A BatchedDeepQAgent's two networks <- state dicts, the fused kernels' transposed copies refreshed."""
    dev = agent.device
    agent.Q.load_state_dict({k: torch.as_tensor(v).to(dev) for k, v in q_state.items()})
    agent.target_Q.load_state_dict({k: torch.as_tensor(v).to(dev) for k, v in t_state.items()})
    agent._refresh_fused_weights()
    agent._fl["w2t"].copy_(agent.Q[1][0][0].weight.data.t())
    agent._refresh_target_transposes()


def _dqn_agent_state(agent):
    """Everything sgk_dqn_sgd_step reads and updates of a BatchedDeepQAgent, under the population's tensor names."""
    fl, fw = agent._fl, agent._fw
    out = {"w1t": fw["w1t"], "w2t": fl["w2t"], "w3t": fw["w3t"], "step": fl["step"][0], "loss": fl["loss"][0],
           "target_w1t": fl["tw1t"], "target_w2t": fl["tw2t"]}
    for i, (k, p, tp) in enumerate(zip(DP.PARAMS, agent.Q.parameters(), agent.target_Q.parameters())):
        out.update({k: p.data, "m_" + k: fl["m"][i], "v_" + k: fl["v"][i], "vmax_" + k: fl["vmax"][i], "target_" + k: tp.data})
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name,members,E,hidden", [(n, 3, 4, h) for n in LEVELS for h in (64, 100)] + [("BoatRace-v0", 5, 2, 100)])
def test_a_dqn_member_with_its_own_hyper_parameters_is_the_single_agent_with_them(name, members, E, hidden):
    """A warm-up of the whole ring, then 12 lockstep learning steps (sync_every = 8: one target sync inside) of a population whose members
    differ in lr, discount and the starting epsilon, against one BatchedDeepQAgent(sgd_steps=1, fused_learn=True) per member on a handle
    of its own built from args that carry member m's values. After every step: actions, the member's annealed epsilon (the single
    agent's float, bit for bit), the handle's state, the ring columns, the minibatch rows and every learner tensor."""
    torch = _torch()
    steps, batch = 12, 7
    args = _dqn_args(hidden=hidden, batch=batch)
    hyper = _hyper(DQN_HYPER, members)
    N = members * E
    env = S.BatchedGridworldEnv(name, N, seed=SEED, env_index_base=BASE)
    singles = [S.BatchedGridworldEnv(name, E, seed=SEED, env_index_base=BASE + m * E) for m in range(members)]
    try:
        pop = S.BatchedDeepQPopulation(env, args, members, member_seeds=[31 + m for m in range(members)], member_keys=[SEED] * members,
                                       replay_slices=SLICES, member_hyper=hyper)
        dev = pop.device
        used = torch.zeros((members, batch), dtype=torch.int64, device=dev)
        used_m = torch.zeros(batch, dtype=torch.int64, device=dev)
        pop.learn_batch = functools.partial(pop.learn_batch, rows_out=used)  # (step() calls self.learn_batch())
        agents = []
        for m, e in enumerate(singles):
            st = pop.member_state(m)
            assert st["hyper"] == {k: v[m] for k, v in hyper.items()}
            agent = S.BatchedDeepQAgent(e, _with(args, **st["hyper"]), sgd_steps=1, replay_slices=SLICES, fused_learn=True)
            assert agent.fused_learn
            agent.fuse_reset = False
            _load_dqn_agent(torch, agent, st["Q"], st["target_Q"])
            agent.learn_batch = functools.partial(agent._learn_batch_fused, rows_out=used_m)
            agents.append(agent)

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
                _same_bytes(_pop_tensors(pop, m), _dqn_agent_state(agent), (what, "learner", m))

        pop.warmup(SLICES)
        for agent in agents:
            agent.warmup(SLICES)
        for e in [env] + singles:
            e.reset()
            e.metrics_reset()
        pop.reset_member_metrics()
        compare("warm-up")
        for t in range(steps):
            eps = pop.epsilon.cpu().numpy().copy()  # the values this step acts with
            for m, agent in enumerate(agents):
                assert eps[m] == agent.epsilon == annealed_epsilon(hyper["epsilon"][m], t, args.epsilon_anneal), (t, m)
            a = pop.step(learn=True).cpu().numpy()
            rows = used.cpu().numpy()
            for m, agent in enumerate(agents):
                am = agent.step(learn=True).cpu().numpy()
                assert a[m * E:(m + 1) * E].tobytes() == am.tobytes(), (t, m)
                sl_, col = rows[m] // N, rows[m] % N
                assert ((col >= m * E) & (col < (m + 1) * E)).all(), (t, m)  # a member draws from its own columns
                assert (sl_ * E + (col - m * E) == used_m.cpu().numpy()).all(), (t, m)
                assert agent.t == pop.t
            compare("step %d" % t)
        assert int(pop.step_count[0]) == steps and pop.t == steps
    finally:
        env.close()
        for e in singles:
            e.close()


# ---- 3. isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", [_Mlp, _Cnn], ids=["Mlp", "Cnn"])
def test_changing_member_1s_lr_or_discount_moves_member_1_alone(body):
    """Two populations from the same seeds; the second gets member 1's lr x 10, then (set_member_hyper) member 1's discount 0.5: after a
    gather + learn the members 0 and 2 are byte-identical in returns and in every learner tensor, member 1 is not."""
    torch = _torch()
    members, E = 3, 4
    args = body.args(64, rollouts=E)
    envs = [S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=SEED, env_index_base=BASE) for _ in range(2)]
    try:
        base = {k: [getattr(args, k)] * members for k in PP.PPO_NAMES}
        other = dict(base, lr=[args.lr, args.lr * 10, args.lr])
        pops = [body.population(envs[0], args, members, member_hyper=base), body.population(envs[1], args, members, member_hyper=other)]
        pops[1].set_member_hyper("discount", [args.discount, 0.5, args.discount])
        assert pops[1].member_hyper_of(1)["discount"] == 0.5 and pops[1].member_hyper_of(2)["discount"] == args.discount
        ros = [p.gather_rollout() for p in pops]
        for m in range(members):
            sl = slice(m * E, (m + 1) * E)
            a, b = _rollout_bytes(ros[0], sl), _rollout_bytes(ros[1], sl)
            _same_bytes({k: v for k, v in a.items() if k != "returns"}, {k: v for k, v in b.items() if k != "returns"}, ("rollout", m))
            assert (a["returns"].tobytes() != b["returns"].tobytes()) == (m == 1), m  # the discount reaches member 1's returns alone
        pops[1].set_member_hyper("discount", base["discount"])  # back: from here on only the lr differs
        ros[1] = pops[1].gather_rollout()
        ros[0] = pops[0].gather_rollout()
        _same_bytes(_rollout_bytes(ros[0]), _rollout_bytes(ros[1]), "rollouts after the discount went back")
        for p, ro in zip(pops, ros):
            p.learn(ro)
        for m in range(members):
            a, b = _pop_tensors(pops[0], m), _pop_tensors(pops[1], m)
            if m == 1:
                assert _differs(a, b, ["w1", "m_w1"]) and a["step"] == b["step"]
            else:
                _same_bytes(a, b, ("learn", m))
    finally:
        for env in envs:
            env.close()


def test_changing_member_1s_dqn_values_moves_member_1_alone():
    """Deep-Q: member 1's epsilon 0.05 -> 1.0 changes member 1's actions alone (one acting step from equal states); member 1's lr and
    discount change member 1's learner tensors alone (one learn_batch on the same ring)."""
    torch = _torch()
    members, E = 3, 4
    args = _dqn_args(hidden=64)
    envs = [S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=SEED, env_index_base=BASE) for _ in range(2)]
    try:
        base = {k: [getattr(args, k)] * members for k in DP.DQN_NAMES}
        pops = [S.BatchedDeepQPopulation(e, args, members, replay_slices=SLICES, member_hyper=base) for e in envs]
        for pop, env in zip(pops, envs):
            pop.warmup(SLICES)
            env.reset()
            pop.t = 150  # far into the schedule: epsilon 0.2875 for a start of 0.05, still 1.0 for a start of 1.0
        pops[1].set_member_hyper("epsilon", [args.epsilon, 1.0, args.epsilon])
        acts = []
        for _ in range(6):  # six acting steps without learning: 24 draws per member
            acts.append([pop.step(learn=False).cpu().numpy() for pop in pops])
        a, b = np.stack([x[0] for x in acts], 0), np.stack([x[1] for x in acts], 0)
        for m in range(members):
            sl = slice(m * E, (m + 1) * E)
            if m == 1:
                assert a[0][sl].tobytes() != b[0][sl].tobytes() or a[:, sl].tobytes() != b[:, sl].tobytes()
            else:
                assert a[0][sl].tobytes() == b[0][sl].tobytes(), m  # (the first step starts from equal states)
        assert a[:, E:2 * E].tobytes() != b[:, E:2 * E].tobytes()
        # the learner: fresh rings, then one SGD step with member 1's lr x 10 and discount 0.5
        for pop in pops:
            pop.warmup(SLICES)
        pops[1].set_member_hyper("lr", [args.lr, args.lr * 10, args.lr])
        pops[1].set_member_hyper("discount", [args.discount, 0.5, args.discount])
        for pop in pops:
            pop.learn_batch()
        for m in range(members):
            x, y = _pop_tensors(pops[0], m), _pop_tensors(pops[1], m)
            if m == 1:
                assert _differs(x, y, ["w1"]) and _differs(x, y, ["loss"]) and x["step"] == y["step"] == 1
            else:
                _same_bytes(x, y, ("learn", m))
    finally:
        for env in envs:
            env.close()


# ---- 4. a recorded learn() follows set_member_hyper ---------------------------------------------------------------------------------
@pytest.mark.parametrize("body", [_Mlp, _Cnn], ids=["Mlp", "Cnn"])
def test_a_replayed_learn_runs_with_the_values_set_between_replays(body):
    """pop.learn recorded once under torch.cuda.graph after a warm-up call; replayed from the same start; set_member_hyper("lr", ...) and
    ("clipping", ...); replayed again from the same start: the first replay equals the eager call with the old values, the second the
    eager call with the new ones (and differs from the first) -- the kernels read the values when they run, the tensors kept their
    addresses."""
    torch = _torch()
    members, E = 3, 4
    args = body.args(64, rollouts=E)
    env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=6)
    try:
        pop = body.population(env, args, members, member_hyper=_hyper(PPO_HYPER, members))
        address = pop.hyper["learner"].data_ptr()
        ro = pop.gather_rollout()
        used = torch.zeros((members, args.epochs, args.batch_size), dtype=torch.int64, device=pop.device)
        start = {k: t.clone() for k, t in pop.tensors().items()}

        def restore():
            for k, t in pop.tensors().items():
                t.copy_(start[k])
            used.zero_(); pop.stats.zero_()

        def outputs():
            out = _pop_tensors(pop)
            out["rows"] = used.cpu().numpy()
            return out

        new_lr, new_clip = [3e-2, 1e-3, 4e-3], [0.3, 0.1, 0.05]
        pop.learn(ro, rows_out=used)  # eager (also the warm-up: the kernel's attributes are set)
        eager_old = outputs()
        restore()
        pop.set_member_hyper("lr", new_lr)
        pop.set_member_hyper("clipping", new_clip)
        pop.learn(ro, rows_out=used)
        eager_new = outputs()
        assert _differs(eager_old, eager_new, ["w1"]) and pop.hyper["learner"].data_ptr() == address
        pop.set_member_hyper("lr", PPO_HYPER["lr"][:members])
        pop.set_member_hyper("clipping", PPO_HYPER["clipping"][:members])
        restore()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            pop.learn(ro, rows_out=used)
        restore()
        graph.replay()
        torch.cuda.synchronize()
        _same_bytes(eager_old, outputs(), "replay with the recorded values")
        pop.set_member_hyper("lr", new_lr)
        pop.set_member_hyper("clipping", new_clip)
        restore()
        graph.replay()
        torch.cuda.synchronize()
        _same_bytes(eager_new, outputs(), "replay after set_member_hyper")
    finally:
        env.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """A NULL per-member pointer, a member count that does not divide the batch, and the shapes the shared calls refuse, through the new
    entry points: SGK_ERR_INVALID with the shared call's reason; bad values through set_member_hyper: ValueError. Afterwards the
    handle's state, every learner tensor and the device values are byte-identical."""
    torch = _torch()
    members, E = 3, 4
    env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=6)
    try:
        args = _ppo_args(hidden=64, rollouts=E)
        pop = S.BatchedPPOPopulation(env, args, members, member_hyper=_hyper(PPO_HYPER, members))
        dq = S.BatchedDeepQPopulation(env, _dqn_args(hidden=64), members, replay_slices=SLICES, member_hyper=_hyper(DQN_HYPER, members))
        dq.warmup(SLICES)
        env.reset()
        ro = pop.gather_rollout()
        lib, dev, h = env.lib, pop.device, env._h.ptr
        before = {"pop": _pop_tensors(pop), "dq": _pop_tensors(dq), "env": _handle_state(env),
                  "hyper": {k: v.cpu().numpy() for k, v in list(pop.hyper.items()) + [("dq " + k, v) for k, v in dq.hyper.items()]},
                  "returns": ro.returns.cpu().numpy()}
        T = int(ro.actions.shape[0])
        hp, dhp = pop.hyper["learner"].data_ptr(), dq.hyper["learner"].data_ptr()
        # the rollout: its own NULL, and the sibling's refusals with the sibling's words
        w = env._member_weights_arg(pop._old_weights(), members)
        eps = torch.zeros(members, dtype=torch.float64, device=dev)
        roll = lambda m, mode, e: lib.sgk_policy_rollout_members_eps(h, ctypes.byref(w), m, mode, 0.0, 0, 5, 0, None, None, None, None, e)  # noqa: E731
        assert roll(members, 0, None) == _lib.ERR_INVALID and b"member_epsilon_dev is NULL" in lib.sgk_last_error()
        for bad in (5, 0, -1):
            assert roll(bad, 0, eps.data_ptr()) == _lib.ERR_INVALID and b"n_members" in lib.sgk_last_error()
            assert lib.sgk_policy_rollout_members(h, ctypes.byref(w), bad, 0, 0.0, 0, 5, 0, None, None, None, None) == _lib.ERR_INVALID
        assert roll(members, 2, eps.data_ptr()) == _lib.ERR_INVALID and b"mode" in lib.sgk_last_error()
        # the returns
        ret = lambda m, t, g: lib.sgk_discounted_returns_members(h, ro.rewards.data_ptr(), None, ro.returns.data_ptr(), members * E, t, m, g)  # noqa: E731
        g = pop.hyper["gamma_pow"].data_ptr()
        assert ret(members, T, None) == _lib.ERR_INVALID and b"gamma_pow_dev is NULL" in lib.sgk_last_error()
        assert ret(5, T, g) == _lib.ERR_INVALID and b"n_members" in lib.sgk_last_error()
        assert ret(0, T, g) == _lib.ERR_INVALID and b"n_members" in lib.sgk_last_error()
        assert ret(members, 1025, g) == _lib.ERR_INVALID and b"t_max" in lib.sgk_last_error()
        # the PPO learner: a struct the library accepts (the population's own), then one thing wrong at a time
        captured = {}
        real = env.ppo_epochs_members
        env.ppo_epochs_members = lambda L, M, keys, member_hyper=None: captured.update(L=L)  # (takes the struct, launches nothing)
        pop.learn(ro)
        env.ppo_epochs_members = real
        L = captured["L"]
        ppo = lambda m, p: lib.sgk_ppo_epochs_members_hyper(h, ctypes.byref(L), m, None, p)  # noqa: E731
        assert ppo(members, None) == _lib.ERR_INVALID and b"hyper_dev is NULL" in lib.sgk_last_error()
        for bad in (5, 0):
            assert ppo(bad, hp) == _lib.ERR_INVALID and b"n_members" in lib.sgk_last_error()
        for field, value, reason in (("n_hidden", 128, b"n_hidden"), ("batch", 65, b"batch"), ("n_epochs", 0, b"n_epochs")):
            keep = getattr(L, field)
            setattr(L, field, value)
            assert ppo(members, hp) == _lib.ERR_INVALID and reason in lib.sgk_last_error(), field
            assert lib.sgk_ppo_epochs_members(h, ctypes.byref(L), members, None) == _lib.ERR_INVALID and reason in lib.sgk_last_error()
            setattr(L, field, keep)
        # the Deep-Q learner
        D = dq._learner()
        D.slices_filled = int(dq.replay.filled)
        ws = dq.workspace.data_ptr()
        dqn = lambda m, wsp, p: lib.sgk_dqn_sgd_step_members_hyper(h, ctypes.byref(D), m, None, wsp, p)  # noqa: E731
        assert dqn(members, ws, None) == _lib.ERR_INVALID and b"hyper_dev is NULL" in lib.sgk_last_error()
        assert dqn(5, ws, dhp) == _lib.ERR_INVALID and b"n_members" in lib.sgk_last_error()
        assert dqn(members, None, dhp) == _lib.ERR_INVALID and b"workspace" in lib.sgk_last_error()
        keep, D.batch = D.batch, 65
        assert dqn(members, ws, dhp) == _lib.ERR_INVALID and b"batch" in lib.sgk_last_error()
        D.batch = keep
        # the Python layer: tensors of the wrong shape / dtype never reach a kernel; values are validated
        with pytest.raises(ValueError, match="member_hyper"):
            env.ppo_epochs_members(L, members, None, member_hyper=pop.hyper["learner"][:2])
        with pytest.raises(ValueError, match="member_hyper"):
            env.ppo_epochs_members(L, members, None, member_hyper=pop.hyper["learner"].to(torch.float32))
        with pytest.raises(ValueError, match="member_epsilon"):
            env.policy_rollout_members(pop._old_weights(), members, 5, mode="greedy", member_epsilon=eps.to(torch.float32))
        with pytest.raises(ValueError, match="gamma_pow"):
            env.discounted_returns_members(ro.rewards, pop.hyper["gamma_pow"][:, :T - 1].contiguous())
        for p, name, bad, reason in ((pop, "lr", [1e-3, 0.0, 1e-3], "lr must be > 0"), (pop, "discount", [0.9, 1.5, 0.9], r"\(0, 1\]"),
                                     (pop, "lr", [1e-3, 1e-3], "2 values"), (pop, "epsilon", [0.1] * 3, "no 'epsilon' here"),
                                     (dq, "epsilon", [0.1, 1.5, 0.1], r"\[0, 1\]"), (dq, "clipping", [0.1] * 3, "no 'clipping' here"),
                                     (dq, "lr", [1e-3, float("nan"), 1e-3], "not finite")):
            with pytest.raises(ValueError, match=reason):
                p.set_member_hyper(name, bad)
        shared = S.BatchedPPOPopulation(env, args, members)
        with pytest.raises(ValueError, match="without member_hyper"):
            shared.set_member_hyper("lr", [1e-3] * 3)
        torch.cuda.synchronize()
        after = {"pop": _pop_tensors(pop), "dq": _pop_tensors(dq), "env": _handle_state(env),
                 "hyper": {k: v.cpu().numpy() for k, v in list(pop.hyper.items()) + [("dq " + k, v) for k, v in dq.hyper.items()]},
                 "returns": ro.returns.cpu().numpy()}
        for k in before:
            if isinstance(before[k], dict):
                _same_bytes(before[k], after[k], k)
            else:
                assert before[k].tobytes() == after[k].tobytes(), k
        assert pop.member_values["lr"] == PPO_HYPER["lr"][:members] and dq.member_values["epsilon"] == DQN_HYPER["epsilon"][:members]
    finally:
        env.close()
