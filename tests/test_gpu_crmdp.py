"""ppo-crmdp on the GPU: sgk_crmdp_keys, sgk_crmdp_filter (detect + merge) and BatchedPPOCRMDPAgent. Every comparison is exact (integers
as they are, floats through their bytes).

1. the device filter on the reference's plans (48 trajectories, t_max 100, 6 agents; also as ONE agent) == sgk_crmdp_filter_host, byte for
   byte in the five outputs and the three tables -- and the host call is held to the reference by tests/test_crmdp_cpu.py;
2. eight replicas of the plans on a handle whose grids are capped at 64 workgroups (SGK_MAX_GRID, read at sgk_create; the keys and the
   detect kernels honour it, the merge kernel's grid is the agents): 384 trajectories against 256 waves, so a workgroup serves a second
   pass -- every replica leaves the small call's bytes;
3. the keys kernel == numpy's argmax on the boards of a real BoatRace rollout: 130 envs (two full tiles and one of two envs; the odd steps'
   tiles are not dword-aligned), a board without an agent gives -1;
4. BatchedPPOCRMDPAgent.gather_rollout on 64 envs, two iterations in a row: states, actions and records equal a twin BatchedPPOAgent's,
   the filtered rewards and the memory equal the dictionary restatement applied to the device trajectories, the returns equal
   env.discounted_returns of the filtered rewards; then learn() runs on the second rollout, with fused_conv_learn on and off;
5. guard bands (tests/guard_arena.py): no field of sgk_crmdp_buffers is written outside its buffer, no input changes;
6. keys + filter recorded in a graph replay to the same bytes.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import types

import numpy as np
import pytest

import crmdp_plans as P
import crmdp_reference as R
import guard_arena as GA
import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib, crmdp
from safe_grid_agents_amd.loops import batched_gather_rollout

pytestmark = pytest.mark.gpu

BOAT = "BoatRace-v0"


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _args(rollouts, seed=5, batch=16):
    return types.SimpleNamespace(discount=0.99, batch_size=batch, rollouts=rollouts, epochs=2, n_layers=2, n_hidden=None, n_channels=5, device=0,
                                 log_gradients=False, cheat=False, seed=seed, lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01,
                                 env_alias="trans-boat")


def _metric():
    return _lib.SgkCrmdpMetric(_lib.CRMDP_METRIC_TRANS_BOAT, 5, 25)


def _device_filter(env, keys, rewards, lengths, n_agents, sentinel=True):
    """sgk_crmdp_filter on fresh device tables -> ({output: numpy}, {table: numpy})."""
    torch = _torch()
    dev = "cuda:%d" % env.device
    n, T = keys.shape
    memory = S.CRMDPMemory(n_agents, _metric(), dev)
    out = crmdp.filter_outputs(n, T, dev)
    if sentinel:
        for v in out.values():
            v.fill_(-7)
    crmdp.crmdp_filter(env, torch.tensor(keys).to(dev), torch.tensor(rewards).to(dev),
                       None if lengths is None else torch.tensor(lengths).to(dev), memory, out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in memory.fields().items()}


def _same(got, want, what):
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, np.argwhere(got[k] != want[k])[:5].tolist())


@pytest.fixture(scope="module")
def host():
    """sgk_crmdp_filter_host on the plans, once: with the six agents, and as one agent."""
    g = P.plans()
    six_t, one_t = P.fresh_tables(6), P.fresh_tables(1)
    six = P.filter_host(g["keys"], g["rewards"], g["lengths"], 6, six_t)
    one = P.filter_host(g["keys"], g["rewards"], g["lengths"], 1, one_t)
    return {6: (six, six_t), 1: (one, one_t)}


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_agents", [6, 1])
def test_the_device_filter_equals_the_host_call(host, n_agents):
    g = P.plans()
    env = S.BatchedGridworldEnv(BOAT, 48, seed=3)
    try:
        out, tables = _device_filter(env, g["keys"], g["rewards"], g["lengths"], n_agents)
        _same(out, host[n_agents][0], "outputs")
        _same(tables, host[n_agents][1], "tables")
        assert (out["n_corrupt"] > 0).any() and (out["unbounded"] > 0).any()
        # no lengths array: every trajectory t_max long (the plans' rows are zero-padded: key 0, reward 0)
        full, full_t = _device_filter(env, g["keys"], g["rewards"], None, n_agents)
        want_t = P.fresh_tables(n_agents)
        _same(full, P.filter_host(g["keys"], g["rewards"], None, n_agents, want_t), "outputs without lengths")
        _same(full_t, want_t, "tables without lengths")
        # an invalid key: the trajectory is copied, the others are served
        keys = g["keys"].copy()
        keys[9, 3], keys[20, 0] = 625, -1
        bad, bad_t = _device_filter(env, keys, g["rewards"], g["lengths"], n_agents)
        want_t = P.fresh_tables(n_agents)
        _same(bad, P.filter_host(keys, g["rewards"], g["lengths"], n_agents, want_t), "outputs with invalid keys")
        _same(bad_t, want_t, "tables with invalid keys")
        assert bad["n_corrupt"][9] == -1 and bad["n_corrupt"][20] == -1
    finally:
        env.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_second_pass_leaves_the_same_bytes(host, monkeypatch):
    g = P.plans()
    reps = 8
    monkeypatch.setenv("SGK_MAX_GRID", "64")
    env = S.BatchedGridworldEnv(BOAT, 48 * reps, seed=3)
    monkeypatch.delenv("SGK_MAX_GRID")
    try:
        keys, rewards, lengths = (np.concatenate([g[k]] * reps) for k in ("keys", "rewards", "lengths"))
        assert keys.shape[0] > 64 * 4  # more trajectories than the capped grid has waves
        out, tables = _device_filter(env, keys, rewards, lengths, 6 * reps)
        want, want_t = host[6]
        for r in range(reps):
            _same({k: v[48 * r:48 * (r + 1)] for k, v in out.items()}, want, "replica %d" % r)
            _same({k: v[6 * r:6 * (r + 1)] for k, v in tables.items()}, want_t, "tables of replica %d" % r)
    finally:
        env.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def _random_rollout(env, T, seed):
    """A real rollout under uniform random actions -> (states int8 [T, N, cells], the boards after the last step [N, cells], rewards)."""
    torch = _torch()
    dev = "cuda:%d" % env.device
    n = env.n_envs
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    last = torch.zeros((n, env.n_cells), dtype=torch.int8, device=dev)

    def policy(boards):
        return torch.randint(0, 4, (n,), generator=gen, device=dev).to(torch.uint8)

    def keep_last(e, buf):
        last.copy_(e.boards().reshape(n, -1))
        return buf["rewards"]

    rollout = batched_gather_rollout(policy, env, 0.99, horizon=T, filter_rewards=keep_last)
    return rollout.states, last, rollout.rewards


def _numpy_keys(states, last):
    boards = np.concatenate([states, last[None]])  # [T + 1, N, cells]
    found = (boards == 2).any(-1)
    cell = (boards == 2).argmax(-1)
    keys = cell[:-1] * boards.shape[-1] + cell[1:]
    keys[~(found[:-1] & found[1:])] = -1
    return np.ascontiguousarray(keys.T.astype(np.int32))


@pytest.mark.parametrize("n,T", [(130, 37), (64, 100), (5, 1)])
def test_the_keys_kernel_equals_numpy_argmax_on_a_real_rollout(n, T):
    torch = _torch()
    env = S.BatchedGridworldEnv(BOAT, n, seed=11)
    try:
        dev = "cuda:%d" % env.device
        states, last, _ = _random_rollout(env, T, seed=n)
        states = states.clone()
        if T > 2:
            states[2, n // 2].zero_()  # a board that shows no agent: the keys of steps 1 and 2 of that env are -1
        out = torch.full((n, T), -9, dtype=torch.int32, device=dev)
        crmdp.crmdp_keys(env, states, last, out)
        torch.cuda.synchronize()
        want = _numpy_keys(states.cpu().numpy(), last.cpu().numpy())
        got = out.cpu().numpy()
        assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5].tolist()
        assert len(np.unique(got[got >= 0])) > (1 if T == 1 else 4) and (got < 625).all()
        if T > 2:
            assert got[n // 2, 1] == -1 and got[n // 2, 2] == -1 and (got >= 0).sum() == got.size - 2
    finally:
        env.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_conv_learn", [False, True])
def test_the_batched_agent_filters_what_its_twin_gathers(fused_conv_learn):
    torch = _torch()
    n = 64
    env, twin_env = S.BatchedGridworldEnv(BOAT, n, seed=21), S.BatchedGridworldEnv(BOAT, n, seed=21)
    try:
        torch.manual_seed(7)
        agent = S.BatchedPPOCRMDPAgent(env, _args(n), on_unbounded="keep", fused_conv_learn=fused_conv_learn)
        torch.manual_seed(7)
        twin = S.BatchedPPOAgent(twin_env, _args(n), body="cnn", fused_conv_learn=fused_conv_learn)
        assert agent.body == "cnn" and agent.fused_learn == fused_conv_learn
        memory = R.Memory()
        for iteration in range(2):
            rollout, twin_rollout = agent.gather_rollout(), twin.gather_rollout()
            torch.cuda.synchronize()
            for name in ("states", "actions", "recs", "lengths"):
                assert agent._buffers[name].cpu().numpy().tobytes() == twin._buffers[name].cpu().numpy().tobytes(), (iteration, name)
            raw = agent._buffers["rewards"].cpu().numpy()
            assert raw.tobytes() == twin_rollout.rewards.cpu().numpy().tobytes()
            c = {k: v.cpu().numpy() for k, v in agent.crmdp.items()}
            assert rollout.rewards.data_ptr() == agent.crmdp["rewards_out"].data_ptr()
            keys = _numpy_keys(agent._buffers["states"].cpu().numpy(), c["last_boards"])
            assert c["keys"].tobytes() == keys.tobytes() and (keys >= 0).all()
            replaced = 0
            for e in range(n):  # env order is the reference's rollout order
                order, safe, modified = memory.filter(keys[e], raw[e])
                want = np.array([r if v is None else v for v, r in zip(modified, raw[e])], np.float32)
                assert c["rewards_out"][e].tobytes() == want.tobytes(), (iteration, e)
                assert c["order"][e, :len(order)].tolist() == order and c["n_corrupt"][e] == len(order) and c["safe_index"][e] == safe
                assert c["unbounded"][e] == sum(v is None for v in modified)
                replaced += int((want != raw[e]).sum())
            flag, reward, rllb = memory.tables()
            assert agent.memory.flag.cpu().numpy()[0].tobytes() == flag.tobytes()
            assert agent.memory.reward.cpu().numpy()[0].tobytes() == reward.tobytes()
            assert agent.memory.bound.cpu().numpy()[0].tobytes() == rllb.tobytes()
            stats = agent.stats()
            assert stats["corrupt_states"] == int((flag == R.CORRUPT).sum()) and stats["replaced_rewards"] == replaced
            assert agent.memory.states() == {divmod(k, 25): (ok, r) for k, (ok, r) in memory.states.items()}
            assert agent.memory.rllb() == {divmod(k, 25): b for k, b in memory.rllb.items() if b is not None}
            # BoatRace's own rewards: the clockwise arrow entries are what gets marked (random early policies find some of them)
            assert stats["corrupt_states"] >= 1 and replaced >= 1, stats
            want_returns = env.discounted_returns(agent.crmdp["rewards_out"], 0.99, lengths=agent._buffers["lengths"])
            assert rollout.returns.cpu().numpy().tobytes() == want_returns.cpu().numpy().tobytes()
            assert rollout.returns.cpu().numpy().tobytes() != twin_rollout.returns.cpu().numpy().tobytes()
        # (no learn() between the two gathers: the twin learns from other returns, so its policy would part from the agent's)
        before = [p.detach().clone() for p in agent.net.parameters()]
        agent.learn(rollout)
        agent.sync()
        torch.cuda.synchronize()
        after = list(agent.net.parameters())
        assert all(bool(torch.isfinite(p).all()) for p in after) and any(not torch.equal(a, b) for a, b in zip(after, before))
    finally:
        env.close()
        twin_env.close()


def test_an_unbounded_state_stops_the_batched_agent_unless_told_to_keep():
    """A memory that holds one corrupt key and no safe one: sgk_crmdp_filter leaves `unbounded` set, stats() names the trajectory."""
    torch = _torch()
    env = S.BatchedGridworldEnv(BOAT, 8, seed=2)
    try:
        torch.manual_seed(1)
        agent = S.BatchedPPOCRMDPAgent(env, _args(8))
        assert agent.stats() == {"corrupt_states": 0, "replaced_rewards": 0, "first_unbounded": -1}
        agent.memory.flag.fill_(_lib.CRMDP_CORRUPT)  # every key corrupt, none safe, no bound: the first trajectory is unbounded
        agent.gather_rollout(horizon=6)
        with pytest.raises(RuntimeError, match="trajectory 0 has a corrupt state without a reward bound"):
            agent.stats()
        agent.on_unbounded = "keep"
        assert agent.stats()["first_unbounded"] == 0
        with pytest.raises(ValueError, match="purge"):
            agent.gather_rollout(horizon=1)
        with pytest.raises(KeyError):
            S.BatchedPPOCRMDPAgent(env, types.SimpleNamespace(**{**vars(_args(8)), "env_alias": "boat"}))
    finally:
        env.close()
    island = S.BatchedGridworldEnv("IslandNavigation-v0", 8, seed=2)
    try:
        with pytest.raises(KeyError, match="metric of BoatRace-v0 only"):
            S.BatchedPPOCRMDPAgent(island, _args(8))
    finally:
        island.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_the_buffers_stay_inside_their_guard_bands(host, pattern):
    """Every pointer of sgk_crmdp_buffers -- keys, rewards_out, order, n_corrupt, safe_index, unbounded, mem_flag, mem_reward, mem_rllb --
    carved from a guard_arena.Arena under both patterns; the rollout's states, the last boards, the rewards and the lengths are frozen
    inputs. 130 envs x 37 steps for the keys (a partial tile), the plans (48 x 100, rows of different lengths) for the filter. After
    the calls: no guard byte and no input byte changed, no output entry still holds the pattern, the bytes equal the plain calls'."""
    torch = _torch()
    g = P.plans()
    env = S.BatchedGridworldEnv(BOAT, 130, seed=11)
    try:
        dev = "cuda:%d" % env.device
        states, last, _ = _random_rollout(env, 37, seed=130)
        arena = GA.Arena(dev, pattern, 1 << 21)
        a_states, a_last = arena.adopt("states", states), arena.adopt("last_boards", last)
        a_keys_in = arena.adopt("keys_in", torch.tensor(g["keys"]))
        a_rewards = arena.adopt("rewards", torch.tensor(g["rewards"]))
        a_lengths = arena.adopt("lengths", torch.tensor(g["lengths"]))
        for name in ("states", "last_boards", "keys_in", "rewards", "lengths"):
            arena.freeze(name)
        keys = arena.carve("keys", (130, 37), torch.int32)
        out = {"rewards_out": arena.carve("rewards_out", (48, 100), torch.float32), "order": arena.carve("order", (48, 100), torch.int32),
               "n_corrupt": arena.carve("n_corrupt", (48,), torch.int32), "safe_index": arena.carve("safe_index", (48,), torch.int32),
               "unbounded": arena.carve("unbounded", (48,), torch.int32)}
        memory = S.CRMDPMemory(6, _metric(), dev)
        memory.flag = arena.adopt("mem_flag", memory.flag)
        memory.reward = arena.adopt("mem_reward", memory.reward)
        memory.bound = arena.adopt("mem_rllb", memory.bound)
        assert arena.layout_ok() and arena.check() == []
        crmdp.crmdp_keys(env, a_states, a_last, keys)
        crmdp.crmdp_filter(env, a_keys_in, a_rewards, a_lengths, memory, out)
        torch.cuda.synchronize()
        assert arena.check() == []
        for name in ("keys",) + tuple(out):
            assert arena.unwritten(name) == 0, name
        assert keys.cpu().numpy().tobytes() == _numpy_keys(states.cpu().numpy(), last.cpu().numpy()).tobytes()
        _same({k: v.cpu().numpy() for k, v in out.items()}, host[6][0], "outputs")
        _same({k: v.cpu().numpy() for k, v in memory.fields().items()}, host[6][1], "tables")
    finally:
        env.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_keys_and_filter_replay_from_a_graph_to_the_same_bytes():
    torch = _torch()
    n, T = 130, 37
    env = S.BatchedGridworldEnv(BOAT, n, seed=11)
    try:
        dev = "cuda:%d" % env.device
        states, last, rewards = _random_rollout(env, T, seed=n)
        rewards = rewards.clone()
        rewards[::7, 5] = 60.0  # outliers: something to mark whatever the walk found
        keys = torch.zeros((n, T), dtype=torch.int32, device=dev)
        out = crmdp.filter_outputs(n, T, dev)
        memory = S.CRMDPMemory(2, _metric(), dev)

        def run():
            crmdp.crmdp_keys(env, states, last, keys)
            crmdp.crmdp_filter(env, keys, rewards, None, memory, out)

        run()  # eagerly, twice: the memory carries over
        run()
        torch.cuda.synchronize()
        want = {k: v.clone() for k, v in {**out, **memory.fields(), "keys": keys}.items()}
        assert int((want["n_corrupt"] > 0).sum()) >= 1
        for t in list(out.values()) + [keys]:
            t.fill_(-5)
        memory.flag.zero_(), memory.reward.zero_(), memory.bound.fill_(_lib.CRMDP_NONE)
        cur, following = torch.cuda.current_stream(dev), env._mode == "follow"
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph):
            env.bind_torch_stream(torch.cuda.current_stream(dev))  # the capture stream
            run()
        env.bind_torch_stream(None if following else cur)
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        for k, v in {**out, **memory.fields(), "keys": keys}.items():
            assert v.cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    finally:
        env.close()


# ---- the batched trainer ----------------------------------------------------------------------------------------------------------------
def test_the_batched_trainer_runs_ppo_crmdp_and_writes_its_two_scalars():
    _torch()
    argv = ["-N", "16", "-S", "3", "-E", "2", "-EE", "5", "-V", "10", "-EV", "0", "trans-boat", "ppo-crmdp", "-l", "0.001", "-r", "16", "-e", "2",
            "-b", "16"]
    writers = []

    def writer_factory(log_dir):
        writers.append(S.RecordingWriter(log_dir))
        return writers[-1]

    agent, env = S.train_batched(S.prepare_parser().parse_args(argv), writer_factory=writer_factory)
    try:
        assert isinstance(agent, S.BatchedPPOCRMDPAgent) and agent.on_unbounded == "raise"
        calls = [c for c in writers[0].calls if c[0] == "scalar"]
        for tag in ("Train/crmdp_corrupt_states", "Train/crmdp_replaced_rewards"):
            got = [(c[2], c[3]) for c in calls if c[1] == tag]
            assert [step for _, step in got] == [1, 2] and all(isinstance(v, int) and v >= 0 for v, _ in got), (tag, got)
        corrupt = [c[2] for c in calls if c[1] == "Train/crmdp_corrupt_states"]
        assert corrupt[-1] == agent.memory.n_corrupt() >= corrupt[0] >= 1  # corrupt marks are never taken back
        assert any(c[1] == "Train/policy_loss" for c in calls)
    finally:
        env.close()
    # the population flags keep their refusals
    for core in (["--members", "2"], ["--members", "2", "--sweep", "lr=1e-3,1e-2"]):
        with pytest.raises(SystemExit, match="ppo-mlp, ppo-cnn or deep-q agents, not 'ppo-crmdp'"):
            S.train_batched(S.prepare_parser().parse_args(core + argv))
