"""sgk_tabq_eval -- default_eval (reference eval.py:8-56) for the batched tabular-Q agents in ONE launch -- against what it fuses:
loops.batched_default_eval's loop of {sgk_tabq_act(explore = 0), sgk_step, sgk_reset_done} calls (fused_eval = False, the path every
earlier test of the evaluation went through). Bit for bit, on every level, through both kernels (each agent's greedy policy in a
register word / a row gather per state change), from reset states and from arbitrary ones; against the reference's own evaluation
fixtures; recorded in a graph; and with a hash table that fills up while evaluating."""
import types

import numpy as np
import pytest

import batched_golden as BG
import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib

pytestmark = pytest.mark.gpu

LEVELS = sorted(S.envs.ENV_IDS)
KERNELS = {"auto": _lib.TABQ_KERNEL_AUTO, "lds": _lib.TABQ_KERNEL_LDS, "hbm": _lib.TABQ_KERNEL_HBM}
HASH_TRAIN_STEPS = 50  # TomatoWatering, 64-slot tables: learning steps that leave room in every agent's table (at most one new board per step)
N = 1061  # neither a multiple of 64 (the wave of the policy-in-registers kernel) nor of 256 (the workgroup of the other)


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _args(**kw):
    d = dict(lr=0.4, discount=0.95, epsilon=0.15, epsilon_anneal=400)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _pair(name, n=N, seed=77, **kw):
    """Two identically seeded (env, agent) pairs; TomatoWatering with hash tables the training steps of these tests do not fill."""
    if name == "TomatoWatering-v0":
        kw.setdefault("hash_capacity", 1024)
    out = []
    for _ in range(2):
        env = S.BatchedGridworldEnv(name, n, seed=seed, env_index_base=4321)
        out.append((env, S.BatchedTabularQAgent(env, _args(**kw))))
    return out


def _close(pair):
    for env, agent in pair:
        agent.close(); env.close()


def _snapshot(env, agent):
    info = _lib.SgkInfo()
    _lib.check(env.lib.sgk_get_info(env.handle, info))
    metrics = env.metrics().copy()  # (16 words; SGK_M_STEPS is the handle's steps_issued)
    snap = {"metrics": metrics, "steps_issued": metrics[_lib.M_STEPS:_lib.M_STEPS + 1].copy(),
            "boards": env.boards_host().copy(), "rec": env.step_records_host().copy(),
            "lockstep_t": np.array([info.lockstep_t]), "agent_t": np.array([agent.t]),
            "table": agent.table_host().view(np.uint64).copy()}  # (f64 bit patterns: -0.0 != 0.0, a NaN equals itself)
    snap.update({k: v.copy() for k, v in env.episode_state_host().items()})
    snap.update({k: v.copy() for k, v in env.last_episode_host().items()})
    if env.name == "FriendFoe-v0":
        snap["bandit"] = env.bandit_policy().view(np.uint64).copy()
    if env.name == "TomatoWatering-v0":
        snap["keys"] = agent.keys_host().copy()
        snap["hash_info"] = np.array(agent.hash_info(), dtype=np.int64)
    return snap


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        assert (a[k] == b[k]).all(), (what, k, np.argwhere(np.atleast_1d(a[k] != b[k]))[:4].tolist())


def _loop_of_calls(agent, env, eval_timesteps):
    """What the fused call replaces, through the public loop: fused_eval = False. reads_boards makes the loop's env.step calls write
    the boards (a table agent's loop leaves them out; the fused call materialises those of the final states): the boards the loop of
    calls leaves when it writes them."""
    agent.fused_eval = False
    agent.reads_boards = True
    return S.batched_default_eval(agent, env, eval_timesteps)


def _evaluate_or_skip(agent, eval_timesteps, kernel):
    try:
        return agent.evaluate(eval_timesteps, kernel=kernel)
    except _lib.SgkError as exc:
        assert kernel == "lds" and "do not fit LDS" in str(exc)
        pytest.skip("%s: tables do not fit LDS" % agent.env.name)


# ---- 1. bit-exactness against the loop of calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["auto", "lds", "hbm"])
@pytest.mark.parametrize("eval_timesteps", [1, 2, 37, 250])
@pytest.mark.parametrize("name", LEVELS)
def test_fused_evaluation_equals_the_loop_of_calls(name, eval_timesteps, kernel):
    _torch()
    pair = _pair(name)
    (e0, a0), (e1, a1) = pair
    try:
        a0.rollout(700); a1.rollout(700)
        t_before, table_before = a1.t, a1.table_host().view(np.uint64).copy()
        m0 = _loop_of_calls(a0, e0, eval_timesteps)
        if kernel == "auto":  # through the public loop: it hands the evaluation to agent.evaluate()
            assert a1.fused_eval
            m1 = S.batched_default_eval(a1, e1, eval_timesteps)
        else:
            m1 = _evaluate_or_skip(a1, eval_timesteps, kernel)
        steps = max(eval_timesteps - 1, 0) + e1.info.max_iterations
        assert m1.vec == m0.vec and m1.episodes >= N and m1.steps == N * steps
        s0, s1 = _snapshot(e0, a0), _snapshot(e1, a1)
        _same(s0, s1, "after the evaluation")
        assert s1["over"].all()  # the tail ran every episode to its end
        assert a1.t == t_before == 700
        if name != "TomatoWatering-v0":  # (there greedy act() claims slots for boards it has not seen: rows of zeros, keys compared above)
            assert (s1["table"] == table_before).all()
        # nothing stale is left behind: both go on learning to the same tables (from reset envs: a rollout leaves an env that is
        # over alone, and after the evaluation's tail all of them are)
        e0.reset(); e1.reset()
        a0.rollout(300); a1.rollout(300)
        assert not (a1.table_host().view(np.uint64) == table_before).all()
        _same(_snapshot(e0, a0), _snapshot(e1, a1), "after 300 more learning steps")
        # ... and through the per-step kernels, whose kept rows the evaluation must have invalidated
        for env, agent in pair:
            for _ in range(5):
                agent.step()
        _same(_snapshot(e0, a0), _snapshot(e1, a1), "after 5 per-step launches")
    finally:
        _close(pair)


# ---- 2. entry from an arbitrary state -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(0, 1), (1, 0), (3, 0), (0, 40), (23, 130)], ids=lambda c: "%d+%d" % c)
@pytest.mark.parametrize("kernel", ["auto", "hbm"])
@pytest.mark.parametrize("name,k", [("IslandNavigation-v0", 12), ("SideEffectsSokoban-v0", 80)])
def test_the_c_call_from_an_arbitrary_state_equals_the_per_step_calls(name, k, kernel, counts):
    """Some envs over (they idle; in the reset phase they are reset BEHIND the first step), some in the middle of an episode."""
    _torch()
    n_reset, n_tail = counts
    pair = _pair(name)
    (e0, a0), (e1, a1) = pair
    try:
        for env, agent in pair:
            agent.rollout(300)
            env.step_random(k, auto_reset=False)
        over = e1.episode_state_host()["over"]
        assert 0 < int(over.sum()) < N, int(over.sum())
        for i in range(n_reset + n_tail):
            e0.step(a0.act(), auto_reset=False)
            if i < n_reset:
                e0.reset_done()
        e1._follow()
        _lib.check(e1.lib.sgk_tabq_eval(a1._h, n_reset, n_tail, KERNELS[kernel]))
        s0, s1 = _snapshot(e0, a0), _snapshot(e1, a1)
        _same(s0, s1, "%s %s %r" % (name, kernel, counts))
        assert s1["lockstep_t"][0] == 300 + k + n_reset + n_tail
        assert s1["steps_issued"][0] == N * (300 + k + n_reset + n_tail)  # (no metrics_reset since the envs were made)
        a0.rollout(100); a1.rollout(100)
        _same(_snapshot(e0, a0), _snapshot(e1, a1), "after 100 more learning steps")
    finally:
        _close(pair)


def test_argument_errors_and_the_empty_call():
    _torch()
    env = S.BatchedGridworldEnv("SideEffectsSokoban-v0", 256, seed=3)
    agent = S.BatchedTabularQAgent(env, _args())
    lib = env.lib
    try:
        agent.rollout(50)
        before = _snapshot(env, agent)
        assert lib.sgk_tabq_eval(agent._h, 0, 0, _lib.TABQ_KERNEL_AUTO) == 0  # nothing to do: nothing done
        _same(before, _snapshot(env, agent), "empty call")
        for call, word in [((None, 1, 1, 0), b"NULL"), ((agent._h, -1, 1, 0), b"n_reset_steps"), ((agent._h, 1, -1, 0), b"n_tail_steps"),
                           ((agent._h, 1, 1, 3), b"kernel"), ((agent._h, 1, 1, _lib.TABQ_KERNEL_LDS), b"do not fit LDS")]:
            assert lib.sgk_tabq_eval(*call) == _lib.ERR_INVALID, call
            assert word in lib.sgk_last_error(), (call, lib.sgk_last_error())
        _same(before, _snapshot(env, agent), "refused calls")
        with pytest.raises(_lib.SgkError):
            agent.evaluate(5, kernel="lds")
    finally:
        agent.close(); env.close()


# ---- 3. the reference's own evaluations -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["auto", "hbm"])
@pytest.mark.parametrize("name", BG.TABQ_FIXTURES)
def test_fused_evaluation_reproduces_the_reference_default_eval(name, kernel):
    """default_eval (eval.py:8-56) of every reference agent after the fixture's training steps: every episode's return and
    performance as its track_metrics calls saw them, aggregated like the metrics vector."""
    from oracle import oracle as O

    _torch()
    fx = BG.TabqFixture(name)
    env = S.BatchedGridworldEnv(fx.env, fx.n, seed=fx.seed)
    agent = S.BatchedTabularQAgent(env, fx.args())
    try:
        agent.rollout(fx.steps, cheat=fx.cheat)
        bm = agent.evaluate(fx.eval_timesteps, kernel=kernel)
        BG.assert_eval_metrics(bm.vec, fx, O)
        assert bm.episodes == sum(len(a["eval_episodes"]) for a in fx.agents)
    finally:
        agent.close(); env.close()


def test_the_cell_state_levels_take_the_policy_in_registers_kernel():
    """BoatRace, IslandNavigation and DistributionalShift qualify for the on-chip kernel (no skip in the tests above); a level whose
    table state is more than the agent's cell does not."""
    _torch()
    for name, ok in [("BoatRace-v0", True), ("IslandNavigation-v0", True), ("DistributionalShift-v0", True),
                     ("SideEffectsSokoban-v0", False), ("TomatoWatering-v0", False)]:
        env = S.BatchedGridworldEnv(name, 100, seed=1)
        agent = S.BatchedTabularQAgent(env, _args())
        try:
            rc = env.lib.sgk_tabq_eval(agent._h, 2, 3, _lib.TABQ_KERNEL_LDS)
            assert (rc == 0) == ok, name
        finally:
            agent.close(); env.close()


# ---- 4. graph capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["IslandNavigation-v0", "SideEffectsSokoban-v0"])
def test_the_evaluation_is_capturable(name):
    """agent.evaluate's call sequence (metrics_reset, reset, sgk_tabq_eval) recorded in a torch.cuda.graph and replayed from another
    state gives the eager call's metrics and final state."""
    torch = _torch()
    eval_timesteps = 120
    env = S.BatchedGridworldEnv(name, N, seed=11)
    agent = S.BatchedTabularQAgent(env, _args())
    try:
        agent.rollout(700)
        steps = eval_timesteps - 1 + env.info.max_iterations
        want = agent.evaluate(eval_timesteps)
        assert want.episodes >= N
        eager = _snapshot(env, agent)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            agent.evaluate_enqueue(eval_timesteps)
        env.account_steps(-steps)  # the recorded (not executed) call bumped the host-side counters once
        # somewhere else entirely: random steps from the final states, other metrics
        env.step_random(13, auto_reset=True)
        assert env.metrics().tolist() != want.vec
        env.account_steps(-13)
        env.metrics_reset()  # (the host-side half of the recorded metrics_reset: the step count)
        graph.replay()
        env.account_steps(steps)
        torch.cuda.synchronize()
        assert env.metrics().tolist() == want.vec
        got = _snapshot(env, agent)
        for snap in (eager, got):
            del snap["lockstep_t"]  # (the handle's step accounting lives on the host: a replay does not move it, account_steps does)
            del snap["n_episodes"]  # (counts every episode since the env was made: the replay's come on top of the eager call's)
        _same(eager, got, "replayed")
    finally:
        agent.close(); env.close()


# ---- 5. a hash table that fills up during the evaluation ------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["auto", "hbm"])
def test_a_hash_table_that_overflows_during_the_evaluation(kernel):
    """TomatoWatering with 64-slot tables: greedy act() claims a slot for every new board until the table is full; from then on a
    board that is not in it reads as zeros and the overflow flag is up -- the same slots, the same flag, the same episodes as the
    per-step path."""
    _torch()
    pair = _pair("TomatoWatering-v0", hash_capacity=64)
    (e0, a0), (e1, a1) = pair
    try:
        a0.rollout(HASH_TRAIN_STEPS); a1.rollout(HASH_TRAIN_STEPS)
        cap, used, overflowed = a1.hash_info()
        assert cap == 64 and not overflowed, (cap, used, overflowed)  # the training steps leave room ...
        m0 = _loop_of_calls(a0, e0, 250)
        m1 = a1.evaluate(250, kernel=kernel)
        assert a0.hash_info() == (64, 64, True)  # ... which the evaluation uses up
        assert a1.hash_info() == (64, 64, True)
        assert m1.vec == m0.vec
        _same(_snapshot(e0, a0), _snapshot(e1, a1), "after the evaluation")
    finally:
        _close(pair)

