"""Guard bands: no call of libsgk.so writes outside the buffers it is given.

Every tensor a case hands to the library is carved out of ONE pattern-filled allocation (tests/guard_arena.py): 256-byte aligned, with
max(4096, one outermost slice) guard bytes on each side, so a store in front of a buffer, behind it, or one step / ring slice / member /
row too far lands on the pattern instead of in the caching allocator's slack. Every case runs under both patterns ("p" and its bytewise
complement: a stray byte cannot equal both) and asserts

1. arena.check() == [] after a synchronize -- no guard byte and no byte of a frozen input changed (and the layout facts: every view
   has its own full guard inside the allocation, clear of every other view);
2. the carved outputs hold, as bytes, what a TWIN handle (same level, n, seed, env_index_base, the same calls before) leaves when it
   makes the same call on ordinary exact-size tensors, and the handle state the call touches is equal too -- the twin ties the case to
   the references the other test files pin; it is no reference of its own;
3. no carved output that the call writes completely still holds pattern (Arena.unwritten): the work was done in the arena.

All comparisons are exact. Under -s every case prints one line (case id, tensors carved, guard bytes checked, stray bytes found,
seconds): profiles/guard_bands/results.log. profiles/guard_bands/mutations.log: three mutations of the library against this file.

COVERED / EXEMPT (below) place every pointer include/sgk.h lets the library write through; tests/test_guard_arena_cpu.py holds the two
tables against the header.
"""
import ctypes
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "safe-grid-agents_amd")):  # (run as a script: see the last lines)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import guard_arena as GA  # noqa: E402
import safe_grid_agents_amd as S  # noqa: E402
from safe_grid_agents_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERNS = GA.PATTERNS
BOAT, SOKOBAN = "BoatRace-v0", "SideEffectsSokoban-v0"
CELL_LEVEL = {25: BOAT, 30: "FriendFoe-v0", 36: SOKOBAN, 63: "DistributionalShift-v0"}  # K0 -> a level with such boards
I64_MIN = -(2 ** 63)


# ---- what is covered where, and what is not ----------------------------------------------------------------------------------------------
def _keys(fn, *params):
    return ["%s.%s" % (fn, p) for p in params]


def _table(*groups):
    out = {}
    for keys, value in groups:
        for k in keys:
            assert k not in out, k
            out[k] = value
    return out


_ROLLOUT_OUTS = ("states_out_dev", "actions_out_dev", "recs_out_dev")
COVERED = _table(
    (_keys("sgk_obs_f32", "dst_dev") + _keys("sgk_render_rgb", "rgb_dev"), ["test_per_step_observations"]),
    (_keys("sgk_epsilon_greedy", "actions_out_dev") + _keys("sgk_epsilon_greedy_ex", "actions_out_dev")
     + _keys("sgk_categorical_sample", "actions_out_dev"), ["test_per_step_draws"]),
    (_keys("sgk_policy_act", "actions_out_dev", "scores_out_dev") + _keys("sgk_policy_sample", "actions_out_dev", "logits_out_dev")
     + _keys("sgk_convq_act", "actions_out_dev", "scores_out_dev") + _keys("sgk_convq_sample", "actions_out_dev", "logits_out_dev"),
     ["test_acting_forwards"]),
    (_keys("sgk_tabq_act", "actions_out_dev") + _keys("sgk_tabq_step", "actions_out_dev"), ["test_tabq_actions"]),
    (_keys("sgk_finished", "ids_dev", "return_dev", "performance_dev"), ["test_finished"]),
    (_keys("sgk_step_store", "successors_ring", "actions_ring", "rewards_ring", "terminals_ring")
     + _keys("sgk_reset_done_store", "states_ring")
     + _keys("sgk_replay_store", "states_ring", "successors_ring", "actions_ring", "rewards_ring", "terminals_ring"), ["test_replay_rings"]),
    (_keys("sgk_dqn_sgd_step_reset_store", "states_ring"), ["test_dqn_reset_store_rings", "test_dqn_learner"]),
    (_keys("sgk_discounted_returns", "returns_dev") + _keys("sgk_discounted_returns_members", "returns_dev"), ["test_discounted_returns"]),
    (_keys("sgk_policy_rollout", *_ROLLOUT_OUTS) + _keys("sgk_convq_rollout", *_ROLLOUT_OUTS)
     + _keys("sgk_policy_rollout_members", *_ROLLOUT_OUTS, "member_metrics_dev")
     + _keys("sgk_policy_rollout_members_eps", *_ROLLOUT_OUTS, "member_metrics_dev")
     + _keys("sgk_convq_rollout_members", *_ROLLOUT_OUTS, "member_metrics_dev"), ["test_rollouts"]),
    (_keys("sgk_policy_act_members_all", "member_actions_out_dev", "member_scores_out_dev")
     + _keys("sgk_members_vote", "actions_out_dev", "votes_out_dev", "dissent_dev"), ["test_ensemble"]),
    (_keys("sgk_tabq_consensus", "votes_out_dev", "voters_out_dev"), ["test_tabq_consensus"]),
    (_keys("sgk_members_select", "src_out_dev") + _keys("sgk_members_explore", "hyper_dev", "generation_dev"), ["test_members_select"]),
    (_keys("sgk_dqn_learner", "w1", "b1", "w2", "b2", "w3", "b3", "w1t", "w2t", "w3t", "m", "v", "vmax", "step", "loss_out", "rows_out"),
     ["test_dqn_learner", "test_dqn_learner_members", "test_dqn_one_launch_adam"]),
    (_keys("sgk_dqn_sgd_step_members", "workspace") + _keys("sgk_dqn_sgd_step_members_hyper", "workspace"), ["test_dqn_learner_members"]),
    (_keys("sgk_ppo_learner", "w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc", "w1t", "w2t", "m", "v", "step", "stats_out", "rows_out"),
     ["test_ppo_learner", "test_ppo_learner_members"]),
    (_keys("sgk_ppo_cnn_learner", "params", "m", "v", "step", "stats_out", "rows_out", "workspace"),
     ["test_ppo_cnn_learner", "test_ppo_cnn_learner_members"]),
    # sgk_members_clone: another file's tests ("module.test"), which put guard rows around every cloned tensor and read the status word back
    (_keys("sgk_members_clone", "status_dev") + _keys("sgk_members_tensor", "base"),
     ["test_gpu_pbt.test_clone_copies_the_sources_slabs_and_nothing_else",
      "test_gpu_pbt.test_clone_refuses_a_source_that_is_a_destination_and_serves_the_others"]),
)

_HOST = "host memory: the library writes it with a host store or a synchronising copy of the documented size, no kernel"
_OUT = "out-param in host memory that receives one handle, device pointer or scalar"
_STREAM = "a hipStream_t passed by value: nothing is stored through it"
_RCCL = "the multi-GPU communicator (RCCL): out of scope for the guard bands, tests/test_dist_gloo.py and the multi-chip runs hold it"
_DEBUG = "sgk_debug_* test hook on host memory, never on a product path"
_TRAJ = "trajectory ring: left to its two guard tests in tests/test_gpu_parity.py (64-byte block right behind the ring)"
EXEMPT = _table(
    (_keys("sgk_device_count", "n_out") + _keys("sgk_get_info", "out") + _keys("sgk_reward_scale", "scale_out")
     + _keys("sgk_tabq_global_step", "t_out") + _keys("sgk_tabq_hash_info", "capacity_out", "max_used_out", "overflowed_out")
     + _keys("sgk_issue_peak", "valu_wave_instr_per_s", "salu_wave_instr_per_s") + _keys("sgk_ring_probe", "us_per_slice")
     + _keys("sgk_finished", "n_host"), _HOST),
    (_keys("sgk_create", "out") + _keys("sgk_create_ex", "out") + _keys("sgk_tabq_create", "out") + _keys("sgk_tabq_create_ex", "out")
     + _keys("sgk_ring_alloc", "dev_ptr") + _keys("sgk_boards_dev", "boards_dev", "pitch") + _keys("sgk_step_records_dev", "rec_dev")
     + _keys("sgk_metrics_dev", "metrics_dev") + _keys("sgk_episode_arrays_dev", "last_return_dev", "last_performance_dev", "n_episodes_dev")
     + _keys("sgk_tabq_table_dev", "table_dev", "n_states", "n_actions"), _OUT),
    (_keys("sgk_set_stream", "hip_stream") + _keys("sgk_stream_wait", "other_stream") + _keys("sgk_stream_signal", "other_stream"), _STREAM),
    (_keys("sgk_ring_free", "dev_ptr"), "the allocation is released, not written"),
    (_keys("sgk_step_host", "rec_host", "boards_host", "episode_return_host") + _keys("sgk_copy_boards", "boards_host")
     + _keys("sgk_copy_step_records", "rec_host")
     + _keys("sgk_copy_episode_state", "episode_return_host", "hidden_return_host", "frame_host", "over_host", "agent_cell_host", "box_cell_host")
     + _keys("sgk_copy_last_episode", "last_return_host", "last_performance_host", "n_episodes_host") + _keys("sgk_metrics", "out_host")
     + _keys("sgk_copy_bandit_policy", "out_host") + _keys("sgk_tabq_copy_keys", "keys_host") + _keys("sgk_tabq_copy_table", "table_host")
     + _keys("sgk_tabq_consensus_host", "votes_out_host", "voters_out_host") + _keys("sgk_discount_powers", "out_host")
     + _keys("sgk_members_vote_host", "actions_out", "votes_out", "dissent") + _keys("sgk_members_select_host", "src_out"), _HOST),
    (_keys("sgk_rollout_random_stream", "boards_ring_dev", "recs_ring_dev") + _keys("sgk_ring_probe", "boards_ring_dev", "recs_ring_dev"), _TRAJ),
    (_keys("sgk_comm_available", "version_out") + _keys("sgk_comm_unique_id", "id_out") + _keys("sgk_comm_create", "out")
     + _keys("sgk_comm_info", "rank_out", "world_out", "device_out") + _keys("sgk_allreduce_metrics", "inout_dev", "hip_stream")
     + _keys("sgk_metrics_allreduced", "out_host"), _RCCL),
    (_keys("sgk_debug_host_transition", "out") + _keys("sgk_debug_host_step", "state_word_out", "out", "aux_env")
     + _keys("sgk_debug_level", "dims", "templ", "agent_value") + _keys("sgk_debug_graph_count", "env_graphs_out", "tabq_graphs_out")
     + _keys("sgk_debug_launch_grids", "out"), _DEBUG),
)


# ---- the harness -------------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class _ArenaAlloc:
    """A case's tensors out of the arena. out(): the call writes it (fill=None: every entry -- the view keeps the pattern until then);
    state(): read and updated in place (parameters, moments, accumulated counters); inp(): only read, frozen."""

    def __init__(self, arena):
        self.arena, self.outs, self.full = arena, {}, []

    def out(self, name, shape, dtype, fill=None, outer=None):
        t = self.arena.carve(name, shape, dtype, fill=fill, outer=outer)
        self.outs[name] = t
        if fill is None:
            self.full.append(name)
        return t

    def state(self, name, tensor, outer=None):
        t = self.arena.adopt(name, tensor, outer=outer)
        self.outs[name] = t
        return t

    def scratch(self, name, nbytes, outer=None):
        """A workspace: sized exactly, guarded, its contents mean nothing (not compared with the twin's)."""
        torch = _torch()
        return self.arena.carve(name, (int(nbytes),), torch.uint8, outer=outer)

    def inp(self, name, tensor, outer=None):
        t = self.arena.adopt(name, tensor, outer=outer)
        self.arena.freeze(name)
        return t


class _PlainAlloc:
    """The twin's: ordinary exact-size torch tensors."""

    def __init__(self, device):
        self.device, self.outs, self.keep = device, {}, []  # (keep: what only a raw pointer in a struct would otherwise hold)

    def out(self, name, shape, dtype, fill=None, outer=None):
        torch = _torch()
        t = torch.full(tuple(shape), 0 if fill is None else fill, dtype=dtype, device=self.device)
        self.outs[name] = t
        return t

    def state(self, name, tensor, outer=None):
        t = tensor.detach().to(self.device).clone()
        self.outs[name] = t
        return t

    def scratch(self, name, nbytes, outer=None):
        torch = _torch()
        self.keep.append(torch.zeros(int(nbytes), dtype=torch.uint8, device=self.device))
        return self.keep[-1]

    def inp(self, name, tensor, outer=None):
        self.keep.append(tensor.detach().to(self.device).clone())
        return self.keep[-1]


def _handle_state(env):
    """Everything a call can leave in the handle: boards, last step records, the decoded state words, the episode arrays, the metrics."""
    v = env._device_views()
    out = {"boards": env.boards_host(), "records": env.step_records_host(), "metrics": env.metrics(), "lockstep_t": np.int64(env.lockstep_t)}
    out.update({"word " + k: a for k, a in env.episode_state_host().items()})
    out.update({k: v[k].cpu().numpy() for k in ("last_return", "last_performance", "n_episodes")})
    return out


def _bytes(t):
    torch = _torch()
    return t.detach().contiguous().view(-1).view(torch.uint8) if t.numel() else t.detach().reshape(0).view(torch.uint8)


def check_case(case_id, pattern, make_env, body, arena_bytes=4 << 20):
    """Run `body(env, alloc)` on a fresh handle with arena tensors and on its twin with plain ones; print the log line; assert 1-3.
    body returns a dict of host arrays to compare besides the carved outputs and the handle state (or None). Returns the log record."""
    torch = _torch()
    t0 = time.perf_counter()
    env, twin = make_env(), make_env()
    try:
        dev = "cuda:%d" % env.device
        arena = GA.Arena(dev, pattern, arena_bytes)
        A, P = _ArenaAlloc(arena), _PlainAlloc(dev)
        extra_a, failed = {}, None
        try:
            extra_a = body(env, A) or {}
        except AssertionError as exc:  # (the guards are read all the same: where a wrong result came from is what the log line is for)
            failed = exc
        torch.cuda.synchronize()
        stray = arena.check()
        layout_ok = arena.layout_ok()
        rec = {"case": case_id, "pattern": pattern, "tensors": arena.names(), "guard_bytes": arena.guard_bytes(),
               "stray_bytes": sum(s[3] for s in stray)}

        def log():
            rec["seconds"] = round(time.perf_counter() - t0, 3)
            print("GUARD_BAND case=%s pattern=%s tensors=%s guard_bytes=%d stray_bytes=%d seconds=%.3f"
                  % (case_id, pattern, ",".join(rec["tensors"]), rec["guard_bytes"], rec["stray_bytes"], rec["seconds"]), flush=True)

        if stray or failed is not None:  # a call that strays inside the arena is NOT made again on exact-size tensors
            log()
            assert stray == [], (case_id, stray, failed)
            raise failed
        extra_p = body(twin, P) or {}
        torch.cuda.synchronize()
        state_a, state_p = _handle_state(env), _handle_state(twin)
        log()
        assert layout_ok, "a carved tensor lacks its guard"
        assert sorted(A.outs) == sorted(P.outs)
        for k in A.outs:
            a, p = A.outs[k], P.outs[k]
            assert a.shape == p.shape and a.dtype == p.dtype and torch.equal(_bytes(a), _bytes(p)), (case_id, "output differs from the twin's", k)
        assert sorted(state_a) == sorted(state_p) and sorted(extra_a) == sorted(extra_p)
        for what, xa, xp in (("handle", state_a, state_p), ("extra", extra_a, extra_p)):
            for k in xa:
                x, y = np.asarray(xa[k]), np.asarray(xp[k])
                assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (case_id, what, k)
        for k in A.full:
            assert arena.unwritten(k) == 0, (case_id, "entries the call should have written still hold the pattern", k, arena.unwritten(k))
        return rec
    finally:
        env.close()
        twin.close()


def _env(level, n, steps=0, auto_reset=True, layout="compact", seed=11, base=1000):
    def make():
        env = S.BatchedGridworldEnv(level, n, seed=seed, env_index_base=base, layout=layout)
        if steps:
            env.step_random(steps, auto_reset=auto_reset)
        return env
    return make


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _call(env, fn, *args):
    env._sync_torch_to_lib()
    _lib.check(fn(env.handle, *args))
    env._sync_lib_to_torch()


def _f32(torch, rng, shape, scale=0.3):
    return torch.as_tensor(rng.normal(0.0, scale, shape).astype(np.float32))


# ---- a. per-step outputs -----------------------------------------------------------------------------------------------------------------
PER_STEP_N = (1, 37, 257)
PER_STEP_LEVELS = (BOAT, SOKOBAN)  # rows of 25 bytes; the second level


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", PER_STEP_N)
@pytest.mark.parametrize("level", PER_STEP_LEVELS)
def test_per_step_observations(level, n, pattern):
    torch = _torch()

    def body(env, A):
        env.obs_f32(out=A.out("obs", (n, env.n_cells), torch.float32))
        shape = (n, env.H, env.W, 3) if env.info.render_hwc else (n, 3, env.H, env.W)
        env.render(out=A.out("rgb", shape, torch.uint8))

    check_case("obs_render/%s/n%d" % (level, n), pattern, _env(level, n, steps=7), body)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", PER_STEP_N)
@pytest.mark.parametrize("level", PER_STEP_LEVELS)
def test_per_step_draws(level, n, pattern):
    torch = _torch()

    def body(env, A):
        rng = np.random.default_rng(100 + n)
        scores = A.inp("scores", _f32(torch, rng, (n, 4), 1.0))
        eps_dev = A.inp("epsilon_dev", torch.tensor([0.4], dtype=torch.float64))
        draw_dev = A.inp("draw_index_dev", torch.tensor([9], dtype=torch.int64))
        _call(env, env.lib.sgk_epsilon_greedy, _ptr(scores), 0.3, 5, _ptr(A.out("eps_actions", (n,), torch.uint8)))
        _call(env, env.lib.sgk_epsilon_greedy_ex, _ptr(scores), 0.0, 0, _ptr(eps_dev), _ptr(draw_dev), _ptr(A.out("eps_ex_actions", (n,), torch.uint8)))
        _call(env, env.lib.sgk_epsilon_greedy_ex, _ptr(scores), 0.0, 6, None, None, _ptr(A.out("greedy_actions", (n,), torch.uint8)))
        _call(env, env.lib.sgk_categorical_sample, _ptr(scores), 7, None, _ptr(A.out("cat_actions", (n,), torch.uint8)))
        _call(env, env.lib.sgk_categorical_sample, _ptr(scores), 0, _ptr(draw_dev), _ptr(A.out("cat_dev_actions", (n,), torch.uint8)))

    check_case("draws/%s/n%d" % (level, n), pattern, _env(level, n, steps=7), body)


def _mlp_weights(torch, rng, cells, hidden, members=None):
    lead = () if members is None else (members,)
    shapes = {"w1t": (cells, hidden), "b1": (hidden,), "w2": (hidden, hidden), "b2": (hidden,), "w3t": (hidden, 4), "b3": (4,)}
    return {k: _f32(torch, rng, lead + s) for k, s in shapes.items()}


def _conv_weights(torch, rng, cells, C, members=None):
    lead = () if members is None else (members,)
    shapes = {"w1": (C, 1, 3, 3), "b1": (C,), "w2": (C, C, 3, 3), "b2": (C,), "wb": (C, 1, 1, 1), "bb": (C,), "wh": (C, C, 3, 3),
              "bh": (C,), "wl": (4, C * cells), "bl": (4,)}
    return {k: _f32(torch, rng, lead + s) for k, s in shapes.items()}


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("level,hidden,channels", [(BOAT, 100, 5), (SOKOBAN, 64, 4), ("DistributionalShift-v0", 128, 8)])
def test_acting_forwards(level, hidden, channels, pattern):
    """161 envs: one full tile of 128 and a ragged one. The float64 tests guard the tails of these outputs; here the FRONT too."""
    torch = _torch()
    n = 161

    def body(env, A):
        rng = np.random.default_rng(7)
        w = {k: A.inp("mlp_" + k, t) for k, t in _mlp_weights(torch, rng, env.n_cells, hidden).items()}
        cw = {k: A.inp("conv_" + k, t) for k, t in _conv_weights(torch, rng, env.n_cells, channels).items()}
        env.policy_act(w, 0.25, 3, out=A.out("act_actions", (n,), torch.uint8), scores_out=A.out("act_scores", (n, 4), torch.float32))
        env.policy_sample(w, 4, out=A.out("sample_actions", (n,), torch.uint8), logits_out=A.out("sample_logits", (n, 4), torch.float32))
        env.policy_act(w, 0.25, 5, out=A.out("act_actions_only", (n,), torch.uint8))
        env.convq_act(cw, 0.25, 3, channels, out=A.out("convq_actions", (n,), torch.uint8), scores_out=A.out("convq_scores", (n, 4), torch.float32))
        env.convq_sample(cw, 4, channels, out=A.out("convs_actions", (n,), torch.uint8), logits_out=A.out("convs_logits", (n, 4), torch.float32))
        env.convq_sample(cw, 6, channels, out=A.out("convs_actions_only", (n,), torch.uint8))

    check_case("acting/%s/H%d/C%d" % (level, hidden, channels), pattern, _env(level, n, steps=7), body)


def _tabq(env, epsilon=0.3):
    return S.BatchedTabularQAgent(env, types.SimpleNamespace(lr=0.1, discount=0.99, epsilon=epsilon, epsilon_anneal=100))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("level,n", [(BOAT, 1), (BOAT, 37), (BOAT, 257), (SOKOBAN, 1), (SOKOBAN, 37), (SOKOBAN, 257), (BOAT, 70001)])
def test_tabq_actions(level, n, pattern):
    """sgk_tabq_act and sgk_tabq_step with actions_out; 70 001 envs = the grid-stride form with a ragged last tile (on BoatRace alone: the
    ragged tile is the level's business no more than the grid stride is, and Sokoban's tables, a row per agent cell x box cell, would take gigabytes per handle there)."""
    torch = _torch()

    def body(env, A):
        agent = _tabq(env)
        try:
            for _ in range(3):  # (tables that are not all zeros)
                agent.step()
            for explore in (1, 0):
                agent._actions = A.out("act%d" % explore, (n,), torch.uint8)
                agent._act(explore)
            agent._actions = A.out("step_actions", (n,), torch.uint8)
            agent.step()
            agent._actions = A.out("step_cheat_actions", (n,), torch.uint8)
            agent.step(cheat=True, write_boards=False)
            torch.cuda.synchronize()
            k = min(n, 300)
            return {"table_head": agent.table_host(0, k), "table_tail": agent.table_host(n - k, k), "t": np.int64(agent.t)}
        finally:
            agent.close()

    check_case("tabq_act_step/%s/n%d" % (level, n), pattern, _env(level, n, steps=5), body)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("steps", [12, 0])
@pytest.mark.parametrize("n", PER_STEP_N)
def test_finished(n, steps, pattern):
    """Buffers of capacity n. 12 random steps without a reset on DistributionalShift (the lava is two cells from the start): some
    episodes are over (asserted for n > 1), the others are not; no step at all: none is, and nothing is written."""
    torch = _torch()
    seen = []

    def body(env, A):
        env._finished_bufs = tuple(A.out(k, (n,), torch.int32, fill=-7) for k in ("ids", "returns", "performance"))
        ids, ret, perf = env.finished()
        seen.append(int(ids.numel()))
        assert ids.numel() == 0 or torch.equal(ids, env._finished_bufs[0][:ids.numel()])
        return {"count": np.int64(ids.numel())}

    check_case("finished/n%d/steps%d" % (n, steps), pattern, _env("DistributionalShift-v0", n, steps=steps, auto_reset=False), body)
    if steps == 0:
        assert seen == [0, 0]
    elif n > 1:
        assert 0 < seen[0] < n, seen


# ---- b. replay rings ---------------------------------------------------------------------------------------------------------------------
RING_SLICES = 3
RING_SPECS = {"slice0": (0, None), "slice2": (2, None), "wrap": (1, 2)}  # (slice, *slice_dev): (2 + 1) % 3 = slice 0
# 257 / 70 001: rows that never line up with 16 bytes (lane-by-lane stores, a ragged last tile); 272 x 25 bytes is a multiple of 16:
# the tile writer, with a last tile of 16 envs
RING_N = (257, 272, 70001)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("spec", sorted(RING_SPECS))
@pytest.mark.parametrize("cheat", [0, 1])
@pytest.mark.parametrize("n", RING_N)
@pytest.mark.parametrize("layout", ["compact", "pitched"])
def test_replay_rings(layout, n, cheat, spec, pattern):
    """sgk_step_store, sgk_reset_done_store and both phases of sgk_replay_store into rings of 3 slices whose `outer` is one slice: a
    slice index off by one in either direction, or one that missed its modulo, lands in a guard."""
    torch = _torch()
    sl, sl_dev = RING_SPECS[spec]
    resolved = (sl + (sl_dev or 0)) % RING_SLICES

    def body(env, A):
        nc, lib = env.n_cells, env.lib
        rng = np.random.default_rng(n + cheat)
        actions = A.inp("actions", torch.as_tensor(rng.integers(0, 4, n).astype(np.uint8)))
        sd = None if sl_dev is None else A.inp("slice_dev", torch.tensor([sl_dev], dtype=torch.int64))
        sd2 = None if sl_dev is None else A.inp("replay_slice_dev", torch.tensor([resolved], dtype=torch.int64))  # (sgk_replay_store: no modulo)
        rings = {}
        for pre in ("", "replay_"):
            rings[pre + "states"] = A.out(pre + "states_ring", (RING_SLICES, n, nc), torch.int8, fill=0x5A)
            rings[pre + "successors"] = A.out(pre + "successors_ring", (RING_SLICES, n, nc), torch.int8, fill=0x5A)
            rings[pre + "actions"] = A.out(pre + "actions_ring", (RING_SLICES, n), torch.uint8, fill=0x5A)
            rings[pre + "rewards"] = A.out(pre + "rewards_ring", (RING_SLICES, n), torch.int8, fill=0x5A)
            rings[pre + "terminals"] = A.out(pre + "terminals_ring", (RING_SLICES, n), torch.uint8, fill=0x5A)
        p = {k: _ptr(t) for k, t in rings.items()}
        env._version += 1
        _call(env, lib.sgk_replay_store, 0, _ptr(actions), cheat, resolved, _ptr(sd2), p["replay_states"], p["replay_successors"],
              p["replay_actions"], p["replay_rewards"], p["replay_terminals"])
        _call(env, lib.sgk_step_store, _ptr(actions), 0, cheat, sl, _ptr(sd), RING_SLICES, p["successors"], p["actions"], p["rewards"], p["terminals"])
        _call(env, lib.sgk_replay_store, 1, _ptr(actions), cheat, resolved, _ptr(sd2), p["replay_states"], p["replay_successors"],
              p["replay_actions"], p["replay_rewards"], p["replay_terminals"])
        _call(env, lib.sgk_reset_done_store, 0, sl, _ptr(sd), RING_SLICES, p["states"])
        torch.cuda.synchronize()
        # the work was done in the arena: the named slice is written in full, the two others keep their fill; and the fused stores left
        # what the separate ones left
        for k, t in rings.items():
            others = [s for s in range(RING_SLICES) if s != resolved]
            assert bool((t[others] == 0x5A).all()), k
            assert not bool((t[resolved] == 0x5A).all()), k
        for k in ("successors", "actions", "rewards", "terminals"):
            assert torch.equal(rings[k], rings["replay_" + k]), k
        assert torch.equal(rings["states"][resolved].cpu(), torch.as_tensor(env.boards_host().reshape(n, nc)))

    # BoatRace, 99 steps into the episodes: the stored step is the 100th and ends every episode, the reset then restarts every env
    check_case("rings/%s/n%d/cheat%d/%s" % (layout, n, cheat, spec), pattern, _env(BOAT, n, steps=99, auto_reset=False, layout=layout), body,
               arena_bytes=(48 << 20) if n > 1000 else (4 << 20))


# ---- c. discounted returns ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("lengths", ["ragged", "null"])
@pytest.mark.parametrize("t_max", [1, 65, 100, 1024])
def test_discounted_returns(t_max, lengths, pattern):
    """9 trajectories (a workgroup serves 4: two full workgroups and one wave), lengths 0, 1, t_max and t_max + 5 (clamped) among them;
    the members form with 3 members x 3 trajectories. Entries at and behind a trajectory's length are not written: they keep the fill."""
    torch = _torch()
    n, members = 9, 3
    lens = np.array([0, 1, t_max, t_max + 5, max(t_max // 2, 1), t_max, 0, t_max + 5, 1], dtype=np.int32)

    def body(env, A):
        rng = np.random.default_rng(t_max)
        rewards = A.inp("rewards", _f32(torch, rng, (n, t_max), 1.0))
        lp = A.inp("lengths", torch.as_tensor(lens)) if lengths == "ragged" else None
        gp = np.stack([_lib.discount_powers(g, t_max) for g in (0.99, 0.9, 0.5)])
        gamma_pow = A.inp("gamma_pow", torch.as_tensor(gp))
        fill = 7.5 if lengths == "ragged" else None
        out1 = A.out("returns", (n, t_max), torch.float32, fill=fill)
        out2 = A.out("returns_members", (n, t_max), torch.float32, fill=fill)
        _call(env, env.lib.sgk_discounted_returns, _ptr(rewards), _ptr(lp), _ptr(out1), n, t_max, 0.9)
        _call(env, env.lib.sgk_discounted_returns_members, _ptr(rewards), _ptr(lp), _ptr(out2), n, t_max, members, _ptr(gamma_pow))
        torch.cuda.synchronize()
        assert torch.equal(out1[3:6], out2[3:6])  # member 1's discount is the shared call's
        if lengths == "ragged":
            for i, k in enumerate(np.minimum(lens, t_max)):
                assert bool((out1[i, k:] == 7.5).all()) and bool((out2[i, k:] == 7.5).all()), i
                assert k == 0 or out1[i, k - 1] == rewards[i, k - 1] * float(_lib.discount_powers(0.9, t_max)[k - 1])

    check_case("returns/T%d/%s" % (t_max, lengths), pattern, _env(BOAT, 4), body)


# ---- d. rollouts -------------------------------------------------------------------------------------------------------------------------
ROLLOUT_STEPS = 6
ROLLOUT_FORMS = {  # form: (level, members, envs per member)
    "policy": (BOAT, None, 161), "policy_members": (BOAT, 3, 43), "policy_members_eps": (SOKOBAN, 5, 2),
    "convq": (SOKOBAN, None, 161), "convq_members": (BOAT, 3, 43),
}
ROLLOUT_VARIANTS = [("greedy", True, False, "all"), ("sample", False, True, "all"), ("sample", True, True, "all"), ("greedy", False, False, "all"),
                    ("sample", False, False, "actions")]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("mode,auto_reset,mask,outs", ROLLOUT_VARIANTS)
@pytest.mark.parametrize("form", sorted(ROLLOUT_FORMS))
def test_rollouts(form, mode, auto_reset, mask, outs, pattern):
    """6 steps from boards 97 random steps into their episodes (BoatRace's end at step 100: inside the rollout); every output's `outer`
    is one step. `actions`: only actions_out is passed."""
    torch = _torch()
    level, members, E = ROLLOUT_FORMS[form]
    n, T, C, hidden = (members or 1) * E, ROLLOUT_STEPS, 5, 100 if members is None else 64

    def body(env, A):
        rng = np.random.default_rng(3)
        nc = env.n_cells
        if form.startswith("policy"):
            w = {k: A.inp("w_" + k, t) for k, t in _mlp_weights(torch, rng, nc, hidden, members).items()}
        else:
            w = {k: A.inp("w_" + k, t) for k, t in _conv_weights(torch, rng, nc, C, members).items()}
        kw = dict(mode=mode, epsilon=0.3, draw_index0=40, auto_reset=auto_reset, mask_finished=mask,
                  actions=A.out("actions_out", (T, n), torch.uint8))
        if outs == "all":
            kw.update(states=A.out("states_out", (T, n, nc), torch.int8), recs=A.out("recs_out", (T, n, 4), torch.int8))
        if members is not None:
            mm = torch.zeros((members, _lib.METRICS_LEN), dtype=torch.int64)
            mm[:, _lib.M_MAX_RETURN:_lib.M_MAX_MARGIN_POS + 1] = I64_MIN
            kw.update(member_metrics=A.state("member_metrics", mm))
        if form == "policy":
            env.policy_rollout(w, T, **kw)
        elif form == "convq":
            env.convq_rollout(w, T, C, **kw)
        elif form == "convq_members":
            env.convq_rollout_members(w, members, T, C, **kw)
        else:
            if form.endswith("_eps"):
                kw.update(member_epsilon=A.inp("member_epsilon", torch.as_tensor(np.linspace(0.0, 1.0, members))))
            env.policy_rollout_members(w, members, T, **kw)
        if members is not None and auto_reset:
            torch.cuda.synchronize()
            assert int(kw["member_metrics"][:, _lib.M_EPISODES].sum()) > 0  # episodes did end inside the rollout

    check_case("rollout/%s/%s/reset%d/mask%d/%s" % (form, mode, auto_reset, mask, outs), pattern, _env(level, n, steps=97), body)


# ---- e. ensemble and consensus -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("voters", ["all", "two"])
def test_ensemble(voters, pattern):
    torch = _torch()
    M, n = 3, 165

    def body(env, A):
        rng = np.random.default_rng(5)
        w = {k: A.inp("w_" + k, t) for k, t in _mlp_weights(torch, rng, env.n_cells, 100, M).items()}
        env.policy_act_members_all(w, M, out=A.out("member_actions", (M, n), torch.uint8), scores_out=A.out("member_scores", (M, n, 4), torch.float32))
        env.policy_act_members_all(w, M, out=A.out("member_actions_only", (M, n), torch.uint8))
        ma = rng.integers(0, 4, (M, n)).astype(np.uint8)
        ma[1, ::17] = 200  # (a byte above 3 casts no vote)
        ma = A.inp("vote_member_actions", torch.as_tensor(ma))
        ids = None if voters == "all" else A.inp("member_ids", torch.tensor([2, 0], dtype=torch.int32))
        dissent = A.state("dissent", torch.tensor([5, 11], dtype=torch.int64))
        env.members_vote(ma, members=ids, out=A.out("vote_actions", (n,), torch.uint8), votes_out=A.out("votes", (n, 4), torch.int16), dissent=dissent)
        env.members_vote(ma, members=ids, out=A.out("vote_actions_only", (n,), torch.uint8))
        torch.cuda.synchronize()
        assert int(dissent[1]) > 11 and int(dissent[0]) >= 5

    check_case("ensemble/%s" % voters, pattern, _env(BOAT, n, steps=7), body)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("level,n", [(BOAT, 200), (BOAT, 4160), (SOKOBAN, 130)])
def test_tabq_consensus(level, n, mask, pattern):
    """sgk_tabq_consensus (4160 agents: the multi-workgroup atomics form) and sgk_tabq_load_shared, whose table is a frozen input."""
    torch = _torch()

    def body(env, A):
        agent = _tabq(env, epsilon=0.8)
        try:
            for _ in range(12):
                agent.step()
            S_ = agent.n_states
            m = None
            if mask:
                m = A.inp("voters_mask", torch.as_tensor((np.random.default_rng(n).random(n) < 0.6).astype(np.uint8)))
            votes, voters = A.out("votes", (S_, 4), torch.int64), A.out("voters", (S_,), torch.int64)
            agent.consensus(mask=m, votes_out=votes, voters_out=voters)
            env._sync_torch_to_lib()
            _lib.check(env.lib.sgk_tabq_consensus(agent._h, _ptr(m), _ptr(A.out("votes_only", (S_, 4), torch.int64)), None))
            torch.cuda.synchronize()
            assert int(voters.sum()) > 0 and torch.equal(votes.sum(dim=1), voters)
            shared = A.inp("shared_table", torch.as_tensor(np.random.default_rng(1).normal(size=(S_, 4))))
            agent.load_shared_table(shared)
            torch.cuda.synchronize()
            k = min(n, 300)
            tail = agent.table_host(n - k, k)
            assert (tail == shared.cpu().numpy()[None]).all()
            return {"table_head": agent.table_host(0, k), "table_tail": tail}
        finally:
            agent.close()

    check_case("consensus/%s/n%d/mask%d" % (level, n, mask), pattern, _env(level, n, steps=5), body)


# ---- f. population-based training --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("M", [1, 5, 1025])
def test_members_select(M, explore, pattern):
    """sgk_members_select; with the explore step both hyper layouts ([M, 4] PPO rows, [M, 2] DQN rows) and the generation word.
    (sgk_members_clone: tests/test_gpu_pbt.py has guard rows around the cloned tensors.)"""
    torch = _torch()

    def body(env, A):
        rng = np.random.default_rng(M)
        scores = A.inp("scores", torch.as_tensor(rng.normal(size=M)))
        for cols in (4, 2):
            src = A.out("src_out_%d" % cols, (M,), torch.int32)
            ex = None
            if explore:
                hyper = A.state("hyper_%d" % cols, torch.as_tensor(rng.uniform(0.1, 1.0, (M, cols))))
                gen = A.state("generation_%d" % cols, torch.tensor([41], dtype=torch.int64))
                ex = _lib.SgkMembersExplore(hyper_dev=hyper.data_ptr(), n_columns=cols, perturb_mask=0b0101, factor_down=0.8, factor_up=1.25,
                                            key=77, generation_dev=gen.data_ptr())
                for k in range(cols):
                    ex.lo[k], ex.hi[k] = 0.05, 1.1
            env.members_select(scores, M // 4, src, explore=ex)
            if explore:
                torch.cuda.synchronize()
                assert int(gen[0]) == 42

    check_case("select/M%d/explore%d" % (M, explore), pattern, _env(BOAT, 4), body)


# ---- g. learners -------------------------------------------------------------------------------------------------------------------------
DQN_PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")
PPO_PARAMS = ("w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc")
CNN_PARAMS = ("w1", "b1", "w2", "b2", "wb", "bb", "wa", "ba", "la", "lab", "wv", "bv", "lv", "lvb")


def _lead(members):
    return () if members is None else (members,)


def _adam_state(torch, rng, shape, amsgrad):
    m = _f32(torch, rng, shape, 0.01)
    v = torch.as_tensor((rng.random(shape) * 1e-4 + 1e-6).astype(np.float32))
    out = [m, v]
    if amsgrad:
        out.append(v * torch.as_tensor(rng.choice(np.array([0.5, 2.0], dtype=np.float32), shape)))
    return out


def _hyper_rows(torch, rng, members, base):
    return torch.as_tensor(np.asarray(base)[None] * rng.uniform(0.5, 1.5, (members, len(base))))


def dqn_body(cells, hidden, batch, loss_mode, rows_mode, form, members=None, E=None, slices=RING_SLICES, reset_spec="wrap"):
    """One sgk_dqn_sgd_step[_reset_store | _members | _members_hyper] with EVERY pointer of sgk_dqn_learner carved. Stacked tensors
    ([members, ...]) get one member slice as their `outer` from their shape."""
    torch = _torch()
    M = members or 1

    def body(env, A):
        n, lib = env.n_envs, env.lib
        rng = np.random.default_rng(cells * 1000 + hidden + batch)
        ld = _lead(members)
        L = _lib.SgkDqnLearner()
        ring = {"states": rng.integers(0, 5, (slices, n, cells)).astype(np.int8), "successors": rng.integers(0, 5, (slices, n, cells)).astype(np.int8),
                "actions": rng.integers(0, 4, (slices, n)).astype(np.uint8), "rewards": rng.integers(-2, 3, (slices, n)).astype(np.int8),
                "terminals": (rng.random((slices, n)) < 0.3).astype(np.uint8)}
        for k, a in ring.items():
            setattr(L, k, A.inp("ring_" + k, torch.as_tensor(a)).data_ptr())
        L.slices_filled, L.n_hidden, L.batch, L.loss_mode = slices, hidden, batch, loss_mode
        shapes = {"w1": (hidden, cells), "b1": (hidden,), "w2": (hidden, hidden), "b2": (hidden,), "w3": (4, hidden), "b3": (4,)}
        cur = {k: _f32(torch, rng, ld + s) for k, s in shapes.items()}
        for i, k in enumerate(DQN_PARAMS):
            setattr(L, k, A.state(k, cur[k]).data_ptr())
            for name, arr, t in zip(("m", "v", "vmax"), (L.m, L.v, L.vmax), _adam_state(torch, rng, ld + shapes[k], True)):
                arr[i] = A.state("%s_%s" % (name, k), t).data_ptr()
        for k in ("w1", "w2", "w3"):
            setattr(L, k + "t", A.state(k + "t", cur[k].transpose(-1, -2).contiguous()).data_ptr())
        tshapes = {"tw1t": (cells, hidden), "tb1": (hidden,), "tw2t": (hidden, hidden), "tb2": (hidden,), "tw3": (4, hidden), "tb3": (4,)}
        for k, s in tshapes.items():
            setattr(L, k, A.inp(k, _f32(torch, rng, ld + s)).data_ptr())
        step = A.state("step", torch.full((M,), 4999, dtype=torch.int64))
        L.step, L.loss_out = step.data_ptr(), A.out("loss_out", (M,), torch.float32).data_ptr()
        L.lr, L.beta1, L.beta2, L.eps, L.discount, L.max_grad_norm = 1e-2, 0.9, 0.999, 1e-8, 0.9, 10.0
        rows_out = A.out("rows_out", ld + (batch,), torch.int64)
        L.rows_out = rows_out.data_ptr()
        if rows_mode == "given":
            E_ = n // M
            rows = np.stack([rng.integers(0, slices, batch) * n + m * E_ + rng.integers(0, E_, batch) for m in range(M)]).reshape(ld + (batch,))
            rows = A.inp("rows", torch.as_tensor(rows.astype(np.int64)))
            L.rows = rows.data_ptr()
        if form == "single":
            _call(env, lib.sgk_dqn_sgd_step, ctypes.byref(L))
        elif form == "first_call_in_a_capture":  # (one_launch_probe: the status alone, nothing runs)
            torch.cuda.synchronize()
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                step.add_(0)  # (no empty capture)
                env._sync_torch_to_lib()
                return {"rc": int(lib.sgk_dqn_sgd_step(env.handle, ctypes.byref(L)))}
        elif form == "reset_store":
            sl, sl_dev = RING_SPECS[reset_spec]
            sd = None if sl_dev is None else A.inp("slice_dev", torch.tensor([sl_dev], dtype=torch.int64))
            states_ring = A.out("next_states_ring", (RING_SLICES, n, cells), torch.int8, fill=0x5A)
            env._version += 1
            _call(env, lib.sgk_dqn_sgd_step_reset_store, ctypes.byref(L), 0, sl, _ptr(sd), RING_SLICES, _ptr(states_ring))
            torch.cuda.synchronize()
            resolved = (sl + (sl_dev or 0)) % RING_SLICES
            assert torch.equal(states_ring[resolved].cpu(), torch.as_tensor(env.boards_host().reshape(n, cells)))
            assert bool((states_ring[[s for s in range(RING_SLICES) if s != resolved]] == 0x5A).all())
        else:
            need = env.dqn_members_workspace_bytes(hidden, M)
            ws = A.scratch("workspace", need, outer=need // M)  # sized exactly: no rounding added
            keys = A.inp("member_keys", torch.as_tensor(np.arange(M, dtype=np.int64) * 7919 + 3))
            if form == "members_hyper":
                hyper = A.inp("member_hyper", _hyper_rows(torch, rng, M, (1e-2, 0.9)))
                _call(env, lib.sgk_dqn_sgd_step_members_hyper, ctypes.byref(L), M, _ptr(keys), _ptr(ws), _ptr(hyper))
            else:
                _call(env, lib.sgk_dqn_sgd_step_members, ctypes.byref(L), M, _ptr(keys), _ptr(ws))
        torch.cuda.synchronize()
        assert bool((step == 5000).all())
        if rows_mode == "given":
            assert torch.equal(rows_out, rows)
        else:
            r = rows_out.reshape(M, batch)
            for m in range(M):  # a member draws inside the stored transitions, from its own columns
                assert bool(((r[m] >= 0) & (r[m] < slices * n) & (r[m] % n // (n // M) == m)).all()), m

    return body


DQN_CASES = (
    # K0, hidden, batch, loss_mode, rows: both K0 % 4 classes (25, 30, 63 / 36), both widths, batches 1 / 7 / 64, both losses, both row sources
    [(k0, h, b, (k0 + h + b) % 2, "given" if (k0 // 5 + h // 50 + b) % 2 else "null") for k0 in (25, 30, 36, 63) for h in (64, 100) for b in (1, 64)]
    + [(25, 100, 7, 0, "null"), (36, 64, 7, 1, "given"), (25, 64, 64, 0, "given"), (36, 100, 1, 0, "given")])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("form", ["single", "reset_store"])
@pytest.mark.parametrize("cells,hidden,batch,loss_mode,rows_mode", DQN_CASES)
def test_dqn_learner(cells, hidden, batch, loss_mode, rows_mode, form, pattern):
    # 9 envs x 3 slices; the reset half's ring: 3 slices, *slice_dev = 2 and slice = 1 wrap to slice 0
    check_case("dqn/%s/K%d/H%d/B%d/loss%d/rows_%s" % (form, cells, hidden, batch, loss_mode, rows_mode), pattern,
               _env(CELL_LEVEL[cells], 9, steps=100, auto_reset=False), dqn_body(cells, hidden, batch, loss_mode, rows_mode, form))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("spec", sorted(RING_SPECS))
@pytest.mark.parametrize("n", RING_N)
@pytest.mark.parametrize("layout", ["compact", "pitched"])
def test_dqn_reset_store_rings(layout, n, spec, pattern):
    """The reset half of sgk_dqn_sgd_step_reset_store -- reset_done + the next transitions' states, carried by the Adam launch -- at the
    replay rings' own shapes: 3 slices, n 257 / 272 / 70 001, both board layouts, slices 0 and 2 named directly and the wrapped one.
    BoatRace 100 steps into its episodes: every env is over and is reset."""
    check_case("dqn/reset_store_ring/%s/n%d/%s" % (layout, n, spec), pattern, _env(BOAT, n, steps=100, auto_reset=False, layout=layout),
               dqn_body(25, 64, 7, 0, "null", "reset_store", reset_spec=spec), arena_bytes=(48 << 20) if n > 1000 else (4 << 20))


MEMBER_SHAPES = [(3, 4), (5, 2)]  # (members, envs / trajectories per member)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("form", ["members", "members_hyper"])
@pytest.mark.parametrize("members,E", MEMBER_SHAPES)
@pytest.mark.parametrize("cells,hidden,batch,loss_mode,rows_mode", [(25, 64, 7, 0, "null"), (36, 100, 64, 1, "given"), (63, 100, 1, 0, "null"),
                                                                    (30, 64, 64, 1, "null")])
def test_dqn_learner_members(cells, hidden, batch, loss_mode, rows_mode, members, E, form, pattern):
    check_case("dqn/%s/M%dxE%d/K%d/H%d/B%d/loss%d/rows_%s" % (form, members, E, cells, hidden, batch, loss_mode, rows_mode), pattern,
               _env(CELL_LEVEL[cells], members * E, steps=5), dqn_body(cells, hidden, batch, loss_mode, rows_mode, form, members, E))


ONE_LAUNCH_CASES = [(25, 100, 64, 0, "null"), (36, 64, 7, 1, "given")]


def one_launch_probe():
    """Which Adam does this process's library run? The status of sgk_dqn_sgd_step made as a handle's FIRST learner call inside a stream
    capture: the two-launch form has to allocate the handle's scratch block for the gradient and refuses (SGK_ERR_INVALID, "call it once
    before capturing it": nothing is launched); the in-kernel Adam needs no block and the call is recorded (SGK_OK; the recording is
    dropped without a replay). The difference include/sgk.h documents for sgk_dqn_sgd_step's first call."""
    torch = _torch()
    env = _env(BOAT, 9)()
    try:
        return dqn_body(25, 100, 64, 0, "null", "first_call_in_a_capture")(env, _PlainAlloc("cuda:%d" % env.device))["rc"]
    finally:
        torch.cuda.synchronize()
        env.close()


def one_launch_records():
    """This file's DQN case for ONE_LAUNCH_CASES under both patterns, in this process (run as a script by test_dqn_one_launch_adam with
    SGK_DQN_ONE_LAUNCH=1 in the environment: the arena is the child's own, and so is the twin)."""
    out = []
    for cells, hidden, batch, loss_mode, rows_mode in ONE_LAUNCH_CASES:
        for pattern in PATTERNS:
            case = "dqn/one_launch/K%d/H%d/B%d/loss%d/rows_%s" % (cells, hidden, batch, loss_mode, rows_mode)
            try:
                rec = check_case(case, pattern, _env(CELL_LEVEL[cells], 9, steps=5), dqn_body(cells, hidden, batch, loss_mode, rows_mode, "single"))
                rec["error"] = None
            except AssertionError as exc:
                rec = {"case": case, "pattern": pattern, "error": repr(exc)[:2000]}
            out.append(rec)
    return out


def test_dqn_one_launch_adam():
    """The non-default in-kernel Adam (SGK_DQN_ONE_LAUNCH=1, read when the library is loaded: a fresh child process): dqn_sgd_kernel's own
    16-byte stores into parameters, moments and transposed copies, K0 25 and 36, both patterns. That the child did run that Adam is
    checked, not assumed: one_launch_probe() answers SGK_OK there and SGK_ERR_INVALID in this process (the default two launches)."""
    assert os.environ.get("SGK_DQN_ONE_LAUNCH") != "1" and one_launch_probe() == _lib.ERR_INVALID
    env = dict(os.environ, SGK_DQN_ONE_LAUNCH="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    sys.stdout.write("".join(line + "\n" for line in p.stdout.splitlines() if line.startswith("GUARD_BAND")))
    recs = json.loads(next(line for line in p.stdout.splitlines() if line.startswith("RECORDS "))[len("RECORDS "):])
    assert len(recs) == 2 * len(ONE_LAUNCH_CASES)
    probe = next(line for line in p.stdout.splitlines() if line.startswith("PROBE "))
    assert probe == "PROBE %d" % _lib.SGK_OK, "the child did not run the in-kernel Adam: %s" % probe
    for r in recs:
        assert r["error"] is None and r["stray_bytes"] == 0, r


def ppo_body(cells, hidden, batch, rows_mode, form, members=None, epochs=2):
    """sgk_ppo_epochs[_members | _members_hyper] on a ragged rollout (lengths 0 / 1 / 2 / 5 in turn, horizon 5) with every pointer of
    sgk_ppo_learner carved."""
    torch = _torch()
    M, T = members or 1, 5

    def body(env, A):
        lib = env.lib
        n = env.n_envs  # trajectories
        rng = np.random.default_rng(cells * 1000 + hidden + batch)
        ld = _lead(members)
        L = _lib.SgkPpoLearner()
        lengths = np.array([(0, 1, 2, 5)[(i + i // 4) % 4] for i in range(n)], dtype=np.int32)
        L.states = A.inp("states", torch.as_tensor(rng.integers(0, 5, (T, n, cells)).astype(np.int8))).data_ptr()
        L.actions = A.inp("actions", torch.as_tensor(rng.integers(0, 4, (T, n)).astype(np.uint8))).data_ptr()
        L.returns = A.inp("returns", _f32(torch, rng, (n, T), 1.0)).data_ptr()
        L.lengths = A.inp("lengths", torch.as_tensor(lengths)).data_ptr()
        L.horizon, L.n_hidden, L.batch, L.n_epochs, L.n_trajectories = T, hidden, batch, epochs, n
        shapes = {"w1": (hidden, cells), "b1": (hidden,), "w2": (hidden, hidden), "b2": (hidden,), "wa": (4, hidden), "ba": (4,),
                  "wc": (1, hidden), "bc": (1,)}
        cur = {k: _f32(torch, rng, ld + s) for k, s in shapes.items()}
        for i, k in enumerate(PPO_PARAMS):
            setattr(L, k, A.state(k, cur[k]).data_ptr())
            for name, arr, t in zip(("m", "v"), (L.m, L.v), _adam_state(torch, rng, ld + shapes[k], False)):
                arr[i] = A.state("%s_%s" % (name, k), t).data_ptr()
        for k in ("w1", "w2"):
            setattr(L, k + "t", A.state(k + "t", cur[k].transpose(-1, -2).contiguous()).data_ptr())
        oshapes = {"ow1t": (cells, hidden), "ob1": (hidden,), "ow2t": (hidden, hidden), "ob2": (hidden,), "owa": (4, hidden), "oba": (4,)}
        for k, s in oshapes.items():
            setattr(L, k, A.inp(k, _f32(torch, rng, ld + s)).data_ptr())
        step = A.state("step", torch.full((M,), 300, dtype=torch.int64))
        L.step = step.data_ptr()
        L.stats_out = A.out("stats_out", ld + (epochs, 3), torch.float32).data_ptr()
        rows_out = A.out("rows_out", ld + (epochs, batch), torch.int64)
        L.rows_out = rows_out.data_ptr()
        L.lr, L.beta1, L.beta2, L.eps, L.clipping, L.critic_coeff, L.entropy_bonus = 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.5, 0.02
        E_ = n // M
        if rows_mode == "given":
            own = [np.flatnonzero(lengths[m * E_:(m + 1) * E_] > 0) + m * E_ for m in range(M)]
            rows = np.stack([rng.choice(own[m], (epochs, batch)) for m in range(M)]).reshape(ld + (epochs, batch))  # (step 0 of a trajectory that has one)
            rows = A.inp("rows", torch.as_tensor(rows.astype(np.int64)))
            L.rows = rows.data_ptr()
        keys = None if members is None else A.inp("member_keys", torch.as_tensor(np.arange(M, dtype=np.int64) * 7919 + 3))
        if form == "single":
            _call(env, lib.sgk_ppo_epochs, ctypes.byref(L))
        elif form == "members":
            _call(env, lib.sgk_ppo_epochs_members, ctypes.byref(L), M, _ptr(keys))
        else:
            hyper = A.inp("member_hyper", _hyper_rows(torch, rng, M, (1e-3, 0.1, 0.5, 0.02)))
            _call(env, lib.sgk_ppo_epochs_members_hyper, ctypes.byref(L), M, _ptr(keys), _ptr(hyper))
        torch.cuda.synchronize()
        assert bool((step == 300 + epochs).all())
        r = rows_out.reshape(M, epochs * batch).cpu().numpy()
        if rows_mode == "given":
            assert torch.equal(rows_out, rows)
        else:
            for m in range(M):  # the kernel's own draws: inside an episode of one of the member's own trajectories
                t, traj = r[m] // n, r[m] % n
                assert ((traj // E_ == m) & (t < lengths[traj])).all(), m

    return body


PPO_CASES = ([(k0, h, b, "null") for k0 in (25, 30, 36, 63) for h in (64, 100) for b in (2, 33)]
             + [(25, 100, 33, "given"), (36, 64, 2, "given")])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("cells,hidden,batch,rows_mode", PPO_CASES)
def test_ppo_learner(cells, hidden, batch, rows_mode, pattern):
    check_case("ppo/single/K%d/H%d/B%d/rows_%s" % (cells, hidden, batch, rows_mode), pattern, _env(CELL_LEVEL[cells], 8),
               ppo_body(cells, hidden, batch, rows_mode, "single"))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("form", ["members", "members_hyper"])
@pytest.mark.parametrize("members,E", MEMBER_SHAPES)
@pytest.mark.parametrize("cells,hidden,batch,rows_mode", [(25, 64, 33, "null"), (36, 100, 2, "given"), (63, 100, 33, "null"), (30, 64, 2, "null")])
def test_ppo_learner_members(cells, hidden, batch, rows_mode, members, E, form, pattern):
    check_case("ppo/%s/M%dxE%d/K%d/H%d/B%d/rows_%s" % (form, members, E, cells, hidden, batch, rows_mode), pattern,
               _env(CELL_LEVEL[cells], members * E), ppo_body(cells, hidden, batch, rows_mode, form, members))


def ppo_cnn_body(C, batch, rows_mode, form, members=None, epochs=2):
    """sgk_ppo_cnn_epochs[_members | _members_hyper] with every pointer of sgk_ppo_cnn_learner carved; the workspace holds exactly
    sgk_ppo_cnn[_members]_workspace_bytes bytes."""
    torch = _torch()
    M, T = members or 1, 5

    def body(env, A):
        lib, cells = env.lib, env.n_cells
        n = env.n_envs
        rng = np.random.default_rng(cells * 1000 + C + batch)
        ld = _lead(members)
        L = _lib.SgkPpoCnnLearner()
        lengths = np.array([(5, 1, 2, 0)[(i + i // 4) % 4] for i in range(n)], dtype=np.int32)
        L.states = A.inp("states", torch.as_tensor(rng.integers(0, 5, (T, n, cells)).astype(np.int8))).data_ptr()
        L.actions = A.inp("actions", torch.as_tensor(rng.integers(0, 4, (T, n)).astype(np.uint8))).data_ptr()
        L.returns = A.inp("returns", _f32(torch, rng, (n, T), 1.0)).data_ptr()
        L.lengths = A.inp("lengths", torch.as_tensor(lengths)).data_ptr()
        L.horizon, L.n_channels, L.batch, L.n_epochs, L.n_trajectories = T, C, batch, epochs, n
        conv, lin = (C, C, 3, 3), C * cells
        shapes = {"w1": (C, 1, 3, 3), "b1": (C,), "w2": conv, "b2": (C,), "wb": (C, 1, 1, 1), "bb": (C,), "wa": conv, "ba": (C,),
                  "la": (4, lin), "lab": (4,), "wv": conv, "bv": (C,), "lv": (1, lin), "lvb": (1,)}
        for i, k in enumerate(CNN_PARAMS):
            L.params[i] = A.state(k, _f32(torch, rng, ld + shapes[k], 0.2)).data_ptr()
            for name, arr, t in zip(("m", "v"), (L.m, L.v), _adam_state(torch, rng, ld + shapes[k], False)):
                arr[i] = A.state("%s_%s" % (name, k), t).data_ptr()
        for i, k in enumerate(CNN_PARAMS[:10]):
            L.old_params[i] = A.inp("old_" + k, _f32(torch, rng, ld + shapes[k], 0.2)).data_ptr()
        step = A.state("step", torch.full((M,), 300, dtype=torch.int64))
        L.step = step.data_ptr()
        L.stats_out = A.out("stats_out", ld + (epochs, 3), torch.float32).data_ptr()
        rows_out = A.out("rows_out", ld + (epochs, batch), torch.int64)
        L.rows_out = rows_out.data_ptr()
        L.lr, L.beta1, L.beta2, L.eps, L.clipping, L.critic_coeff, L.entropy_bonus = 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.5, 0.02
        E_ = n // M
        if rows_mode == "given":
            own = [np.flatnonzero(lengths[m * E_:(m + 1) * E_] > 0) + m * E_ for m in range(M)]
            rows = np.stack([rng.choice(own[m], (epochs, batch)) for m in range(M)]).reshape(ld + (epochs, batch))
            rows = A.inp("rows", torch.as_tensor(rows.astype(np.int64)))
            L.rows = rows.data_ptr()
        if form == "single":
            need = env.ppo_cnn_workspace_bytes(C, batch)
            L.workspace = A.scratch("workspace", need).data_ptr()
            _call(env, lib.sgk_ppo_cnn_epochs, ctypes.byref(L))
        else:
            need = env.ppo_cnn_members_workspace_bytes(C, batch, M)
            L.workspace = A.scratch("workspace", need, outer=need // M).data_ptr()
            keys = A.inp("member_keys", torch.as_tensor(np.arange(M, dtype=np.int64) * 7919 + 3))
            if form == "members":
                _call(env, lib.sgk_ppo_cnn_epochs_members, ctypes.byref(L), M, _ptr(keys))
            else:
                hyper = A.inp("member_hyper", _hyper_rows(torch, rng, M, (1e-3, 0.1, 0.5, 0.02)))
                _call(env, lib.sgk_ppo_cnn_epochs_members_hyper, ctypes.byref(L), M, _ptr(keys), _ptr(hyper))
        torch.cuda.synchronize()
        assert bool((step == 300 + epochs).all())
        r = rows_out.reshape(M, epochs * batch).cpu().numpy()
        if rows_mode == "given":
            assert torch.equal(rows_out, rows)
        else:
            for m in range(M):
                t, traj = r[m] // n, r[m] % n
                assert ((traj // E_ == m) & (t < lengths[traj])).all(), m

    return body


CNN_LEVELS = {"5x5": BOAT, "6x8": "IslandNavigation-v0", "7x9": "DistributionalShift-v0"}
PPO_CNN_CASES = ([(b, C, batch, "null") for b in ("5x5", "6x8", "7x9") for C in (4, 5, 8) for batch in (2, 37)]
                 + [("5x5", 5, 37, "given"), ("7x9", 8, 2, "given")])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("board,C,batch,rows_mode", PPO_CNN_CASES)
def test_ppo_cnn_learner(board, C, batch, rows_mode, pattern):
    check_case("ppo_cnn/single/%s/C%d/B%d/rows_%s" % (board, C, batch, rows_mode), pattern, _env(CNN_LEVELS[board], 8),
               ppo_cnn_body(C, batch, rows_mode, "single"), arena_bytes=16 << 20)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("form", ["members", "members_hyper"])
@pytest.mark.parametrize("members,E", MEMBER_SHAPES)
@pytest.mark.parametrize("board,C,batch,rows_mode", [("5x5", 5, 37, "null"), ("6x8", 4, 2, "given"), ("7x9", 8, 37, "null")])
def test_ppo_cnn_learner_members(board, C, batch, rows_mode, members, E, form, pattern):
    check_case("ppo_cnn/%s/M%dxE%d/%s/C%d/B%d/rows_%s" % (form, members, E, board, C, batch, rows_mode), pattern,
               _env(CNN_LEVELS[board], members * E), ppo_cnn_body(C, batch, rows_mode, form, members), arena_bytes=48 << 20)


if __name__ == "__main__":  # the child of test_dqn_one_launch_adam
    print("RECORDS " + json.dumps(one_launch_records()), flush=True)
    print("PROBE %d" % one_launch_probe(), flush=True)  # (behind the cases: the kernel's dynamic-LDS opt-in is made by then)
