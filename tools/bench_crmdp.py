"""ppo-crmdp's device path per shape, BoatRace, 100-step episodes: N = 256 / 4 096 / 32 768 trajectories with ONE agent (the merge is
serial by definition: one workgroup walks all N trajectories) and with N / 8 agents of 8 trajectories each:
    sgk_crmdp_keys            the keys of a rollout (reads T x N x 25 bytes once)
    sgk_crmdp_filter          detect + merge, two launches (the split per kernel: --trace, below)
    sgk_crmdp_filter_host     the same inputs on ONE core (wall clock; with several agents and more than HOST_CAP trajectories the first
                              HOST_CAP of them -- whole agents -- are run and the figure is scaled, the call being linear in the
                              trajectories, and labelled so; one agent always runs them all)
    gather_rollout            BatchedPPOCRMDPAgent's whole gather against BatchedPPOAgent(body="cnn")'s unfiltered one (one agent only:
                              the batched agent has one memory)
The inputs are a real rollout of the agent's own policy (BoatRace's own rewards). ROUNDS alternating rounds after a warm-up round,
device events on the handle's stream, one process per shape. The memory is reset before every filter round: every round merges into a
fresh memory, as the first iteration of a run does.

    python tools/bench_crmdp.py [LOG]        (default LOG: profiles/crmdp/bench_crmdp.log)
  --shape N AGENTS LOG     one shape, appended to LOG (what the driver starts)
  --trace N AGENTS         keys + filter only, six times, nothing else: the body of
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_crmdp.py --trace N AGENTS`
                           (a run of its own, no counters), whose *_kernel_stats.csv rows give detect and merge apart
                           (profiles/crmdp/kernel_trace.log)"""
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, ROUNDS, T, HOST_CAP = (256, 4096, 32768), 5, 100, 2048


def _import():
    for p in (ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
        sys.path.insert(0, p)
    import torch

    import safe_grid_agents_amd as S

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    return torch, S


def _args(n):
    return types.SimpleNamespace(discount=0.99, batch_size=64, rollouts=n, epochs=2, n_layers=2, n_hidden=None, n_channels=5, device=0,
                                 log_gradients=False, cheat=False, seed=5, lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01,
                                 env_alias="trans-boat")


def _events(torch, fn):
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    fn()
    end.record()
    end.synchronize()
    return 1e3 * begin.elapsed_time(end)


def _med(t):
    return (statistics.median(t), min(t), max(t))


def _setup(torch, S, n, agents):
    """The agent after one gather (its buffers hold a real rollout) and the raw calls on those buffers with a memory of `agents` agents."""
    from safe_grid_agents_amd import crmdp

    env = S.BatchedGridworldEnv("BoatRace-v0", n, seed=5)
    env.bind_torch_stream()
    torch.manual_seed(5)
    agent = S.BatchedPPOCRMDPAgent(env, _args(n), on_unbounded="keep")
    agent.gather_rollout()
    torch.cuda.synchronize()
    c, buf = agent.crmdp, agent._buffers
    memory = S.CRMDPMemory(agents, agent.metric, agent.device)
    out = {k: c[k] for k in ("rewards_out", "order", "n_corrupt", "safe_index", "unbounded")}

    def clear():
        memory.flag.zero_(), memory.reward.zero_(), memory.bound.fill_(-2 ** 31)

    def keys():
        crmdp.crmdp_keys(env, buf["states"], c["last_boards"], c["keys"])

    def filt():
        crmdp.crmdp_filter(env, c["keys"], buf["rewards"], buf["lengths"], memory, out)

    return env, agent, memory, clear, keys, filt


def run_trace(n, agents):
    torch, S = _import()
    env, agent, memory, clear, keys, filt = _setup(torch, S, n, agents)
    for _ in range(ROUNDS + 1):
        clear()
        keys()
        filt()
    torch.cuda.synchronize()
    env.close()


def run_shape(n, agents, log):
    import ctypes

    import numpy as np

    torch, S = _import()
    from safe_grid_agents_amd import _lib, crmdp

    env, agent, memory, clear, keys, filt = _setup(torch, S, n, agents)
    twin_env = S.BatchedGridworldEnv("BoatRace-v0", n, seed=5)
    twin_env.bind_torch_stream()
    torch.manual_seed(5)
    twin = S.BatchedPPOAgent(twin_env, _args(n), body="cnn")
    twin.gather_rollout()
    c, buf = agent.crmdp, agent._buffers
    # the host call on the same inputs, one core
    per = n // agents
    m = max(per, min(n, HOST_CAP) // per * per)  # whole agents
    h_keys, h_rewards = c["keys"][:m].cpu().numpy(), buf["rewards"][:m].cpu().numpy()
    h_lengths = buf["lengths"][:m].cpu().numpy().astype(np.int32)
    h_out = {"rewards_out": np.zeros((m, T), np.float32), "order": np.zeros((m, T), np.int32), "n_corrupt": np.zeros(m, np.int32),
             "safe_index": np.zeros(m, np.int32), "unbounded": np.zeros(m, np.int32)}
    h_mem = {"mem_flag": np.zeros((m // per, 625), np.uint8), "mem_reward": np.zeros((m // per, 625), np.int32),
             "mem_rllb": np.full((m // per, 625), -2 ** 31, np.int32)}
    h_buf = _lib.SgkCrmdpBuffers(**{k: v.ctypes.data for k, v in {**h_out, **h_mem}.items()})

    def host():
        h_mem["mem_flag"][:], h_mem["mem_reward"][:], h_mem["mem_rllb"][:] = 0, 0, -2 ** 31
        t0 = time.perf_counter()
        _lib.check(_lib.load().sgk_crmdp_filter_host(h_keys.ctypes.data, h_rewards.ctypes.data, h_lengths.ctypes.data, m, T, m // per,
                                                     ctypes.byref(agent.metric), ctypes.byref(h_buf)))
        return 1e6 * (time.perf_counter() - t0) * (n / m)

    t_keys, t_filter, t_host, t_gather, t_plain = [], [], [], [], []
    for rnd in range(ROUNDS + 1):
        clear()
        k, f, h = _events(torch, keys), _events(torch, filt), host()
        if rnd == 0:  # the device call left the host call's bytes (the trajectories the host call ran)
            assert c["rewards_out"][:m].cpu().numpy().tobytes() == h_out["rewards_out"].tobytes()
            assert c["n_corrupt"][:m].cpu().numpy().tobytes() == h_out["n_corrupt"].tobytes()
        g = _events(torch, agent.gather_rollout) if agents == 1 else 0.0
        p = _events(torch, twin.gather_rollout) if agents == 1 else 0.0
        if rnd:
            t_keys.append(k); t_filter.append(f); t_host.append(h); t_gather.append(g); t_plain.append(p)
    marked = int((c["n_corrupt"] > 0).sum())
    line = ("BoatRace N=%6d x %d steps, %5d agent(s) of %5d trajectories (%d trajectories mark something): keys %.1f us [%.1f .. %.1f]; "
            "filter (detect + merge) %.1f us [%.1f .. %.1f]; sgk_crmdp_filter_host on one core %.0f us [%.0f .. %.0f]%s -> %.0fx the device filter"
            % ((n, T, agents, per, marked) + _med(t_keys) + _med(t_filter) + _med(t_host)
               + (" (run on %d trajectories, scaled)" % m if m < n else "", _med(t_host)[0] / _med(t_filter)[0])))
    if agents == 1:
        g, p = _med(t_gather), _med(t_plain)
        line += ("; gather_rollout with the filter %.0f us [%.0f .. %.0f] against BatchedPPOAgent's %.0f us [%.0f .. %.0f] = %+.1f%%"
                 % (g + p + (100.0 * (g[0] - p[0]) / p[0],)))
    print(line, flush=True)
    log.write(line + "\n")
    env.close(); twin_env.close()


if __name__ == "__main__":
    rest = [v for v in sys.argv[1:] if not v.startswith("--")]
    if "--trace" in sys.argv:
        run_trace(int(rest[0]), int(rest[1]))
        sys.exit(0)
    if "--shape" in sys.argv:
        with open(rest[2], "a") as log:
            run_shape(int(rest[0]), int(rest[1]), log)
        sys.exit(0)
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "crmdp", "bench_crmdp.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_crmdp.py -- us by device events (the host call: wall clock), median [min .. max] of %d alternating rounds "
                  "after a warm-up round, one process per shape\n" % ROUNDS)
    for n in SIZES:  # (this process never touches the GPU: each shape is a child of its own)
        for agents in (1, n // 8):
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shape", str(n), str(agents), out])
            if rc != 0:
                sys.exit(rc)
