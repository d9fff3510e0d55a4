"""learn() of the two-board conv body (BatchedPPOAgent(body="cnn", transitions=True)), 16 epochs x 64 rows on BoatRace at N = 2 048 envs,
C = 5 and C = 8 channels, three ways on one gathered rollout each:
    sgk_ppo_cnn_epochs_trans   fused_transition_learn=True: three launches per epoch
    the torch hipGraph         the same two-channel agent without the keyword (the path of the parent commit: sampling, gathers, autograd
                               and Adam of every epoch replayed from one graph) -- the baseline
    sgk_ppo_cnn_epochs         the one-channel agent, fused_conv_learn=True, beside them: the tap counts predict a ratio close to 1
ROUNDS alternating rounds after a warm-up round (the torch path's warm-up records its graph), device events around whole learn() calls,
one process per shape.

    python tools/bench_transition_learn.py [LOG]    (default LOG: profiles/transition_learn/bench_transition_learn.log)
  --shape C LOG            one channel count, appended to LOG (what the driver starts)
  --existing C LOG [TREE]  sgk_ppo_cnn_epochs (the one-channel learner) alone, one line appended to LOG. TREE: a built checkout of another
                           commit whose package and library are used instead of this one's -- the parent's, for an A/B of the existing
                           path in alternating processes (profiles/transition_learn/ab_existing_paths.log); the line says which tree ran
  --trace C                sgk_ppo_cnn_epochs_trans and sgk_ppo_cnn_epochs six times each, nothing else: the body of
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_transition_learn.py --trace C`
                           (a run of its own, no counters), whose *_kernel_stats.csv rows give the three kernels' own durations
                           (profiles/transition_learn/kernel_trace.log)"""
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS, ROUNDS, EPOCHS, BATCH, N = (5, 8), 5, 16, 64, 2048


def _import(root=ROOT):
    for p in (root, os.path.join(root, "safe-grid-agents_amd")):
        sys.path.insert(0, p)
    import torch

    import safe_grid_agents_amd as S

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    return torch, S


def _args(C):
    return types.SimpleNamespace(discount=0.99, batch_size=BATCH, rollouts=N, epochs=EPOCHS, n_layers=2, n_hidden=None, n_channels=C, device=0,
                                 log_gradients=False, cheat=False, seed=5, lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01)


def _events(torch, fn):
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    fn()
    end.record()
    end.synchronize()
    return begin.elapsed_time(end)  # ms


def _med(t):
    return (statistics.median(t), min(t), max(t))


def _agents(torch, S, C, which):
    """{name: (agent, its own gathered rollout)}; every agent gathers on the one env handle, which is reset in between."""
    env = S.BatchedGridworldEnv("BoatRace-v0", N, seed=5)
    env.bind_torch_stream()
    torch.manual_seed(5)
    make = {"trans": lambda: S.BatchedPPOAgent(env, _args(C), body="cnn", transitions=True, fused_transition_learn=True),
            "graph": lambda: S.BatchedPPOAgent(env, _args(C), body="cnn", transitions=True),
            "one": lambda: S.BatchedPPOAgent(env, _args(C), body="cnn", fused_conv_learn=True)}
    out = {}
    for name in which:
        agent = make[name]()
        assert agent.fused_learn == (name != "graph") and agent.fused_conv
        env.reset()
        out[name] = (agent, agent.gather_rollout())
    return env, out


def run_shape(C, log):
    torch, S = _import()
    env, agents = _agents(torch, S, C, ("trans", "graph", "one"))
    t = {k: [] for k in agents}
    for rnd in range(ROUNDS + 1):
        for name, (agent, ro) in agents.items():
            v = _events(torch, lambda: agent.learn(ro))
            if rnd:
                t[name].append(v)
    assert agents["graph"][0]._graph is not None  # (the baseline was the replayed graph, not the eager loop)
    tr, gr, on = (_med(t[k]) for k in ("trans", "graph", "one"))
    line = ("BoatRace N=%d, %d channels, learn() of %d epochs x %d rows: sgk_ppo_cnn_epochs_trans %.3f ms [%.3f .. %.3f] against the torch "
            "hipGraph of the same two-channel agent %.3f ms [%.3f .. %.3f] = 1/%.1f; the one-channel sgk_ppo_cnn_epochs %.3f ms "
            "[%.3f .. %.3f]: two channels / one = x%.3f"
            % ((N, C, EPOCHS, BATCH) + tr + gr + (gr[0] / tr[0],) + on + (tr[0] / on[0],)))
    print(line, flush=True)
    log.write(line + "\n")
    env.close()


def run_trace(C):
    torch, S = _import()
    env, agents = _agents(torch, S, C, ("trans", "one"))
    for _ in range(ROUNDS + 1):
        for agent, ro in agents.values():
            agent.learn(ro)
    torch.cuda.synchronize()
    env.close()


def run_existing(C, log, tree=None):
    torch, S = _import(os.path.abspath(tree) if tree else ROOT)
    env, agents = _agents(torch, S, C, ("one",))
    agent, ro = agents["one"]
    t = []
    for rnd in range(ROUNDS + 1):
        v = _events(torch, lambda: agent.learn(ro))
        if rnd:
            t.append(v)
    line = ("%s: BoatRace N=%d, %d channels: sgk_ppo_cnn_epochs, %d epochs x %d rows, %.3f ms [%.3f .. %.3f]"
            % (("the tree %s" % os.path.basename(os.path.abspath(tree)) if tree else "this commit", N, C, EPOCHS, BATCH) + _med(t)))
    print(line, flush=True)
    log.write(line + "\n")
    env.close()


if __name__ == "__main__":
    rest = [v for v in sys.argv[1:] if not v.startswith("--")]
    if "--trace" in sys.argv:
        run_trace(int(rest[0]))
        sys.exit(0)
    if "--shape" in sys.argv or "--existing" in sys.argv:
        with open(rest[1], "a") as log:
            if "--shape" in sys.argv:
                run_shape(int(rest[0]), log)
            else:
                run_existing(int(rest[0]), log, *rest[2:3])
        sys.exit(0)
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "transition_learn", "bench_transition_learn.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_transition_learn.py -- ms by device events around whole learn() calls, median [min .. max] of %d "
                  "alternating rounds after a warm-up round, one process per shape\n" % ROUNDS)
    for C in CHANNELS:  # (this process never touches the GPU: each shape is a child of its own)
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shape", str(C), out])
        if rc != 0:
            sys.exit(rc)
