"""A population of independent Deep-Q agents (BatchedDeepQPopulation) per member count: one learn_batch() -- sgk_dqn_sgd_step_members:
dqn_sgd_kernel with a workgroup per member, then dqn_adam_kernel over n_members x ceil(P / 256) workgroups -- against the same M learners
as M sequential sgk_dqn_sgd_step calls in the same process, and a whole lockstep step() (act, store, learn, reset-store).

BoatRace and SideEffectsSokoban, E = 8 envs per member, H = 100, batch 64, a ring of 8 slices, M in {1, 16, 256, 1024}. Times are host
clocks around work that ends in a device synchronise, the median of REPS windows of CALLS back-to-back calls each, after a warm-up
window. The two kernels' own times come from a kernel trace taken in runs of their own (one per level and M):

    python tools/bench_dqn_members.py [LOG]             the table (default LOG: profiles/dqn_members/bench_dqn_members.log)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_dqn_members.py --trace ENV M
    python tools/bench_dqn_members.py --kernels DIR ENV M   one line from that trace: the SGD and the Adam kernel, separately
    python tools/bench_dqn_members.py --existing        the paths that were there before: sgk_dqn_sgd_step alone and BASELINE config 4's
                                                        learning step (uses nothing the population added: runs on the parent commit)
"""
import csv
import glob
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
    sys.path.insert(0, p)

ENVS = ("BoatRace-v0", "SideEffectsSokoban-v0")
MEMBERS = (1, 16, 256, 1024)
E, HIDDEN, BATCH, SLICES = 8, 100, 64, 8
REPS, CALLS = 7, 1000


def args_():
    return types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=BATCH, sync_every=10000, epsilon=0.01, epsilon_anneal=100000,
                                 n_layers=2, n_hidden=HIDDEN, seed=5)


def timed(torch, fn, calls=CALLS):
    """Median and spread, in us per call, over REPS windows of `calls` calls ending in a synchronise (after one warm-up window)."""
    out = []
    for rep in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(1e6 * (time.perf_counter() - t0) / calls)
    out = out[1:]
    return statistics.median(out), min(out), max(out)


def population(S, name, members):
    env = S.BatchedGridworldEnv(name, members * E, seed=5)
    env.bind_torch_stream()
    pop = S.BatchedDeepQPopulation(env, args_(), members, replay_slices=SLICES)
    pop.warmup(SLICES)
    env.reset()
    return env, pop


def member_learner(_lib, pop, ring, m):
    """The sgk_dqn_learner of member m ALONE: pointers at its slices of the stacked tensors, a ring of E env columns."""
    L = _lib.SgkDqnLearner()
    for k, t in ring.items():
        setattr(L, k, t.data_ptr())
    L.slices_filled, L.n_hidden, L.batch, L.loss_mode = SLICES, HIDDEN, BATCH, _lib.DQN_LOSS_REFERENCE
    for i, k in enumerate(("w1", "b1", "w2", "b2", "w3", "b3")):
        setattr(L, k, pop.cur[k][m].data_ptr())
        L.m[i], L.v[i], L.vmax[i] = pop.adam_m[i][m].data_ptr(), pop.adam_v[i][m].data_ptr(), pop.adam_vmax[i][m].data_ptr()
    L.w1t, L.w2t, L.w3t = (pop.cur_t[k][m].data_ptr() for k in ("w1t", "w2t", "w3t"))
    tg, tt = pop.target, pop.target_t
    L.tw1t, L.tb1, L.tw2t, L.tb2, L.tw3, L.tb3 = (tt["w1t"][m].data_ptr(), tg["b1"][m].data_ptr(), tt["w2t"][m].data_ptr(),
                                                  tg["b2"][m].data_ptr(), tg["w3"][m].data_ptr(), tg["b3"][m].data_ptr())
    L.step, L.loss_out = pop.step_count[m:m + 1].data_ptr(), pop.loss[m:m + 1].data_ptr()
    L.lr, L.beta1, L.beta2, L.eps, L.discount, L.max_grad_norm = pop.lr, 0.9, 0.999, 1e-8, pop.discount, 10.0
    return L


def run(torch, S, _lib, name, members, log):
    import ctypes

    env, pop = population(S, name, members)
    learn = timed(torch, pop.learn_batch)
    step = timed(torch, lambda: pop.step(learn=True), calls=200)
    one = S.BatchedGridworldEnv(name, E, seed=5)
    one.bind_torch_stream()
    ring = {k: getattr(pop.replay, k)[:, :E].contiguous() for k in ("states", "successors", "actions", "rewards", "terminals")}
    singles = [member_learner(_lib, pop, ring, m) for m in range(members)]

    def sequential():
        for L in singles:
            _lib.check(one.lib.sgk_dqn_sgd_step(one._h.ptr, ctypes.byref(L)))

    sequential()
    seq = timed(torch, sequential, calls=max(2, CALLS // members))
    line = ("%s M=%4d (N=%5d envs): learn_batch %.1f us [%.1f .. %.1f], %d sequential sgk_dqn_sgd_step %.1f us [%.1f .. %.1f] = %.1fx "
            "the members call, step() %.1f us [%.1f .. %.1f]" % ((name, members, members * E) + learn + (members,) + seq + (seq[0] / learn[0],) + step))
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()
    env.close()
    one.close()


def trace(torch, S, name, members):
    env, pop = population(S, name, members)
    for _ in range(60):
        pop.learn_batch()
    torch.cuda.synchronize()
    env.close()


def kernels(directory, name, members):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    parts = []
    for kernel in ("dqn_sgd_kernel", "dqn_adam_kernel"):
        hit = [r for r in rows if kernel + "<" in r["Name"]]
        if not hit:
            raise SystemExit("no %s in the trace under %s" % (kernel, directory))
        r = hit[0]
        parts.append("%s %.1f us [%.1f .. %.1f] over %s calls" % (kernel, float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3,
                                                                   float(r["MaxNs"]) / 1e3, r["Calls"]))
    print("%s M=%4d kernel trace (average [min .. max]): %s" % (name, members, ", ".join(parts)), flush=True)


def existing(torch, S, _lib):
    """sgk_dqn_sgd_step alone (one BatchedDeepQAgent, E envs, the shapes above) and BASELINE config 4's learning step (Sokoban, 32 768
    envs, the captured lockstep iteration)."""
    for name in ENVS:
        env = S.BatchedGridworldEnv(name, E, seed=5)
        env.bind_torch_stream()
        torch.manual_seed(5)
        agent = S.BatchedDeepQAgent(env, args_(), replay_slices=SLICES)
        assert agent.fused_learn
        agent.warmup(SLICES)
        t = timed(torch, agent._learn_batch_fused)
        print("%s sgk_dqn_sgd_step (E=%d, H=%d, batch %d): %.1f us [%.1f .. %.1f]" % ((name, E, HIDDEN, BATCH) + t), flush=True)
        env.close()
    env = S.BatchedGridworldEnv("SideEffectsSokoban-v0", 32768, seed=5)
    env.bind_torch_stream()
    torch.manual_seed(5)
    agent = S.BatchedDeepQAgent(env, args_(), replay_slices=SLICES)
    agent.warmup(SLICES)
    env.reset()
    t = timed(torch, lambda: agent.step(learn=True), calls=300)
    print("config 4 learning step, eager (Sokoban, 32768 envs): %.1f us [%.1f .. %.1f]" % t, flush=True)
    agent.enable_graphs(learn=True)
    t = timed(torch, lambda: agent.step_graphed(learn=True), calls=300)
    print("config 4 learning step, one hipGraph (Sokoban, 32768 envs): %.1f us [%.1f .. %.1f]" % t, flush=True)
    env.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--kernels"]:
        kernels(argv[1], argv[2], int(argv[3]))
        sys.exit(0)
    import torch

    import safe_grid_agents_amd as S
    from safe_grid_agents_amd import _lib

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if argv[:1] == ["--trace"]:
        trace(torch, S, argv[1], int(argv[2]))
    elif argv[:1] == ["--existing"]:
        existing(torch, S, _lib)
    else:
        out = argv[0] if argv else os.path.join(ROOT, "profiles", "dqn_members", "bench_dqn_members.log")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as log:
            log.write("# python tools/bench_dqn_members.py -- %s, torch %s\n" % (torch.cuda.get_device_name(0), torch.__version__))
            log.write("# E = %d envs per member, H = %d, batch %d, ring of %d slices; us per call: median [min .. max] of %d windows\n"
                      % (E, HIDDEN, BATCH, SLICES, REPS))
            for name in ENVS:
                for members in MEMBERS:
                    run(torch, S, _lib, name, members, log)
