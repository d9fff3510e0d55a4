"""The tabular agents' consensus per shape: consensus() (sgk_tabq_consensus), load_shared_table() (sgk_tabq_load_shared) and
evaluate_consensus() on IslandNavigation at 262 144 and 1 024 agents and Sokoban at 32 768, against two baselines measured in the same
run:
  (a) the same votes COMPOSED from torch ops on table(): ne(0).any, argmax, a one-hot sum (torch's tie rule is its own: a timing baseline)
  (b) a plain device read of the same 32 * S * N bytes: a float64 sum over the table, and a device-to-device copy of it (read + write: its
      time halved stands for the read); the vote kernel is reported as a fraction of the faster of the two
and, for the load, a plain device write of the same bytes (zero_() of a table of the same size).

Times are device events around `calls` back-to-back calls, ROUNDS alternating rounds over all the legs after a warm-up round; median
[min .. max] in microseconds per call. One process per shape (started here, one after the other). Run on the GPU box:
    python tools/bench_tabq_consensus.py [LOG]            (default LOG: profiles/tabq_consensus/bench_tabq_consensus.log)

  --shape LEVEL N LOG   one shape, appended to LOG (what the driver starts)
  --existing LOG        instead: sgk_tabq_rollout (100 steps per call) and sgk_tabq_eval (evaluate_enqueue(100)) at config 3's shape,
                        IslandNavigation with 262 144 agents, appended to LOG. Runs with either library (SGK_LIB_PATH=<the parent
                        commit's libsgk.so>: the symbols this commit adds are not bound then), so alternating parent / branch runs are
                        the A/B of the existing paths (profiles/tabq_consensus/ab_existing_paths.log).
"""
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("IslandNavigation-v0", 262144), ("IslandNavigation-v0", 1024), ("SideEffectsSokoban-v0", 32768))
ROUNDS, TRAIN_STEPS, EVAL_T = 5, 300, 100


def _import():
    for p in (ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
        sys.path.insert(0, p)
    import torch

    from safe_grid_agents_amd import _lib

    if "--existing" in sys.argv and os.environ.get("SGK_LIB_PATH"):  # an older library: bind what it has
        for name in ("sgk_tabq_consensus", "sgk_tabq_load_shared", "sgk_tabq_consensus_host"):
            _lib._SIGNATURES.pop(name, None)
    import safe_grid_agents_amd as S

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    return torch, S


def _args():
    return types.SimpleNamespace(lr=0.5, discount=0.99, epsilon=0.05, epsilon_anneal=100000)


def window(torch, fn, calls):
    """Microseconds per call of `calls` back-to-back calls between two device events."""
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return 1e3 * begin.elapsed_time(end) / calls


def alternate(torch, fns, calls):
    """ROUNDS alternating rounds over `fns` after one warm-up round: [(median, min, max)] in microseconds per call."""
    times = [[] for _ in fns]
    for rnd in range(ROUNDS + 1):
        for i, fn in enumerate(fns):
            t = window(torch, fn, calls)
            if rnd:
                times[i].append(t)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def run_shape(level, n, log):
    torch, S = _import()
    env = S.BatchedGridworldEnv(level, n, seed=5)
    env.bind_torch_stream()
    agent = S.BatchedTabularQAgent(env, _args())
    agent.rollout(TRAIN_STEPS)
    twin_env = S.BatchedGridworldEnv(level, n, seed=5)  # the load's target: the source's tables stay what training left
    twin_env.bind_torch_stream()
    twin = S.BatchedTabularQAgent(twin_env, _args())
    ns = agent.n_states
    nbytes = 32 * ns * n
    tbl = agent.table().permute(1, 0, 2)  # the memory as it lies: [S][N][4], contiguous
    assert tbl.is_contiguous()
    votes = torch.empty((ns, 4), dtype=torch.int64, device=tbl.device)
    voters = torch.empty(ns, dtype=torch.int64, device=tbl.device)
    spare = torch.empty_like(tbl)
    twin_tbl = twin.table().permute(1, 0, 2)

    def composed():
        voting = tbl.ne(0).any(dim=2)
        onehot = torch.nn.functional.one_hot(tbl.argmax(dim=2), 4)
        return (onehot * voting.unsqueeze(2)).sum(dim=1)

    cons = agent.consensus(votes_out=votes, voters_out=voters)
    mine, theirs = votes.clone(), composed()
    differ = int((mine != theirs).any(dim=1).sum())  # (states where torch's argmax broke a tie otherwise)
    shared = votes.to(torch.float64)
    calls = max(3, min(200, (1 << 31) // nbytes))
    legs = [lambda: agent.consensus(votes_out=votes, voters_out=voters), composed, lambda: tbl.sum(), lambda: spare.copy_(tbl),
            lambda: twin.load_shared_table(shared), lambda: twin_tbl.zero_()]
    vote, comp, rsum, copy, load, zero = alternate(torch, legs, calls)
    ev, = alternate(torch, [lambda: agent.evaluate_consensus(EVAL_T)], max(3, calls // 8))
    read = min(rsum[0], copy[0] / 2)
    gbs = lambda us: nbytes / us * 1e-3  # noqa: E731
    line = ("%-22s N=%6d S=%4d (%.1f MB, %d calls per window): consensus %.1f us [%.1f .. %.1f] = %.0f GB/s; composed from torch ops %.1f "
            "[%.1f .. %.1f] = %.1fx (%d of %d states differ: torch's ties); plain read: sum %.1f [%.1f .. %.1f], copy / 2 %.1f -> consensus = "
            "%.2fx the plain read; load_shared_table %.1f [%.1f .. %.1f] = %.0f GB/s; zero_() of the same bytes %.1f [%.1f .. %.1f] -> load = "
            "%.2fx the plain write; evaluate_consensus(%d) on %d envs %.1f us [%.1f .. %.1f]; agreement %.4f"
            % ((level, n, ns, nbytes / 1e6, calls) + vote + (gbs(vote[0]),) + comp + (comp[0] / vote[0], differ, ns) + rsum + (copy[0] / 2, vote[0] / read)
               + load + (gbs(load[0]),) + zero + (load[0] / zero[0], EVAL_T, min(n, 1024)) + ev + (cons.agreement(),)))
    print(line, flush=True)
    log.write(line + "\n")
    agent.close(); env.close(); twin.close(); twin_env.close()


def run_existing(log):
    torch, S = _import()
    env = S.BatchedGridworldEnv("IslandNavigation-v0", 262144, seed=5)
    env.bind_torch_stream()
    agent = S.BatchedTabularQAgent(env, _args())
    agent.rollout(TRAIN_STEPS)
    roll, ev = alternate(torch, [lambda: agent.rollout(100), lambda: agent.evaluate_enqueue(100)], 5)
    for what, t in (("sgk_tabq_rollout, 100 steps per call", roll), ("sgk_tabq_eval, evaluate_enqueue(100)", ev)):
        line = "%s, IslandNavigation, 262144 agents: %.1f us [%.1f .. %.1f]" % ((what,) + t)
        print(line, flush=True)
        log.write(line + "\n")
    agent.close(); env.close()


if __name__ == "__main__":
    rest = [v for v in sys.argv[1:] if not v.startswith("--")]
    if "--existing" in sys.argv:
        with open(rest[0], "a") as log:
            log.write("# python tools/bench_tabq_consensus.py --existing -- library %s; us per call by device events: median [min .. max] of %d rounds\n"
                      % ("the parent commit's libsgk.so (SGK_LIB_PATH)" if os.environ.get("SGK_LIB_PATH") else "this tree's", ROUNDS))
            run_existing(log)
        sys.exit(0)
    if "--shape" in sys.argv:
        with open(rest[2], "a") as log:
            run_shape(rest[0], int(rest[1]), log)
        sys.exit(0)
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "tabq_consensus", "bench_tabq_consensus.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_tabq_consensus.py -- after %d training steps; by device events: median [min .. max] of %d alternating "
                  "rounds, one process per shape\n" % (TRAIN_STEPS, ROUNDS))
    for level, n in SHAPES:  # (this process never touches the GPU: each shape is a child of its own)
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shape", level, str(n), out])
        if rc != 0:
            sys.exit(rc)
