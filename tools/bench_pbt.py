"""The exploit / explore step of population-based training per member count: BatchedPPOPopulation.exploit_explore() -- one
sgk_members_select launch + one sgk_members_clone launch for ppo-mlp's 35 + 2 tensors -- against the same effect written with torch
ops on the device in the same process: argsort on the scores, index_select + index_copy_ per stacked tensor, the elementwise perturb.

BoatRace, E = 8 envs per member, H = 100, fraction 0.25, M in {16, 256, 1024}; then sgk_members_select alone at M = 4096 (one workgroup
ranks by counting: M^2 comparisons). Times are device events around a window of CALLS back-to-back calls, ROUNDS alternating rounds
(ours, torch, ours, ...) after a warm-up round; median [min .. max] in microseconds per call. The bytes a step moves (read + written)
over the time gives the copy's rate. Run on the GPU box:  python tools/bench_pbt.py [LOG]   (default LOG: profiles/pbt/bench_pbt.log)

  --existing LOG   instead: learn() of a BatchedPPOPopulation with member_hyper (sgk_ppo_epochs_members_hyper) at M = 1 / 16 / 256, appended
                   to LOG. Runs with either library (SGK_LIB_PATH=<the parent commit's libsgk.so>: the symbols this commit adds are not
                   bound then), so alternating parent / branch runs are the A/B of the existing path (profiles/pbt/ab_existing_paths.log).
"""
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from safe_grid_agents_amd import _lib  # noqa: E402

if "--existing" in sys.argv and os.environ.get("SGK_LIB_PATH"):  # an older library: bind what it has
    for name in ("sgk_members_select", "sgk_members_clone", "sgk_members_select_host", "sgk_members_explore_pick"):
        _lib._SIGNATURES.pop(name, None)

import safe_grid_agents_amd as S  # noqa: E402
from safe_grid_agents_amd import pbt  # noqa: E402

E, HIDDEN, FRACTION = 8, 100, 0.25
ROUNDS, CALLS = 5, 50
FACTORS = (0.8, 1.2)


def window(fn, calls=CALLS):
    """Microseconds per call of `calls` back-to-back calls between two device events."""
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return 1e3 * begin.elapsed_time(end) / calls


def alternate(fns):
    """ROUNDS alternating rounds over `fns` after one warm-up round: [(median, min, max)] in microseconds per call."""
    times = [[] for _ in fns]
    for rnd in range(ROUNDS + 1):
        for i, fn in enumerate(fns):
            t = window(fn)
            if rnd:
                times[i].append(t)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def torch_step(pop, scores, n_replace):
    """exploit_explore's effect with torch ops on the device (its own coins: torch.rand)."""
    M = pop.n_members
    order = torch.argsort(scores, descending=True, stable=True)
    src, dst = order[:n_replace], order[M - n_replace:].flip(0)
    for t in pop.pbt_tensors() + pop._pbt_hyper_tensors():
        t.index_copy_(0, dst, t.index_select(0, src))
    rows = pop.hyper["learner"].index_select(0, src)
    coin = torch.rand(n_replace, device=rows.device) < 0.5
    lr = rows[:, 0] * torch.where(coin, FACTORS[1], FACTORS[0])
    rows[:, 0] = lr.clamp(*pbt.DEFAULT_BOUNDS["lr"])
    pop.hyper["learner"].index_copy_(0, dst, rows)


def run(members, log):
    env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=5)
    env.bind_torch_stream()
    a = types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=64, rollouts=E, epochs=2, clipping=0.2, entropy_bonus=0.01,
                              critic_coeff=1.0, n_layers=2, n_hidden=HIDDEN, n_channels=5, device=0, log_gradients=False, cheat=False, seed=5)
    pop = S.BatchedPPOPopulation(env, a, members, member_hyper={})
    pop.learn(pop.gather_rollout())  # (the horizon's power table exists: it is cloned too)
    pop.sync()
    scores = torch.randn(members, dtype=torch.float64, device=pop.device)
    n_replace = int(FRACTION * members)
    tensors = pop.pbt_tensors() + pop._pbt_hyper_tensors()
    moved = 2 * n_replace * sum(t[0].numel() * t.element_size() for t in tensors)
    ours, theirs = alternate([lambda: pop.exploit_explore(scores, fraction=FRACTION), lambda: torch_step(pop, scores, n_replace)])
    src = torch.empty(members, dtype=torch.int32, device=pop.device)
    select, = alternate([lambda: env.members_select(scores, n_replace, src)])
    assert int(pop.pbt_status.cpu()[0]) == 0
    line = ("M=%4d: %d tensors, %d replaced, %.2f MB read + written; exploit_explore %.1f us [%.1f .. %.1f] = %.0f GB/s; torch ops %.1f us "
            "[%.1f .. %.1f] = %.1fx; sgk_members_select alone %.1f us [%.1f .. %.1f]"
            % ((members, len(tensors), n_replace, moved / 1e6) + ours + (moved / ours[0] / 1e3,) + theirs + (theirs[0] / ours[0],) + select))
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()
    env.close()


def run_select(members, log):
    env = S.BatchedGridworldEnv("BoatRace-v0", 4, seed=5)
    env.bind_torch_stream()
    scores = torch.randn(members, dtype=torch.float64, device="cuda:0")
    src = torch.empty(members, dtype=torch.int32, device="cuda:0")
    ours, theirs = alternate([lambda: env.members_select(scores, members // 4, src),
                              lambda: torch.argsort(scores, descending=True, stable=True)])
    line = ("M=%4d: sgk_members_select alone %.1f us [%.1f .. %.1f]; torch.argsort(stable) %.1f us [%.1f .. %.1f]" % ((members,) + ours + theirs))
    print(line, flush=True)
    log.write(line + "\n")
    env.close()


def run_existing(log):
    for members in (1, 16, 256):
        env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=5)
        env.bind_torch_stream()
        a = types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=64, rollouts=E, epochs=16, clipping=0.2, entropy_bonus=0.01,
                                  critic_coeff=1.0, n_layers=2, n_hidden=HIDDEN, n_channels=5, device=0, log_gradients=False, cheat=False, seed=5)
        pop = S.BatchedPPOPopulation(env, a, members, member_hyper={})
        ro = pop.gather_rollout()
        t, = alternate([lambda: pop.learn(ro)])
        line = "M=%3d per-member sgk_ppo_epochs_members_hyper (E=%d, H=%d, 16 epochs x 64 rows): %.1f us [%.1f .. %.1f]" % ((members, E, HIDDEN) + t)
        print(line, flush=True)
        log.write(line + "\n")
        env.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if "--existing" in sys.argv:
        with open([v for v in sys.argv[1:] if not v.startswith("--")][0], "a") as log:
            log.write("# python tools/bench_pbt.py --existing -- %s, library %s; us per call by device events: median [min .. max] of %d rounds "
                      "of %d calls\n" % (torch.cuda.get_device_name(0), "the parent commit's libsgk.so (SGK_LIB_PATH)"
                                          if os.environ.get("SGK_LIB_PATH") else "this tree's", ROUNDS, CALLS))
            run_existing(log)
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pbt", "bench_pbt.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_pbt.py -- %s, torch %s\n" % (torch.cuda.get_device_name(0), torch.__version__))
        log.write("# BoatRace-v0, ppo-mlp, E = %d envs per member, H = %d, fraction %.2f; us per call by device events: median [min .. max] of "
                  "%d alternating rounds of %d calls\n" % (E, HIDDEN, FRACTION, ROUNDS, CALLS))
        for members in (16, 256, 1024):
            run(members, log)
        run_select(4096, log)
