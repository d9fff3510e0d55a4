"""Ensemble acting per member count: evaluate_ensemble() of a ppo-mlp population -- per lockstep step one sgk_policy_act_members_all
launch, one sgk_members_vote launch and the env's step (+ reset_done) -- eager and replayed from its recorded graph, against the same
schedule COMPOSED from what existed before, in the same process: M sgk_policy_act launches (one per member, greedy) + torch ops for the
vote (scatter_add_ into [N, 4] counts, argmax, a cast) + env.step + reset_done.

BoatRace and Sokoban, H = 100, M in {4, 16, 64, 256} x N in {2 048, 32 768}. A call is one whole evaluation of EVAL_T - 1 + max_iterations
lockstep steps (metrics reset, env reset and the final metrics read-back included); times are device events around it, ROUNDS alternating
rounds (eager, graph, composed, eager, ...) after a warm-up round; median [min .. max] in microseconds per lockstep step. Then, for
context, the acting launch alone against its lower bound measured in the same run: sgk_policy_act on a handle of M x N envs does the same
M x N forwards with ONE weight set. Run on the GPU box:  python tools/bench_ensemble.py [LOG]   (default LOG:
profiles/ensemble/bench_ensemble.log)

  --existing LOG   instead: sgk_policy_act at 32 768 envs and one step / 100 steps of sgk_policy_rollout_members at M = 16 x 128 envs,
                   appended to LOG. Runs with either library (SGK_LIB_PATH=<the parent commit's libsgk.so>: the symbols this commit adds
                   are not bound then), so alternating parent / branch runs are the A/B of the existing paths
                   (profiles/ensemble/ab_existing_paths.log).
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
    for name in ("sgk_policy_act_members_all", "sgk_members_vote", "sgk_members_vote_host"):
        _lib._SIGNATURES.pop(name, None)

import safe_grid_agents_amd as S  # noqa: E402

HIDDEN, EVAL_T = 100, 21
ROUNDS = 5
LEVELS = ("BoatRace-v0", "SideEffectsSokoban-v0")


def window(fn, calls=1):
    """Microseconds per call of `calls` back-to-back calls between two device events."""
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return 1e3 * begin.elapsed_time(end) / calls


def alternate(fns, calls=1, scale=1.0):
    """ROUNDS alternating rounds over `fns` after one warm-up round: [(median, min, max)] in microseconds per call / scale."""
    times = [[] for _ in fns]
    for rnd in range(ROUNDS + 1):
        for i, fn in enumerate(fns):
            t = window(fn, calls) / scale
            if rnd:
                times[i].append(t)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def _args(rollouts):
    return types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=64, rollouts=rollouts, epochs=2, clipping=0.2, entropy_bonus=0.01,
                                 critic_coeff=1.0, n_layers=2, n_hidden=HIDDEN, n_channels=5, device=0, log_gradients=False, cheat=False, seed=5)


def composed_eval(env, singles, member_actions, counts, ones, actions):
    """evaluate_ensemble's schedule from the calls that existed before it."""
    def step(reset_done):
        for m, w in enumerate(singles):
            env.policy_act(w, 0.0, 0, out=member_actions[m])
        counts.zero_()
        counts.scatter_add_(1, member_actions.t().to(torch.int64), ones)
        actions.copy_(counts.argmax(1))
        env.step(actions, auto_reset=False)
        if reset_done:
            env.reset_done()

    env.metrics_reset()
    env.reset()
    for _ in range(EVAL_T - 1):
        step(True)
    for _ in range(int(env.info.max_iterations)):
        step(False)
    return env.metrics()


def run(level, members, n, log):
    env = S.BatchedGridworldEnv(level, n, seed=5)
    env.bind_torch_stream()
    pop = S.BatchedPPOPopulation(env, _args(n // members), members)
    steps = EVAL_T - 1 + int(env.info.max_iterations)
    dev = pop.device
    weights = pop._ensemble_weights()
    singles = [{k: v[m] for k, v in weights.items()} for m in range(members)]
    ma = torch.empty((members, n), dtype=torch.uint8, device=dev)
    counts, ones = torch.zeros((n, 4), dtype=torch.int32, device=dev), torch.ones((n, members), dtype=torch.int32, device=dev)
    actions = torch.empty(n, dtype=torch.uint8, device=dev)
    # the three forms leave the same metrics (the composed vote breaks ties as argmax does: towards the lower action)
    want = pop.evaluate_ensemble(EVAL_T)[0].vec
    assert pop.evaluate_ensemble(EVAL_T, graph=True)[0].vec == want
    assert composed_eval(env, singles, ma, counts, ones, actions).tolist() == want
    eager, graph, composed = alternate([lambda: pop.evaluate_ensemble(EVAL_T), lambda: pop.evaluate_ensemble(EVAL_T, graph=True),
                                        lambda: composed_eval(env, singles, ma, counts, ones, actions)], scale=steps)
    calls = max(3, min(50, (1 << 24) // (members * n)))
    act, = alternate([lambda: env.policy_act_members_all(weights, members, out=ma)], calls=calls)
    vote, = alternate([lambda: env.members_vote(ma, out=actions)], calls=calls)
    line = ("%-22s M=%3d N=%5d: us per lockstep step of %d: evaluate_ensemble %.1f [%.1f .. %.1f]; graph %.1f [%.1f .. %.1f]; composed (%d launches "
            "+ torch ops) %.1f [%.1f .. %.1f] = %.1fx eager, %.1fx graph; alone, us per launch: act_members_all %.1f [%.1f .. %.1f], members_vote "
            "%.1f [%.1f .. %.1f]" % ((level, members, n, steps) + eager + graph + (members,) + composed
                                    + (composed[0] / eager[0], composed[0] / graph[0]) + act + vote))
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()
    env.close()
    return act


def run_bound(level, members, n, act, log):
    """sgk_policy_act on M x N envs: the same number of forwards, one weight set staged per workgroup."""
    env = S.BatchedGridworldEnv(level, members * n, seed=5)
    env.bind_torch_stream()
    dev = "cuda:%d" % env.device
    rng = torch.Generator().manual_seed(1)
    shapes = {"w1t": (env.n_cells, HIDDEN), "b1": (HIDDEN,), "w2": (HIDDEN, HIDDEN), "b2": (HIDDEN,), "w3t": (HIDDEN, 4), "b3": (4,)}
    w = {k: (0.3 * torch.randn(s, generator=rng)).to(dev) for k, s in shapes.items()}
    out = torch.empty(members * n, dtype=torch.uint8, device=dev)
    calls = max(3, min(50, (1 << 24) // (members * n)))
    bound, = alternate([lambda: env.policy_act(w, 0.0, 0, out=out)], calls=calls)
    line = ("%-22s M=%3d N=%5d: sgk_policy_act at M x N = %d envs %.1f us [%.1f .. %.1f]; sgk_policy_act_members_all %.1f us = %.2fx the bound"
            % ((level, members, n, members * n) + bound + (act[0], act[0] / bound[0])))
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()
    env.close()


def run_existing(log):
    env = S.BatchedGridworldEnv("BoatRace-v0", 32768, seed=5)
    env.bind_torch_stream()
    dev = "cuda:%d" % env.device
    rng = torch.Generator().manual_seed(1)
    shapes = {"w1t": (env.n_cells, HIDDEN), "b1": (HIDDEN,), "w2": (HIDDEN, HIDDEN), "b2": (HIDDEN,), "w3t": (HIDDEN, 4), "b3": (4,)}
    w = {k: (0.3 * torch.randn(s, generator=rng)).to(dev) for k, s in shapes.items()}
    out = torch.empty(32768, dtype=torch.uint8, device=dev)
    t, = alternate([lambda: env.policy_act(w, 0.05, 3, out=out)], calls=200)
    line = "sgk_policy_act, BoatRace, 32768 envs, H=%d: %.2f us [%.2f .. %.2f]" % ((HIDDEN,) + t)
    print(line, flush=True)
    log.write(line + "\n")
    env.close()
    members, E = 16, 128
    env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=5)
    env.bind_torch_stream()
    stacked = {k: (0.3 * torch.randn((members,) + s, generator=rng)).to(dev) for k, s in shapes.items()}
    for n_steps, calls in ((1, 200), (100, 20)):
        t, = alternate([lambda: env.policy_rollout_members(stacked, members, n_steps, mode="sample", draw_index0=7, auto_reset=True)], calls=calls)
        line = "sgk_policy_rollout_members, BoatRace, M=%d x %d envs, H=%d, %d step(s) per call: %.2f us [%.2f .. %.2f]" % ((members, E, HIDDEN, n_steps) + t)
        print(line, flush=True)
        log.write(line + "\n")
    env.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if "--existing" in sys.argv:
        with open([v for v in sys.argv[1:] if not v.startswith("--")][0], "a") as log:
            log.write("# python tools/bench_ensemble.py --existing -- %s, library %s; us per call by device events: median [min .. max] of %d "
                      "rounds\n" % (torch.cuda.get_device_name(0), "the parent commit's libsgk.so (SGK_LIB_PATH)"
                                    if os.environ.get("SGK_LIB_PATH") else "this tree's", ROUNDS))
            run_existing(log)
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ensemble", "bench_ensemble.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_ensemble.py -- %s, torch %s\n" % (torch.cuda.get_device_name(0), torch.__version__))
        log.write("# ppo-mlp population, H = %d, evaluate_ensemble(%d); by device events: median [min .. max] of %d alternating rounds\n"
                  % (HIDDEN, EVAL_T, ROUNDS))
        acts = {}
        for level in LEVELS:
            for n in (2048, 32768):
                for members in (4, 16, 64, 256):
                    acts[(level, members, n)] = run(level, members, n, log)
        log.write("# the acting launch against its lower bound: the same M x N forwards through sgk_policy_act (one weight set)\n")
        for (level, members, n), act in acts.items():
            if level == LEVELS[0] and members * n <= (1 << 22):
                run_bound(level, members, n, act, log)
