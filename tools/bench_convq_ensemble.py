"""Ensemble acting of a ppo-cnn population per member count: evaluate_ensemble() -- per lockstep step one sgk_convq_act_members_all launch,
one sgk_members_vote launch and the env's step (+ reset_done) -- eager and replayed from its recorded graph, against the same schedule
COMPOSED from what existed before, in the same process: M sgk_convq_act launches (one per member, greedy) + torch ops for the vote
(scatter_add_ into [N, 4] counts, argmax, a cast) + env.step + reset_done.

BoatRace and Sokoban, C = 5, M in {4, 16, 64, 256} x N in {2 048, 32 768}. A call is one whole evaluation of EVAL_T - 1 + max_iterations
lockstep steps (metrics reset, env reset and the final metrics read-back included); times are device events around it, ROUNDS alternating
rounds (eager, graph, composed, eager, ...) after a warm-up round; median [min .. max] in microseconds per lockstep step. Then the acting
launch alone against its lower bound, re-measured in the same run, alternating: sgk_convq_act on a handle of M x N envs does the same
M x N forwards with ONE weight set. Run on the GPU box:  python tools/bench_convq_ensemble.py [LOG]   (default LOG:
profiles/convq_ensemble/bench_convq_ensemble.log)

  --existing LOG   instead: sgk_convq_act (epsilon-greedy) and one step / 100 steps of sgk_convq_rollout at 32 768 Sokoban envs, C = 5,
                   appended to LOG. Runs with either library (SGK_LIB_PATH=<the parent commit's libsgk.so>: the symbol this commit adds
                   is not bound then), so alternating parent / branch runs are the A/B of the existing paths
                   (profiles/convq_ensemble/ab_existing_paths.log).
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
    _lib._SIGNATURES.pop("sgk_convq_act_members_all", None)

import safe_grid_agents_amd as S  # noqa: E402

CHANNELS, EVAL_T = 5, 21
ROUNDS = 5
LEVELS = ("BoatRace-v0", "SideEffectsSokoban-v0")
BOUND_MAX_ENVS = 1 << 22  # the bound's handle holds M x N envs


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
                                 critic_coeff=1.0, n_layers=2, n_hidden=None, n_channels=CHANNELS, device=0, log_gradients=False, cheat=False,
                                 seed=5)


def _shapes(cells, C=CHANNELS):
    return {"w1": (C, 1, 3, 3), "b1": (C,), "w2": (C, C, 3, 3), "b2": (C,), "wb": (C, 1, 1, 1), "bb": (C,), "wh": (C, C, 3, 3), "bh": (C,),
            "wl": (4, C * cells), "bl": (4,)}


def _random_weights(cells, dev, seed=1):
    rng = torch.Generator().manual_seed(seed)
    return {k: ((0.05 if k == "wl" else 0.3) * torch.randn(s, generator=rng)).to(dev) for k, s in _shapes(cells).items()}


def composed_eval(env, singles, member_actions, counts, ones, actions):
    """evaluate_ensemble's schedule from the calls that existed before it."""
    def step(reset_done):
        for m, w in enumerate(singles):
            env.convq_act(w, 0.0, 0, CHANNELS, out=member_actions[m])
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


def _calls(members, n):
    return max(3, min(50, (1 << 22) // (members * n)))


def run(level, members, n, log):
    env = S.BatchedGridworldEnv(level, n, seed=5)
    env.bind_torch_stream()
    pop = S.BatchedPPOCNNPopulation(env, _args(n // members), members)
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
    vote, = alternate([lambda: env.members_vote(ma, out=actions)], calls=_calls(members, n))
    line = ("%-22s M=%3d N=%5d: us per lockstep step of %d: evaluate_ensemble %.1f [%.1f .. %.1f]; graph %.1f [%.1f .. %.1f]; composed (%d launches "
            "+ torch ops) %.1f [%.1f .. %.1f] = %.1fx eager, %.1fx graph; alone, us per launch: members_vote %.1f [%.1f .. %.1f]"
            % ((level, members, n, steps) + eager + graph + (members,) + composed + (composed[0] / eager[0], composed[0] / graph[0]) + vote))
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()
    env.close()


def run_bound(level, members, n, log):
    """The acting launch on N envs against sgk_convq_act on M x N envs -- the same number of forwards, one weight set staged per workgroup
    --, alternating in one process."""
    env = S.BatchedGridworldEnv(level, n, seed=5)
    big = S.BatchedGridworldEnv(level, members * n, seed=5)
    for e in (env, big):
        e.bind_torch_stream()
        e.step_random(5, auto_reset=True)
    dev = "cuda:%d" % env.device
    shapes = _shapes(env.n_cells)
    rng = torch.Generator().manual_seed(2)
    stacked = {k: ((0.05 if k == "wl" else 0.3) * torch.randn((members,) + s, generator=rng)).to(dev) for k, s in shapes.items()}
    w = _random_weights(env.n_cells, dev)
    ma = torch.empty((members, n), dtype=torch.uint8, device=dev)
    out = torch.empty(members * n, dtype=torch.uint8, device=dev)
    act, bound = alternate([lambda: env.convq_act_members_all(stacked, members, CHANNELS, out=ma),
                            lambda: big.convq_act(w, 0.0, 0, CHANNELS, out=out)], calls=_calls(members, n))
    spread = bound[2] - bound[1]
    inside = bound[1] - spread <= act[0] <= bound[2] + spread
    line = ("%-22s M=%3d N=%5d: sgk_convq_act at M x N = %d envs %.1f us [%.1f .. %.1f]; sgk_convq_act_members_all %.1f us [%.1f .. %.1f] = %.2fx "
            "the bound (%s the bound's [min .. max] widened by its spread)"
            % ((level, members, n, members * n) + bound + act + (act[0] / bound[0], "inside" if inside else "OUTSIDE")))
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()
    env.close()
    big.close()


def run_existing(log):
    level, n = "SideEffectsSokoban-v0", 32768
    env = S.BatchedGridworldEnv(level, n, seed=5)
    env.bind_torch_stream()
    dev = "cuda:%d" % env.device
    w = _random_weights(env.n_cells, dev)
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    t, = alternate([lambda: env.convq_act(w, 0.05, 3, CHANNELS, out=out)], calls=200)
    line = "sgk_convq_act, Sokoban, %d envs, C=%d: %.2f us [%.2f .. %.2f]" % ((n, CHANNELS) + t)
    print(line, flush=True)
    log.write(line + "\n")
    for n_steps, calls in ((1, 200), (100, 10)):
        t, = alternate([lambda: env.convq_rollout(w, n_steps, CHANNELS, mode="sample", draw_index0=7, auto_reset=True)], calls=calls)
        line = "sgk_convq_rollout, Sokoban, %d envs, C=%d, %d step(s) per call: %.2f us [%.2f .. %.2f]" % ((n, CHANNELS, n_steps) + t)
        print(line, flush=True)
        log.write(line + "\n")
    env.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if "--existing" in sys.argv:
        with open([v for v in sys.argv[1:] if not v.startswith("--")][0], "a") as log:
            log.write("# python tools/bench_convq_ensemble.py --existing -- %s, library %s; us per call by device events: median [min .. max] of "
                      "%d rounds\n" % (torch.cuda.get_device_name(0), "the parent commit's libsgk.so (SGK_LIB_PATH)"
                                      if os.environ.get("SGK_LIB_PATH") else "this tree's", ROUNDS))
            run_existing(log)
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "convq_ensemble", "bench_convq_ensemble.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_convq_ensemble.py -- %s, torch %s\n" % (torch.cuda.get_device_name(0), torch.__version__))
        log.write("# ppo-cnn population, C = %d, evaluate_ensemble(%d); by device events: median [min .. max] of %d alternating rounds\n"
                  % (CHANNELS, EVAL_T, ROUNDS))
        configs = [(level, members, n) for level in LEVELS for n in (2048, 32768) for members in (4, 16, 64, 256)]
        for level, members, n in configs:
            run(level, members, n, log)
        log.write("# the acting launch against its lower bound: the same M x N forwards through sgk_convq_act (one weight set), alternating\n")
        for level, members, n in configs:
            if members * n <= BOUND_MAX_ENVS:
                run_bound(level, members, n, log)
