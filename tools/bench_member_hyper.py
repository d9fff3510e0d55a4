"""Per-member hyper-parameters (member_hyper of the three populations): what the per-member read costs, and what a sweep saves.

  --existing   the shared-hyper entry points as they are called today: sgk_ppo_epochs, sgk_dqn_sgd_step (one agent), and at M = 1 / 16 /
               256 members sgk_ppo_epochs_members, sgk_dqn_sgd_step_members, sgk_ppo_cnn_epochs_members, sgk_policy_rollout_members.
               Runs with either library (SGK_LIB_PATH=<the parent commit's libsgk.so>: the symbols this commit adds are not bound then), so
               alternating parent / branch runs of this mode are the A/B of the existing paths AND the baseline of --hyper.
  --hyper      the same calls at the same shapes through sgk_*_members_hyper / sgk_policy_rollout_members_eps, every member given the shared
               value (the same arithmetic: what differs is the one per-workgroup load).
  --sweep      a 16-point lr sweep of PPO-MLP as ONE population of M = 16 (gather + learn + sync per iteration) against 16 sequential
               single-agent runs (BatchedPPOAgent: gather + learn + sync each) in the same process.
  --trace M    workload for a kernel trace: 30 shared and 30 per-member calls of the PPO-MLP and the Deep-Q learner at M members (the
               kernels' names carry the instantiation):
               SGK_NO_BUILD=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_member_hyper.py --trace M

BoatRace, E = 8 envs per member, H = 100 / C = 5, batch 64, 16 epochs, a Deep-Q ring of 8 slices. Times are host clocks around work that
ends in a device synchronise: the median [min .. max] of REPS windows of CALLS back-to-back calls, after a warm-up window.
Run on the GPU box:  python tools/bench_member_hyper.py --existing|--hyper|--sweep [LOG]
"""
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from safe_grid_agents_amd import _lib  # noqa: E402

NEW_SYMBOLS = ("sgk_ppo_epochs_members_hyper", "sgk_ppo_cnn_epochs_members_hyper", "sgk_dqn_sgd_step_members_hyper",
               "sgk_policy_rollout_members_eps", "sgk_discounted_returns_members", "sgk_discount_powers")
if "--existing" in sys.argv and os.environ.get("SGK_LIB_PATH"):  # an older library: bind what it has
    for name in NEW_SYMBOLS:
        _lib._SIGNATURES.pop(name, None)

import safe_grid_agents_amd as S  # noqa: E402

E, HIDDEN, CHANNELS, BATCH, EPOCHS, SLICES = 8, 100, 5, 64, 16, 8
REPS, CALLS = 5, 10
MEMBERS = (1, 16, 256)


def timed(fn, calls=CALLS, scale=1e3):
    """Median and spread over REPS windows of `calls` calls ending in a synchronise (after one warm-up window); ms per call by default."""
    out = []
    for rep in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(scale * (time.perf_counter() - t0) / calls)
    out = out[1:]
    return statistics.median(out), min(out), max(out)


def ppo_args(lr=1e-3):
    return types.SimpleNamespace(discount=0.99, lr=lr, batch_size=BATCH, rollouts=E, epochs=EPOCHS, clipping=0.2, entropy_bonus=0.01,
                                 critic_coeff=1.0, n_layers=2, n_hidden=HIDDEN, n_channels=CHANNELS, device=0, log_gradients=False,
                                 cheat=False, seed=5)


def dqn_args():
    return types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=BATCH, sync_every=10000, epsilon=0.05, epsilon_anneal=1000,
                                 n_layers=2, n_hidden=HIDDEN, seed=5)


def emit(log, line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def same(args, names, members):
    return {k: [getattr(args, k)] * members for k in names}


def members_calls(log, hyper):
    """The four population calls at M = 1 / 16 / 256, shared (hyper=False) or per-member with equal values (hyper=True)."""
    tag = "per-member" if hyper else "shared"
    for members in MEMBERS:
        env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=5)
        env.bind_torch_stream()
        a, d = ppo_args(), dqn_args()
        kw = lambda names, args: dict(member_hyper=same(args, names, members)) if hyper else {}  # noqa: E731
        pop = S.BatchedPPOPopulation(env, a, members, **kw(("lr", "clipping", "critic_coeff", "entropy_bonus", "discount"), a))
        ro = pop.gather_rollout()
        t = timed(lambda: pop.learn(ro))
        emit(log, "M=%3d %s sgk_ppo_epochs_members%s (E=%d, H=%d, %d epochs x %d rows): %.4f ms [%.4f .. %.4f]"
             % ((members, tag, "_hyper" if hyper else "", E, HIDDEN, EPOCHS, BATCH) + t))
        cnn = S.BatchedPPOCNNPopulation(env, a, members, **kw(("lr", "clipping", "critic_coeff", "entropy_bonus", "discount"), a))
        roc = cnn.gather_rollout()
        t = timed(lambda: cnn.learn(roc), calls=max(2, CALLS // 4))
        emit(log, "M=%3d %s sgk_ppo_cnn_epochs_members%s (E=%d, C=%d, %d epochs x %d rows): %.4f ms [%.4f .. %.4f]"
             % ((members, tag, "_hyper" if hyper else "", E, CHANNELS, EPOCHS, BATCH) + t))
        dq = S.BatchedDeepQPopulation(env, d, members, replay_slices=SLICES, **kw(("lr", "discount", "epsilon"), d))
        dq.warmup(SLICES)
        env.reset()
        t = timed(dq.learn_batch, calls=4 * CALLS, scale=1e6)
        emit(log, "M=%3d %s sgk_dqn_sgd_step_members%s (E=%d, H=%d, batch %d): %.2f us [%.2f .. %.2f]"
             % ((members, tag, "_hyper" if hyper else "", E, HIDDEN, BATCH) + t))
        w, T = dq.greedy_weights(), 100
        eps = dict(member_epsilon=torch.full((members,), 0.05, dtype=torch.float64, device=dq.device)) if hyper else {}
        t = timed(lambda: env.policy_rollout_members(w, members, T, mode="greedy", epsilon=0.05, auto_reset=True, **eps), scale=1e6 / T)
        emit(log, "M=%3d %s sgk_policy_rollout_members%s (E=%d, H=%d, mode 0, %d steps per launch): %.3f us per lockstep step [%.3f .. %.3f]"
             % ((members, tag, "_eps" if hyper else "", E, HIDDEN, T) + t))
        env.close()


def single_calls(log):
    """sgk_ppo_epochs and sgk_dqn_sgd_step: one agent on E envs."""
    env = S.BatchedGridworldEnv("BoatRace-v0", E, seed=5)
    env.bind_torch_stream()
    torch.manual_seed(5)
    agent = S.BatchedPPOAgent(env, ppo_args())
    ro = agent.gather_rollout()
    t = timed(lambda: agent._learn_fused(ro))
    emit(log, "single sgk_ppo_epochs (E=%d, H=%d, %d epochs x %d rows): %.4f ms [%.4f .. %.4f]" % ((E, HIDDEN, EPOCHS, BATCH) + t))
    dq = S.BatchedDeepQAgent(env, dqn_args(), sgd_steps=1, replay_slices=SLICES, fused_learn=True)
    dq.warmup(SLICES)
    t = timed(dq._learn_batch_fused, calls=4 * CALLS, scale=1e6)
    emit(log, "single sgk_dqn_sgd_step (E=%d, H=%d, batch %d): %.2f us [%.2f .. %.2f]" % ((E, HIDDEN, BATCH) + t))
    env.close()


def sweep(log):
    """16 learning rates: one population of 16 against 16 single agents one after the other, ITER PPO iterations each."""
    from safe_grid_agents_amd.loops import batched_ppo_learn, population_ppo_learn

    points = [1e-4 * 1.5 ** i for i in range(16)]
    iters = 10
    env = S.BatchedGridworldEnv("BoatRace-v0", 16 * E, seed=5)
    pop = S.BatchedPPOPopulation(env, ppo_args(), 16, member_hyper={"lr": points})
    singles = []
    for m, lr in enumerate(points):
        e = S.BatchedGridworldEnv("BoatRace-v0", E, seed=5, env_index_base=m * E)
        torch.manual_seed(pop.member_seeds[m] % 2 ** 63)
        singles.append((e, S.BatchedPPOAgent(e, ppo_args(lr))))

    def one_population():
        for _ in range(iters):
            population_ppo_learn(pop, env)

    def sequential():
        for e, agent in singles:
            for _ in range(iters):
                batched_ppo_learn(agent, e)

    a = timed(one_population, calls=1)
    b = timed(sequential, calls=1)
    emit(log, "16-point lr sweep, %d PPO iterations (gather + %d epochs x %d rows + sync, E=%d, H=%d): one population of 16 %.2f ms "
              "[%.2f .. %.2f]; 16 sequential single-agent runs %.2f ms [%.2f .. %.2f] = %.1fx"
         % ((iters, EPOCHS, BATCH, E, HIDDEN) + a + b + (b[0] / a[0],)))
    env.close()
    for e, _ in singles:
        e.close()


def trace(members):
    env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=5)
    env.bind_torch_stream()
    a, d = ppo_args(), dqn_args()
    for hyper in (False, True):
        kw = lambda names, args: dict(member_hyper=same(args, names, members)) if hyper else {}  # noqa: E731
        pop = S.BatchedPPOPopulation(env, a, members, **kw(("lr", "clipping", "critic_coeff", "entropy_bonus", "discount"), a))
        ro = pop.gather_rollout()
        dq = S.BatchedDeepQPopulation(env, d, members, replay_slices=SLICES, **kw(("lr", "discount", "epsilon"), d))
        dq.warmup(SLICES)
        for _ in range(30):
            pop.learn(ro)
        for _ in range(30):
            dq.learn_batch()
        torch.cuda.synchronize()
    env.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if "--trace" in sys.argv:
        trace(int(sys.argv[sys.argv.index("--trace") + 1]))
        sys.exit(0)
    modes = [m for m in ("--existing", "--hyper", "--sweep") if m in sys.argv]
    assert len(modes) == 1, "one of --existing, --hyper, --sweep"
    rest = [v for v in sys.argv[1:] if not v.startswith("--")]
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "member_hyper", "bench_member_hyper%s.log" % modes[0].replace("--", "_"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as log:
        emit(log, "# python tools/bench_member_hyper.py %s -- %s, torch %s, library %s" % (
            modes[0], torch.cuda.get_device_name(0), torch.__version__, os.environ.get("SGK_LIB_PATH") or "this tree's"))
        emit(log, "# median [min .. max] of %d windows of >= %d calls" % (REPS, CALLS))
        if modes[0] == "--existing":
            single_calls(log)
            members_calls(log, hyper=False)
        elif modes[0] == "--hyper":
            members_calls(log, hyper=True)
        else:
            sweep(log)
