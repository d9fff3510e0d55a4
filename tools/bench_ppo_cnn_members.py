"""A population of independent PPO-CNN agents (BatchedPPOCNNPopulation) per member count: gather_rollout() -- one
sgk_convq_rollout_members launch + the returns scan -- and learn() -- one sgk_ppo_cnn_epochs_members call, three launches per epoch with
a member axis on the grid -- against the same M agents as M sequential gathers (sgk_convq_rollout on a handle of E envs) and M
sequential sgk_ppo_cnn_epochs calls on the same box in the same process.

BoatRace and SideEffectsSokoban, C = 5 channels, E = 8 envs per member, batch 64, 16 epochs (the reference's ppo-cnn defaults at
`-r 8`), M in {1, 16, 256, 1024}. Times are host clocks around work that ends in a device synchronise, the median of REPS windows of
back-to-back calls, after a warm-up window.

    python tools/bench_ppo_cnn_members.py [LOG]        (default LOG: profiles/ppo_cnn_members/bench_ppo_cnn_members.log)
    python tools/bench_ppo_cnn_members.py --existing   only the single-agent calls that exist without the population (to stdout):
                                                       sgk_convq_rollout at 32 768 Sokoban envs, sgk_ppo_cnn_epochs on BoatRace
    python tools/bench_ppo_cnn_members.py --trace M    one gather + one learn of M BoatRace members and nothing else (for a kernel trace)
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

import safe_grid_agents_amd as S  # noqa: E402
from safe_grid_agents_amd import _lib  # noqa: E402

E, CHANNELS, BATCH, EPOCHS = 8, 5, 64, 16
REPS, CALLS = 7, 20
LEVELS = ("BoatRace-v0", "SideEffectsSokoban-v0")


def timed(fn, calls=CALLS, reps=REPS):
    """Median and spread, in ms per call, over `reps` windows of `calls` calls ending in a synchronise (after one warm-up window)."""
    out = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    out = out[1:]
    return statistics.median(out), min(out), max(out)


def args(rollouts=E):
    return types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=BATCH, rollouts=rollouts, epochs=EPOCHS, clipping=0.2, entropy_bonus=0.01,
                                 critic_coeff=1.0, n_layers=2, n_hidden=None, n_channels=CHANNELS, device=0, log_gradients=False, cheat=False,
                                 seed=5)


def single_agent(name, n):
    env = S.BatchedGridworldEnv(name, n, seed=5)
    env.bind_torch_stream()
    torch.manual_seed(5)
    return env, S.BatchedPPOAgent(env, args(n), body="cnn", fused_conv_learn=True)


def existing():
    """The single-agent paths as they are without a population: us per lockstep step of sgk_convq_rollout at 32 768 Sokoban envs (100
    steps per launch, auto-reset) and ms per sgk_ppo_cnn_epochs call (BoatRace, E envs, 16 epochs x 64 rows)."""
    env, agent = single_agent("SideEffectsSokoban-v0", 32768)
    steps = 100
    t = timed(lambda: env.convq_rollout(agent._cw_old, steps, CHANNELS, mode="sample", auto_reset=True), calls=5)
    print("SideEffectsSokoban-v0 sgk_convq_rollout (32768 envs, C=%d): %.2f us per lockstep step [%.2f .. %.2f]"
          % ((CHANNELS,) + tuple(1e3 * v / steps for v in t)), flush=True)
    env.close()
    env, agent = single_agent("BoatRace-v0", E)
    ro = agent.gather_rollout()
    t = timed(lambda: agent._learn_fused_cnn(ro))
    print("BoatRace-v0 sgk_ppo_cnn_epochs (E=%d, C=%d, %d epochs x %d rows): %.3f ms [%.3f .. %.3f]" % ((E, CHANNELS, EPOCHS, BATCH) + t), flush=True)
    env.close()


def member_learner(pop, ro, m, ws):
    """The sgk_ppo_cnn_learner of member m ALONE: pointers at its slices of the stacked tensors, its E trajectories as a rollout of its
    own (copies with the single-handle strides), the single learner's workspace, for sgk_ppo_cnn_epochs."""
    from safe_grid_agents_amd.ppo_cnn_population import N_OLD, PARAMS

    n, sl = pop.member_envs, slice(m * pop.member_envs, (m + 1) * pop.member_envs)
    keep = {"states": ro.states[:, sl].contiguous(), "actions": ro.actions[:, sl].contiguous(), "returns": ro.returns[sl].contiguous(),
            "lengths": ro.lengths[sl].contiguous()}
    L = _lib.SgkPpoCnnLearner()
    L.states, L.actions, L.returns, L.lengths = (keep[k].data_ptr() for k in ("states", "actions", "returns", "lengths"))
    L.horizon, L.n_channels, L.batch, L.n_epochs, L.n_trajectories = ro.actions.shape[0], CHANNELS, BATCH, EPOCHS, n
    for i, k in enumerate(PARAMS):
        L.params[i], L.m[i], L.v[i] = pop.cur[k][m].data_ptr(), pop.adam_m[i][m].data_ptr(), pop.adam_v[i][m].data_ptr()
    for i, k in enumerate(PARAMS[:N_OLD]):
        L.old_params[i] = pop.old[k][m].data_ptr()
    L.step, L.stats_out, L.workspace = pop.step[m:m + 1].data_ptr(), pop.stats[m].data_ptr(), ws.data_ptr()
    L.lr, L.beta1, L.beta2, L.eps = pop.lr, pop.betas[0], pop.betas[1], pop.adam_eps
    L.clipping, L.critic_coeff, L.entropy_bonus = pop.clipping, pop.critic_coeff, pop.entropy_bonus
    return L, keep


def population(name, members):
    env = S.BatchedGridworldEnv(name, members * E, seed=5)
    env.bind_torch_stream()
    pop = S.BatchedPPOCNNPopulation(env, args(), members)
    ro = pop.gather_rollout()
    return env, pop, ro


def run(name, members, log):
    env, pop, ro = population(name, members)
    gather = timed(pop.gather_rollout, calls=5)
    learn = timed(lambda: pop.learn(ro), calls=5 if members >= 256 else CALLS)
    ws = torch.empty(env.ppo_cnn_workspace_bytes(CHANNELS, BATCH), dtype=torch.uint8, device=pop.device)
    singles = [member_learner(pop, ro, m, ws) for m in range(members)]
    small_env, small = single_agent(name, E)  # M sequential gathers: a handle of E envs, gathered M times

    def seq_learn():
        for L, _ in singles:
            env.ppo_cnn_epochs(L)

    def seq_gather():
        for _ in range(members):
            small.gather_rollout()

    few = dict(calls=max(1, CALLS // members), reps=REPS if members < 256 else 3)
    sl, sg = timed(seq_learn, **few), timed(seq_gather, **few)
    line = ("%s M=%4d (N=%5d envs): gather %.3f ms [%.3f .. %.3f], %d sequential gathers %.3f ms [%.3f .. %.3f] = %.1fx; "
            "learn %.3f ms [%.3f .. %.3f], %d sequential sgk_ppo_cnn_epochs %.3f ms [%.3f .. %.3f] = %.1fx"
            % ((name, members, members * E) + gather + (members,) + sg + (sg[0] / gather[0],) + learn + (members,) + sl + (sl[0] / learn[0],)))
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()
    small_env.close()
    env.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if "--existing" in sys.argv[1:]:
        existing()
        sys.exit(0)
    if "--trace" in sys.argv[1:]:
        env, pop, ro = population("BoatRace-v0", int(sys.argv[sys.argv.index("--trace") + 1]))
        pop.learn(ro)
        torch.cuda.synchronize()
        env.close()
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ppo_cnn_members", "bench_ppo_cnn_members.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_ppo_cnn_members.py -- %s, torch %s\n" % (torch.cuda.get_device_name(0), torch.__version__))
        log.write("# C = %d channels, E = %d envs per member, batch %d, %d epochs; ms per call: median [min .. max] of up to %d windows\n"
                  % (CHANNELS, E, BATCH, EPOCHS, REPS))
        for name in LEVELS:
            for members in (1, 16, 256, 1024):
                run(name, members, log)
