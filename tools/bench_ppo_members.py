"""A population of independent PPO-MLP agents (BatchedPPOPopulation) per member count: gather_rollout() -- one
sgk_policy_rollout_members launch + the returns scan -- and learn() -- one sgk_ppo_epochs_members launch, a workgroup per member --
against the same M learners as M sequential sgk_ppo_epochs launches on the same box in the same process.

BoatRace, E = 8 envs per member, H = 100, batch 64, 16 epochs (the reference's ppo-mlp defaults at `-r 8`), M in {1, 16, 256, 1024}.
Times are host clocks around work that ends in a device synchronise, the median of REPS windows of CALLS back-to-back calls each,
after a warm-up. Run on the GPU box:  python tools/bench_ppo_members.py [LOG]   (default LOG: profiles/ppo_members/bench_ppo_members.log)
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

E, HIDDEN, BATCH, EPOCHS = 8, 100, 64, 16
REPS, CALLS = 7, 20


def timed(fn, calls=CALLS):
    """Median and spread, in ms per call, over REPS windows of `calls` calls ending in a synchronise (after one warm-up window)."""
    out = []
    for rep in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    out = out[1:]
    return statistics.median(out), min(out), max(out)


def member_learner(pop, ro, m):
    """The sgk_ppo_learner of member m ALONE: pointers at its slices of the stacked tensors, its E trajectories as a rollout of its own
    (copies with the single-handle strides), for sgk_ppo_epochs."""
    n, sl = pop.member_envs, slice(m * pop.member_envs, (m + 1) * pop.member_envs)
    keep = {"states": ro.states[:, sl].contiguous(), "actions": ro.actions[:, sl].contiguous(), "returns": ro.returns[sl].contiguous(),
            "lengths": ro.lengths[sl].contiguous()}
    L = _lib.SgkPpoLearner()
    L.states, L.actions, L.returns, L.lengths = (keep[k].data_ptr() for k in ("states", "actions", "returns", "lengths"))
    L.horizon, L.n_hidden, L.batch, L.n_epochs, L.n_trajectories = ro.actions.shape[0], HIDDEN, BATCH, EPOCHS, n
    for i, k in enumerate(("w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc")):
        setattr(L, k, pop.cur[k][m].data_ptr())
        L.m[i], L.v[i] = pop.adam_m[i][m].data_ptr(), pop.adam_v[i][m].data_ptr()
    L.w1t, L.w2t = pop.cur_t["w1t"][m].data_ptr(), pop.cur_t["w2t"][m].data_ptr()
    o = pop.old
    L.ow1t, L.ob1, L.ow2t, L.ob2, L.owa, L.oba = (o[k][m].data_ptr() for k in ("w1t", "b1", "w2t", "b2", "wa", "ba"))
    L.step, L.stats_out = pop.step[m:m + 1].data_ptr(), pop.stats[m].data_ptr()
    L.lr, L.beta1, L.beta2, L.eps = pop.lr, pop.betas[0], pop.betas[1], pop.adam_eps
    L.clipping, L.critic_coeff, L.entropy_bonus = pop.clipping, pop.critic_coeff, pop.entropy_bonus
    return L, keep


def run(members, log):
    env = S.BatchedGridworldEnv("BoatRace-v0", members * E, seed=5)
    env.bind_torch_stream()
    a = types.SimpleNamespace(discount=0.99, lr=1e-3, batch_size=BATCH, rollouts=E, epochs=EPOCHS, clipping=0.2, entropy_bonus=0.01,
                              critic_coeff=1.0, n_layers=2, n_hidden=HIDDEN, n_channels=5, device=0, log_gradients=False, cheat=False, seed=5)
    pop = S.BatchedPPOPopulation(env, a, members)
    ro = pop.gather_rollout()
    gather = timed(pop.gather_rollout, calls=5)
    learn = timed(lambda: pop.learn(ro))
    singles = [member_learner(pop, ro, m) for m in range(members)]

    def sequential():
        for L, _ in singles:
            env.ppo_epochs(L)

    seq = timed(sequential, calls=max(1, CALLS // members))
    line = ("M=%4d (N=%5d envs): gather %.3f ms [%.3f .. %.3f], learn one launch %.3f ms [%.3f .. %.3f], %d sequential sgk_ppo_epochs "
            "%.3f ms [%.3f .. %.3f] = %.1fx the one launch" % ((members, members * E) + gather + learn + (members,) + seq + (seq[0] / learn[0],)))
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()
    env.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ppo_members", "bench_ppo_members.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_ppo_members.py -- %s, torch %s\n" % (torch.cuda.get_device_name(0), torch.__version__))
        log.write("# BoatRace-v0, E = %d envs per member, H = %d, batch %d, %d epochs; ms per call: median [min .. max] of %d windows\n"
                  % (E, HIDDEN, BATCH, EPOCHS, REPS))
        for members in (1, 16, 256, 1024):
            run(members, log)
