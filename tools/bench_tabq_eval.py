"""Greedy evaluation of the batched tabular-Q agents (default_eval, reference eval.py:8-56): the loop of per-step calls
(fused_eval = False: sgk_tabq_act + sgk_step + sgk_reset_done per lockstep step, issued from Python) against the one-launch form
(sgk_tabq_eval: kernel auto, and the HBM variant forced), and against agent.rollout(K) -- the fused LEARNING loop -- for the same
number of lockstep steps on the same batch: evaluation does strictly less per step (no draw, no update, no table store).

    python tools/bench_tabq_eval.py                                   # every config below, each in a process of its own
    python tools/bench_tabq_eval.py --env IslandNavigation-v0 --n 262144   # one config, in this process

Without --env the tool never touches the GPU itself: it runs each config as a child under `timeout -k 10 <limit>` and stops at the
first one that fails (a fault or a hang must not be followed by more GPU work). One JSON line per config: microseconds per lockstep
step (median of --repeats runs after a warm-up) and the ratios. Timing: a pair of HIP events recorded on torch's current stream --
which is the stream the library enqueues on, because the env follows torch's current stream (its default, `stream="torch"`).
What each figure covers: the two evaluations are whole calls -- metrics_reset + reset + the steps + the host read-back of the 16
metric words (a stream wait) --, the learning rollout is reset + the one launch and no read-back: the comparison against the
rollout is slightly against the evaluation, which shows at 1 024 agents, where a whole call is a few hundred microseconds."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
    sys.path.insert(0, p)

CONFIGS = [("IslandNavigation-v0", 262144), ("IslandNavigation-v0", 65536), ("IslandNavigation-v0", 1024),
           ("SideEffectsSokoban-v0", 32768)]


def one(name, n, eval_timesteps, train_steps, repeats):
    import torch

    import safe_grid_agents_amd as S

    args = types.SimpleNamespace(lr=0.5, discount=0.99, epsilon=0.01, epsilon_anneal=100000)
    env = S.BatchedGridworldEnv(name, n, seed=0x5AFE)
    agent = S.BatchedTabularQAgent(env, args)
    agent.rollout(train_steps)
    steps = max(eval_timesteps - 1, 0) + int(env.info.max_iterations)

    def timed(fn, reps):
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / steps)  # us per lockstep step
        return out

    def loop_of_calls():
        agent.fused_eval = False
        return S.batched_default_eval(agent, env, eval_timesteps)

    def fused(kernel):
        agent.fused_eval = True
        return lambda: agent.evaluate(eval_timesteps, kernel=kernel)

    def learn():
        env.reset()
        agent.rollout(steps)

    episodes = {loop_of_calls().episodes, fused("auto")().episodes, fused("hbm")().episodes}  # (also the warm-up)
    if len(episodes) != 1:
        raise SystemExit("the three evaluations disagree: %r episodes" % sorted(episodes))
    res = {"env": name, "n_agents": n, "eval_timesteps": eval_timesteps, "lockstep_steps": steps, "repeats": repeats,
           "episodes_per_evaluation": episodes.pop()}
    runs = {"loop_of_calls": timed(loop_of_calls, repeats), "fused_auto": timed(fused("auto"), repeats),
            "fused_hbm": timed(fused("hbm"), repeats)}
    learn()  # warm-up
    runs["learning_rollout"] = timed(learn, repeats)  # (last: it moves the tables)
    med = {k: statistics.median(v) for k, v in runs.items()}
    res["us_per_step"] = {k: round(v, 4) for k, v in med.items()}
    res["us_per_step_min_max"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in runs.items()}
    res["loop_over_fused_auto"] = round(med["loop_of_calls"] / med["fused_auto"], 2)
    res["loop_over_fused_hbm"] = round(med["loop_of_calls"] / med["fused_hbm"], 2)
    res["fused_auto_over_learning_rollout"] = round(med["fused_auto"] / med["learning_rollout"], 3)
    res["fused_hbm_over_learning_rollout"] = round(med["fused_hbm"] / med["learning_rollout"], 3)
    agent.close(); env.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env")
    ap.add_argument("--n", type=int)
    ap.add_argument("--eval-timesteps", type=int, default=2000)
    ap.add_argument("--train-steps", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each config's process may take")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    if a.env:
        if not a.n:
            ap.error("--env needs --n")
        one(a.env, a.n, a.eval_timesteps, a.train_steps, a.repeats)
        return 0
    for name, n in CONFIGS:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--env", name, "--n", str(n),
               "--eval-timesteps", str(a.eval_timesteps), "--train-steps", str(a.train_steps), "--repeats", str(a.repeats)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("bench_tabq_eval: %s x %d ended with status %d; nothing more is started" % (name, n, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
