"""The two-channel conv body (a transition env's [previous board, board]) per shape, BoatRace, 5 channels, N = 32 768 and 2 048 envs:
    sgk_convq_rollout_trans   STEPS lockstep steps of {forward, Categorical draw, env.step} in one launch, both trajectory channels kept,
                              against the one-channel sgk_convq_rollout with the same outputs but prev_states
    sgk_convq_sample_trans    one forward + draw, against sgk_convq_sample
    the same step from torch  the two-channel PPOCNNAgent forward on [N, 2, 5, 5] float32 (the stacking of the two boards included) +
                              sgk_categorical_sample
ROUNDS alternating rounds after a warm-up round, device events on the handle's stream, one process per shape. The rollouts are timed
per launch and printed per lockstep step; every rollout round starts from freshly reset envs.

    python tools/bench_transition_body.py [LOG]     (default LOG: profiles/transition_body/bench_transition_body.log)
  --shape N LOG            one shape, appended to LOG (what the driver starts)
  --existing N LOG [TREE]  sgk_convq_act and sgk_convq_rollout at N Sokoban envs alone, one line appended to LOG. TREE: a built checkout
                           of another commit whose package and library are used instead of this one's -- the parent's, for an A/B of
                           the existing paths in alternating processes (profiles/transition_body/ab_existing_paths.log); the line
                           says which tree ran
  --trace N                sgk_convq_sample_trans and sgk_convq_sample six times each at N BoatRace envs, nothing else: the body of
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_transition_body.py --trace N`
                           (a run of its own, no counters), whose *_kernel_stats.csv rows give the two kernels' own durations
                           (profiles/transition_body/kernel_trace.log)"""
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, ROUNDS, STEPS, C = (32768, 2048), 5, 100, 5


def _import(root=ROOT):
    for p in (root, os.path.join(root, "safe-grid-agents_amd")):
        sys.path.insert(0, p)
    import torch

    import safe_grid_agents_amd as S

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    return torch, S


def _args(n):
    return types.SimpleNamespace(discount=0.99, batch_size=64, rollouts=n, epochs=2, n_layers=2, n_hidden=None, n_channels=C, device=0,
                                 log_gradients=False, cheat=False, seed=5, lr=1e-3, clipping=0.2, critic_coeff=1.0, entropy_bonus=0.01)


def _events(torch, fn):
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    fn()
    end.record()
    end.synchronize()
    return 1e3 * begin.elapsed_time(end)


def _med(t):
    return (statistics.median(t), min(t), max(t))


def run_shape(n, log):
    torch, S = _import()
    env = S.BatchedGridworldEnv("BoatRace-v0", n, seed=5)
    env.bind_torch_stream()
    torch.manual_seed(5)
    two = S.BatchedPPOAgent(env, _args(n), body="cnn", transitions=True)
    one = S.BatchedPPOAgent(env, _args(n), body="cnn")
    dev = two.device
    buf = {k: torch.empty((STEPS, n) + s, dtype=d, device=dev) for k, s, d in (("states", (25,), torch.int8), ("prev_states", (25,), torch.int8),
                                                                                ("actions", (), torch.uint8), ("recs", (4,), torch.int8))}
    prev = torch.zeros((n, 25), dtype=torch.int8, device=dev)
    actions = torch.empty(n, dtype=torch.uint8, device=dev)
    logits = torch.empty((n, 4), dtype=torch.float32, device=dev)
    kw = dict(mode="sample", draw_index0=0, auto_reset=False, states=buf["states"], actions=buf["actions"], recs=buf["recs"], mask_finished=True)

    def rollout_two():
        env.convq_rollout(two._cw_old, STEPS, C, prev_boards=prev, prev_states=buf["prev_states"], fresh=True, **kw)

    def rollout_one():
        env.convq_rollout(one._cw_old, STEPS, C, **kw)

    def sample_two():
        env.convq_sample(two._cw_old, 3, C, out=actions, prev_boards=prev)

    def sample_one():
        env.convq_sample(one._cw_old, 3, C, out=actions)

    def sample_torch():
        with torch.no_grad():
            cur = env.obs_f32(out=two._obs).reshape(n, 1, 5, 5)
            logits.copy_(two.net.old_policy(torch.cat((prev.to(torch.float32).reshape(n, 1, 5, 5), cur), dim=1))[0])
        env.categorical_sample(logits, 3, out=actions)

    t = {k: [] for k in ("rollout_two", "rollout_one", "sample_two", "sample_one", "sample_torch")}
    for rnd in range(ROUNDS + 1):
        for name, fn in (("rollout_two", rollout_two), ("rollout_one", rollout_one)):
            env.reset()
            v = _events(torch, fn) / STEPS
            if rnd:
                t[name].append(v)
        env.reset()
        env.step_random(7, auto_reset=True)
        prev.copy_(env.boards().reshape(n, -1))
        env.step_random(1, auto_reset=True)
        for name, fn in (("sample_two", sample_two), ("sample_one", sample_one), ("sample_torch", sample_torch)):
            v = _events(torch, fn)
            if rnd:
                t[name].append(v)
    r2, r1, s2, s1, st = (_med(t[k]) for k in ("rollout_two", "rollout_one", "sample_two", "sample_one", "sample_torch"))
    line = ("BoatRace N=%6d, %d channels: sgk_convq_rollout_trans %.2f us per lockstep step [%.2f .. %.2f] (%d steps per launch) against "
            "sgk_convq_rollout %.2f [%.2f .. %.2f] = x%.2f; sgk_convq_sample_trans %.1f us [%.1f .. %.1f] against sgk_convq_sample %.1f "
            "[%.1f .. %.1f] = x%.2f and against the torch forward + sgk_categorical_sample %.1f [%.1f .. %.1f] = 1/%.1f"
            % ((n, C) + r2 + (STEPS,) + r1 + (r2[0] / r1[0],) + s2 + s1 + (s2[0] / s1[0],) + st + (st[0] / s2[0],)))
    print(line, flush=True)
    log.write(line + "\n")
    env.close()


def run_trace(n):
    torch, S = _import()
    env = S.BatchedGridworldEnv("BoatRace-v0", n, seed=5)
    env.bind_torch_stream()
    torch.manual_seed(5)
    two = S.BatchedPPOAgent(env, _args(n), body="cnn", transitions=True)
    one = S.BatchedPPOAgent(env, _args(n), body="cnn")
    env.step_random(7, auto_reset=True)
    prev = env.boards().reshape(n, -1).clone().contiguous()
    env.step_random(1, auto_reset=True)
    actions = torch.empty(n, dtype=torch.uint8, device=two.device)
    for _ in range(ROUNDS + 1):
        env.convq_sample(two._cw_old, 3, C, out=actions, prev_boards=prev)
        env.convq_sample(one._cw_old, 3, C, out=actions)
    torch.cuda.synchronize()
    env.close()


def run_existing(n, log, tree=None):
    torch, S = _import(os.path.abspath(tree) if tree else ROOT)
    env = S.BatchedGridworldEnv("SideEffectsSokoban-v0", n, seed=5)
    env.bind_torch_stream()
    torch.manual_seed(5)
    one = S.BatchedPPOAgent(env, _args(n), body="cnn")
    actions = torch.empty(n, dtype=torch.uint8, device=one.device)
    t_act, t_roll = [], []
    for rnd in range(ROUNDS + 1):
        env.reset()
        a = _events(torch, lambda: env.convq_act(one._cw, 0.0, 0, C, out=actions))
        r = _events(torch, lambda: env.convq_rollout(one._cw_old, STEPS, C, mode="sample", auto_reset=True)) / STEPS
        if rnd:
            t_act.append(a); t_roll.append(r)
    line = ("%s: Sokoban N=%d: sgk_convq_act %.2f us [%.2f .. %.2f]; sgk_convq_rollout %.2f us per lockstep step [%.2f .. %.2f]"
            % (("the tree %s" % os.path.basename(os.path.abspath(tree)) if tree else "this commit", n) + _med(t_act) + _med(t_roll)))
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
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "transition_body", "bench_transition_body.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_transition_body.py -- us by device events, median [min .. max] of %d alternating rounds after a warm-up "
                  "round, one process per shape\n" % ROUNDS)
    for n in SIZES:  # (this process never touches the GPU: each shape is a child of its own)
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shape", str(n), out])
        if rc != 0:
            sys.exit(rc)
