"""Growing the hashed Q-tables (grow_hash = sgk_tabq_hash_grow) per shape, TomatoWatering:
    16 384 agents 1 024 -> 2 048 slots at about half fill; the same with the tables full; 65 536 agents 256 -> 512 slots,
against the least traffic any implementation moves, measured in the same process: the memsets of the new arrays plus a
device-to-device copy of the old arrays' bytes (buffers made beforehand). A table can be grown once, so every round fills a fresh
handle the same way (same seed: the same tables) and grows it; ROUNDS alternating rounds after a warm-up round, device events on the
handle's stream. The window around grow_hash holds everything the call does, its two hipMalloc included -- the host allocates while
the device idles --, so a raw allocation of the same bytes is timed beside it (wall clock) and the kernel's share is stated as
window - allocation - memsets: an estimate; `rocprofv3 --kernel-trace --stats -- python tools/bench_hash_grow.py --shape ...` in a run
of its own gives the kernel alone (profiles/hash_grow/kernel_trace.log).

    python tools/bench_hash_grow.py [LOG]      (default LOG: profiles/hash_grow/bench_hash_grow.log; one process per shape)
  --shape N CAP FILL LOG   one shape, appended to LOG (what the driver starts); FILL: half | full
  --period LOG             a training period, rollout(100), with and without reserve_hash(100) in front of it (16 384 agents,
                           capacity 4 096: no growth happens, the cost is hash_info's slot count), appended to LOG
  --existing LOG           sgk_tabq_rollout on TomatoWatering (16 384 agents, capacity 4 096, 100 steps per call), appended to LOG. Runs
                           with either library (SGK_LIB_PATH=<the parent commit's libsgk.so>: the symbol this commit adds is not bound
                           then), so alternating parent / branch runs are the A/B of the existing path
                           (profiles/hash_grow/ab_existing_paths.log)."""
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((16384, 1024, "half"), (16384, 1024, "full"), (65536, 256, "half"))
ROUNDS, NAME = 5, "TomatoWatering-v0"


def _import():
    for p in (ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
        sys.path.insert(0, p)
    import torch

    from safe_grid_agents_amd import _lib

    if "--existing" in sys.argv and os.environ.get("SGK_LIB_PATH"):  # an older library: bind what it has
        _lib._SIGNATURES.pop("sgk_tabq_hash_grow", None)
    import safe_grid_agents_amd as S

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    return torch, S


def _make(S, n, cap):
    # epsilon annealed from 1.0 over 10^8 steps: random walks, which keep meeting new boards
    env = S.BatchedGridworldEnv(NAME, n, seed=5)
    env.bind_torch_stream()
    return env, S.BatchedTabularQAgent(env, types.SimpleNamespace(lr=0.4, discount=0.95, epsilon=0.3, epsilon_anneal=10**8, hash_capacity=cap))


def _fill(agent, cap, fill):
    """Rollouts of 100 steps until the fullest table is half full, or until the FIRST refusal + as long again (full: most tables at
    the capacity). Deterministic: every handle of a shape ends with the same tables. Returns the steps taken."""
    steps = 0
    while True:
        agent.rollout(100, kernel="hbm")
        steps += 100
        _, used, over = agent.hash_info()
        if (fill == "half" and used >= cap // 2) or over or steps >= 20000:
            break
    if fill == "full":
        agent.rollout(steps, kernel="hbm")
        steps *= 2
    return steps


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


def run_shape(n, cap, fill, log):
    torch, S = _import()
    dev = torch.device("cuda:0")
    old_bytes, new_bytes = 36 * n * cap, 36 * n * 2 * cap
    src, dst = torch.empty(old_bytes, dtype=torch.uint8, device=dev), torch.empty(old_bytes, dtype=torch.uint8, device=dev)
    new_keys, new_table = torch.empty(4 * n * 2 * cap, dtype=torch.uint8, device=dev), torch.empty(32 * n * 2 * cap, dtype=torch.uint8, device=dev)
    src.zero_()

    def floor():
        new_keys.fill_(0xFF)
        new_table.zero_()
        dst.copy_(src)

    def memsets():
        new_keys.fill_(0xFF)
        new_table.zero_()

    def raw_alloc():  # what the call's two hipMalloc + two hipFree cost: straight from the driver, not from torch's cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = torch.cuda.caching_allocator_alloc(4 * n * 2 * cap)
        b = torch.cuda.caching_allocator_alloc(32 * n * 2 * cap)
        torch.cuda.caching_allocator_delete(a)
        torch.cuda.caching_allocator_delete(b)
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0)

    grow, base, sets, alloc, rows, steps = [], [], [], [], 0, 0
    for rnd in range(ROUNDS + 1):
        env, agent = _make(S, n, cap)
        steps = _fill(agent, cap, fill)
        keys = agent.keys_host()
        rows = int((keys != 0xFFFFFFFF).sum())
        g = _events(torch, lambda: agent.grow_hash(2 * cap))  # (the handle follows torch's current stream: the events bracket its work)
        b = _events(torch, floor)
        s = _events(torch, memsets)
        a = raw_alloc()
        assert agent.hash_info()[0] == 2 * cap and int((agent.keys_host() != 0xFFFFFFFF).sum()) == rows
        if rnd:
            grow.append(g); base.append(b); sets.append(s); alloc.append(a)
        agent.close(); env.close()
    g, b, s, a = _med(grow), _med(base), _med(sets), _med(alloc)
    kernel = max(g[0] - a[0] - s[0], 1e-3)
    line = ("TomatoWatering N=%6d %5d -> %5d slots, %s (%d steps; %d rows = %.1f%% of the old slots; old arrays %.1f MB, new %.1f MB): grow_hash "
            "%.0f us [%.0f .. %.0f] (events around the call, allocation included); floor = memsets + copy of the old bytes %.0f us [%.0f .. %.0f] "
            "-> grow_hash = %.2fx the floor; memsets alone %.0f us [%.0f .. %.0f]; raw allocation + release of the new arrays %.0f us [%.0f .. %.0f] "
            "(wall clock); kernel ~ window - allocation - memsets = %.0f us -> %.1f GB/s of scattered 32-byte row stores (%.1f MB of rows), "
            "(grow_hash - allocation) = %.2fx the floor"
            % ((n, cap, 2 * cap, fill, steps, rows, 100.0 * rows / (n * cap), old_bytes / 1e6, new_bytes / 1e6) + g + b + (g[0] / b[0],) + s + a
               + (kernel, 32 * rows / kernel * 1e-3, 32 * rows / 1e6, max(g[0] - a[0], 0.0) / b[0])))
    print(line, flush=True)
    log.write(line + "\n")


def run_period(log):
    torch, S = _import()
    n, cap = 16384, 4096
    env, agent = _make(S, n, cap)
    agent.rollout(300, kernel="hbm")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0)

    def with_reserve():
        assert agent.reserve_hash(100) == cap
        agent.rollout(100)

    plain, reserve, info = [], [], []
    for rnd in range(ROUNDS + 1):
        p, r, i = wall(lambda: agent.rollout(100)), wall(with_reserve), wall(agent.hash_info)
        if rnd:
            plain.append(p); reserve.append(r); info.append(i)
    p, r, i = _med(plain), _med(reserve), _med(info)
    line = ("TomatoWatering N=%d capacity %d (fullest table %d slots): a period rollout(100) %.0f us [%.0f .. %.0f]; reserve_hash(100) + rollout(100) "
            "%.0f us [%.0f .. %.0f] = %+.1f%%; hash_info() alone %.0f us [%.0f .. %.0f] (wall clock, synchronised at both ends)"
            % ((n, cap, agent.hash_info()[1]) + p + r + (100.0 * (r[0] - p[0]) / p[0],) + i))
    print(line, flush=True)
    log.write(line + "\n")
    agent.close(); env.close()


def run_existing(log):
    torch, S = _import()
    env, agent = _make(S, 16384, 4096)  # (3 300 steps in all: the tables stay far from full, as in a run that is sized or grown right)
    agent.rollout(300)
    times = []
    for rnd in range(ROUNDS + 1):
        t = _events(torch, lambda: [agent.rollout(100) for _ in range(5)]) / 5
        if rnd:
            times.append(t)
    assert not agent.hash_info()[2]
    line = "sgk_tabq_rollout, 100 steps per call, TomatoWatering, 16384 agents, capacity 4096: %.1f us [%.1f .. %.1f]" % _med(times)
    print(line, flush=True)
    log.write(line + "\n")
    agent.close(); env.close()


if __name__ == "__main__":
    rest = [v for v in sys.argv[1:] if not v.startswith("--")]
    if "--existing" in sys.argv:
        with open(rest[0], "a") as log:
            log.write("# python tools/bench_hash_grow.py --existing -- library %s; us per call by device events: median [min .. max] of %d rounds\n"
                      % ("the parent commit's libsgk.so (SGK_LIB_PATH)" if os.environ.get("SGK_LIB_PATH") else "this tree's", ROUNDS))
            run_existing(log)
        sys.exit(0)
    if "--period" in sys.argv:
        with open(rest[0], "a") as log:
            run_period(log)
        sys.exit(0)
    if "--shape" in sys.argv:
        with open(rest[3], "a") as log:
            run_shape(int(rest[0]), int(rest[1]), rest[2], log)
        sys.exit(0)
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "hash_grow", "bench_hash_grow.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_hash_grow.py -- median [min .. max] of %d alternating rounds after a warm-up round, one process per shape\n" % ROUNDS)
    for n, cap, fill in SHAPES:  # (this process never touches the GPU: each shape is a child of its own)
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shape", str(n), str(cap), fill, out])
        if rc != 0:
            sys.exit(rc)
    sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__), "--period", out]))
