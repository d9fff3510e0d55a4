"""The hashed levels' consensus by board key (hash_consensus = sgk_tabq_hash_consensus, load_shared_hash_table =
sgk_tabq_hash_load_shared) per shape, TomatoWatering:
    322 agents x 64 slots (99 steps: the tests' run); 16 384 x 1 024 at about 40 % fill; 65 536 x 256 half full (604 MB),
device events around whole calls on the handle's stream, ROUNDS alternating rounds after a warm-up round, one process per shape.
The vote against two things measured in the same process:
  floor        a plain read of the same key and row bytes: torch `sum` over the table and over the keys
  composed     what a user has today, in torch: vote codes from the permuted table view, `unique` of the voting keys,
               `searchsorted` for the ranks, `scatter_add_` of the one-hot votes (its result is checked against the call's)
The load (every agent; the vote's first capacity / 2 keys with their counts as rows, so the tables end half full and no key is dropped --
a list LONGER than the capacity costs a full probe of the table per dropped key, see include/sgk.h) against `zero_()` of the same
table and key bytes.

    python tools/bench_hash_consensus.py [LOG]   (default LOG: profiles/hash_consensus/bench_hash_consensus.log)
  --shape N CAP FILL LOG   one shape, appended to LOG (what the driver starts); FILL: the fullest table's fill to roll out to, in percent,
                           or `steps99`
  --hot N CAP STEPS        the vote alone, 20 times, for `rocprofv3 --kernel-trace --stats` in a run of its own
  --existing LOG           sgk_tabq_rollout on TomatoWatering (16 384 agents, capacity 4 096, 100 steps per call), appended to LOG. Runs
                           with either library (SGK_LIB_PATH=<the parent commit's libsgk.so>: the symbols this commit adds are not
                           bound then), so alternating parent / branch runs are the A/B of the existing path
                           (profiles/hash_consensus/ab_existing_paths.log)."""
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((322, 64, "steps99"), (16384, 1024, "40"), (65536, 256, "50"))
ROUNDS, NAME = 5, "TomatoWatering-v0"
NEW_SYMBOLS = ("sgk_tabq_hash_consensus_workspace_bytes", "sgk_tabq_hash_consensus", "sgk_tabq_hash_load_shared",
               "sgk_tabq_hash_consensus_host", "sgk_tabq_hash_load_shared_host")


def _import():
    for p in (ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
        sys.path.insert(0, p)
    import torch

    from safe_grid_agents_amd import _lib

    if "--existing" in sys.argv and os.environ.get("SGK_LIB_PATH"):  # an older library: bind what it has
        for name in NEW_SYMBOLS:
            _lib._SIGNATURES.pop(name, None)
    import safe_grid_agents_amd as S

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    return torch, S


def _make(S, n, cap):
    env = S.BatchedGridworldEnv(NAME, n, seed=5)
    env.bind_torch_stream()
    return env, S.BatchedTabularQAgent(env, types.SimpleNamespace(lr=0.4, discount=0.95, epsilon=0.3, epsilon_anneal=400, hash_capacity=cap))


def _fill(agent, cap, fill):
    if fill == "steps99":
        agent.rollout(99, kernel="hbm")
        return 99
    steps = 0
    while True:
        agent.rollout(100, kernel="hbm")
        steps += 100
        _, used, over = agent.hash_info()
        if used * 100 >= cap * int(fill) or over or steps >= 20000:
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
    env, agent = _make(S, n, cap)
    steps = _fill(agent, cap, fill)
    keys_view = torch.as_tensor(agent.keys_host().view("int32"), device="cuda")  # (the library hands out no device view of the keys)
    table = agent.table()  # [N, cap, 4], a permuted view of the slot-major memory
    flat = table.permute(1, 0, 2)  # the memory's own order: contiguous
    K = min(n * cap, 1 << 18)
    state = {}

    def vote():
        state["cons"] = agent.hash_consensus(max_keys=K)

    def floor():
        state["sum"] = (flat.sum(), keys_view.sum())

    def composed():
        nonzero = (table != 0).any(dim=2)
        held = (keys_view != -1) & nonzero
        action = table.argmax(dim=2)  # (torch's argmax also returns the first maximum)
        voting = keys_view[held].to(torch.int64)
        uniq = torch.unique(voting)
        rank = torch.searchsorted(uniq, voting)
        votes = torch.zeros((len(uniq), 4), dtype=torch.int64, device="cuda")  # (a read-back: the composition has no other way to size it)
        votes.view(-1).scatter_add_(0, rank * 4 + action[held], torch.ones_like(rank))
        state["composed"] = (uniq, votes)

    vote(); composed()
    true_u = int(state["cons"].count.item())
    U = min(true_u, K)
    uniq, votes = state["composed"]
    assert len(uniq) == true_u and torch.equal(uniq[:U].to(torch.int32), state["cons"].keys[:U])
    assert torch.equal(votes[:U], state["cons"].votes[:U]), "the composed vote and the call disagree"
    rows = state["cons"].votes.to(torch.float64)
    load_keys = state["cons"].keys.clone()
    load_count = torch.tensor([min(true_u, K, cap // 2)], dtype=torch.int64, device="cuda")
    load_agent_env, load_agent = _make(S, n, cap)
    key_bytes = torch.empty(4 * n * cap, dtype=torch.uint8, device="cuda")
    row_bytes = torch.empty(32 * n * cap, dtype=torch.uint8, device="cuda")

    def load():
        load_agent.load_shared_hash_table(load_keys, rows, load_count)

    def zero():
        key_bytes.zero_()
        row_bytes.zero_()

    t = {k: [] for k in ("vote", "floor", "composed", "load", "zero")}
    for rnd in range(ROUNDS + 1):
        for name, fn in (("vote", vote), ("floor", floor), ("composed", composed), ("load", load), ("zero", zero)):
            v = _events(torch, fn)
            if rnd:
                t[name].append(v)
    m = {k: _med(v) for k, v in t.items()}
    used = int((keys_view != -1).sum().item())
    mb = 36.0 * n * cap / 1e6
    line = ("TomatoWatering N=%6d x %5d slots (%d steps; %d claimed slots = %.1f%%; %d voted boards, max_keys %d; keys + rows %.1f MB): "
            "hash_consensus %.1f us [%.1f .. %.1f] = %.2fx the plain read %.1f us [%.1f .. %.1f], %.2fx faster than the torch composition "
            "%.1f us [%.1f .. %.1f]; load_shared_hash_table of %d keys %.1f us [%.1f .. %.1f] = %.2fx zero_() of the same bytes %.1f us [%.1f .. %.1f]"
            % ((n, cap, steps, used, 100.0 * used / (n * cap), true_u, K, mb) + m["vote"] + (m["vote"][0] / m["floor"][0],) + m["floor"]
               + (m["composed"][0] / m["vote"][0],) + m["composed"] + (min(true_u, K, cap // 2),) + m["load"] + (m["load"][0] / m["zero"][0],) + m["zero"]))
    print(line, flush=True)
    log.write(line + "\n")
    load_agent.close(); load_agent_env.close()
    agent.close(); env.close()


def run_hot(n, cap, steps):
    torch, S = _import()
    env, agent = _make(S, n, cap)
    agent.rollout(steps, kernel="hbm")
    for _ in range(20):
        agent.hash_consensus()
    torch.cuda.synchronize()
    agent.close(); env.close()


def run_existing(log):
    torch, S = _import()
    env, agent = _make(S, 16384, 4096)
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
            log.write("# python tools/bench_hash_consensus.py --existing -- library %s; us per call by device events: median [min .. max] of %d rounds\n"
                      % ("the parent commit's libsgk.so (SGK_LIB_PATH)" if os.environ.get("SGK_LIB_PATH") else "this tree's", ROUNDS))
            run_existing(log)
        sys.exit(0)
    if "--hot" in sys.argv:
        run_hot(int(rest[0]), int(rest[1]), int(rest[2]))
        sys.exit(0)
    if "--shape" in sys.argv:
        with open(rest[3], "a") as log:
            run_shape(int(rest[0]), int(rest[1]), rest[2], log)
        sys.exit(0)
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "hash_consensus", "bench_hash_consensus.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        log.write("# python tools/bench_hash_consensus.py -- us by device events around whole calls: median [min .. max] of %d alternating rounds "
                  "after a warm-up round, one process per shape\n" % ROUNDS)
    for n, cap, fill in SHAPES:  # (this process never touches the GPU: each shape is a child of its own)
        try:  # a time limit per shape; the first failure ends the run
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shape", str(n), str(cap), fill, out], timeout=300)
        except subprocess.TimeoutExpired:
            sys.exit("shape %d x %d ran into its time limit" % (n, cap))
        if rc != 0:
            sys.exit(rc)
