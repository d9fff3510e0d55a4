"""Workload for `rocprofv3 --kernel-trace --stats` (no counters in the same run): the consensus kernels against a plain read / write of
the same bytes. For every shape of SHAPES, in this order: LAUNCHES x consensus() (sgk_tabq_consensus), LAUNCHES x a float64 sum over the
table, LAUNCHES x load_shared_table() (sgk_tabq_load_shared) into a twin, LAUNCHES x zero_() of the twin's table.
    SGK_NO_BUILD=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prof_tabq_consensus.py

  python tools/prof_tabq_consensus.py --summarise DIR   reads the kernel trace under DIR and prints, per run of consecutive dispatches of
                                                         one kernel, the median [min .. max] duration in microseconds (the first dispatch
                                                         of a run is left out), for the runs of at least LAUNCHES - 1 dispatches
"""
import csv
import glob
import os
import statistics
import sys
import types

SHAPES = (("IslandNavigation-v0", 262144), ("IslandNavigation-v0", 1024), ("SideEffectsSokoban-v0", 32768))
LAUNCHES, TRAIN_STEPS = 10, 300


def summarise(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Grid_Size_X", "?")))
    rows.sort()
    runs = []
    for start, end, name, grid in rows:
        if not runs or runs[-1][0] != (name, grid):
            runs.append(((name, grid), []))
        runs[-1][1].append((end - start) / 1e3)
    # (the shared-state vote is memset, vote, row sums in turn: its dispatches do not form runs -- the short runs between two long ones are
    # gathered per kernel and grid, in the order of the trace)
    wanted = ("tabq_vote", "tabq_voters", "tabq_load", "reduce_kernel", "fill", "Fill", "memset")
    gathered = {}

    def flush():
        for (name, grid), us in gathered.items():
            if len(us) >= LAUNCHES - 1:
                report(name, grid, us)
        gathered.clear()

    def report(name, grid, us):
        steady = us[1:] or us
        print("%-100s grid %8s threads, %3d dispatches: %.1f us [%.1f .. %.1f]" % (name[:100], grid, len(us), statistics.median(steady),
                                                                               min(steady), max(steady)))

    for (name, grid), us in runs:
        if not any(k in name for k in wanted):
            continue
        if len(us) >= LAUNCHES - 1:
            flush()
            report(name, grid, us)
        else:
            gathered.setdefault((name, grid), []).extend(us)
    flush()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
        sys.exit(0)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "safe-grid-agents_amd"))
    import torch

    import safe_grid_agents_amd as S

    args = types.SimpleNamespace(lr=0.5, discount=0.99, epsilon=0.05, epsilon_anneal=100000)
    for level, n in SHAPES:
        env, twin_env = S.BatchedGridworldEnv(level, n, seed=5), S.BatchedGridworldEnv(level, n, seed=5)
        agent, twin = S.BatchedTabularQAgent(env, args), S.BatchedTabularQAgent(twin_env, args)
        agent.rollout(TRAIN_STEPS)
        tbl, twin_tbl = agent.table().permute(1, 0, 2), twin.table().permute(1, 0, 2)
        votes = torch.empty((agent.n_states, 4), dtype=torch.int64, device=tbl.device)
        voters = torch.empty(agent.n_states, dtype=torch.int64, device=tbl.device)
        for _ in range(LAUNCHES):
            agent.consensus(votes_out=votes, voters_out=voters)
        torch.cuda.synchronize()
        for _ in range(LAUNCHES):
            tbl.sum()
        torch.cuda.synchronize()
        shared = votes.to(torch.float64)
        for _ in range(LAUNCHES):
            twin.load_shared_table(shared)
        torch.cuda.synchronize()
        for _ in range(LAUNCHES):
            twin_tbl.zero_()
        torch.cuda.synchronize()
        agent.close(); env.close(); twin.close(); twin_env.close()
