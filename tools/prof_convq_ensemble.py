"""Workload for `rocprofv3 --kernel-trace --stats` (no counters in the same run): the conv bodies' cross-product acting kernel against its
lower bound. C = 5; for every (level, M, N) of CONFIGS, in this order: 20 launches of sgk_convq_act_members_all (M members x N envs), then
20 launches of sgk_convq_act (epsilon 0) on a handle of M x N envs (the same number of forwards, one weight set) -- the two kernels
alternate, so the trace falls into runs of 20 dispatches in the order of CONFIGS.

  SGK_NO_BUILD=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/prof_convq_ensemble.py
  python tools/prof_convq_ensemble.py --summarise DIR   reads the kernel trace under DIR and prints, per run of consecutive dispatches of
                                                         one conv acting kernel, the median [min .. max] duration in microseconds (the
                                                         first dispatch of a run, which pays the code object's first use, is left out)
"""
import csv
import glob
import os
import statistics
import sys

BOAT, SOKOBAN = "BoatRace-v0", "SideEffectsSokoban-v0"
CONFIGS = ((BOAT, 64, 2048), (BOAT, 16, 32768), (BOAT, 64, 32768), (SOKOBAN, 16, 2048), (SOKOBAN, 16, 32768), (SOKOBAN, 64, 32768))
LAUNCHES, CHANNELS = 20, 5


def summarise(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                if "convq_act_kernel" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "members_all" if ", true>" in r["Kernel_Name"] else "convq_act",
                                 tuple(r.get(k, "?") for k in ("Grid_Size_X", "Grid_Size_Y"))))
    rows.sort()
    runs = []
    for start, end, kind, grid in rows:
        if not runs or runs[-1][0] != (kind, grid):
            runs.append(((kind, grid), []))
        runs[-1][1].append((end - start) / 1e3)
    pending = None
    for i, ((kind, grid), us) in enumerate(runs):
        steady = us[1:] or us
        level, members, n = CONFIGS[i // 2] if i // 2 < len(CONFIGS) else ("?", "?", "?")
        med = statistics.median(steady)
        line = "%-22s M=%-4s N=%-6s %-12s grid %s x %s threads, %d dispatches: %.1f us [%.1f .. %.1f]" % (level, members, n, kind, grid[0], grid[1],
                                                                                                        len(us), med, min(steady), max(steady))
        if kind == "members_all":
            pending = med
        elif pending is not None:
            line += "   -> members_all / convq_act = %.2f" % (pending / med)
            pending = None
        print(line)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
        sys.exit(0)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "safe-grid-agents_amd"))
    import torch

    import safe_grid_agents_amd as S

    gen = torch.Generator().manual_seed(1)
    C = CHANNELS
    for level, members, n in CONFIGS:
        env = S.BatchedGridworldEnv(level, n, seed=1)
        env.bind_torch_stream()
        env.step_random(7)
        shapes = {"w1": (C, 1, 3, 3), "b1": (C,), "w2": (C, C, 3, 3), "b2": (C,), "wb": (C, 1, 1, 1), "bb": (C,), "wh": (C, C, 3, 3), "bh": (C,),
                  "wl": (4, C * env.n_cells), "bl": (4,)}
        stacked = {k: ((0.05 if k == "wl" else 0.3) * torch.randn((members,) + s, generator=gen)).to("cuda:0") for k, s in shapes.items()}
        out = torch.empty((members, n), dtype=torch.uint8, device="cuda:0")
        for _ in range(LAUNCHES):
            env.convq_act_members_all(stacked, members, C, out=out)
        torch.cuda.synchronize()
        env.close()
        env = S.BatchedGridworldEnv(level, members * n, seed=1)
        env.bind_torch_stream()
        env.step_random(7)
        single = {k: v[0] for k, v in stacked.items()}
        flat = torch.empty(members * n, dtype=torch.uint8, device="cuda:0")
        for _ in range(LAUNCHES):
            env.convq_act(single, 0.0, 0, C, out=flat)
        torch.cuda.synchronize()
        env.close()
