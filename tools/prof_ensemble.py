"""Workload for `rocprofv3 --kernel-trace --stats` (no counters in the same run): the cross-product acting kernel against its lower bound.
BoatRace, H = 100; for every (M, N) of CONFIGS, in this order: 20 launches of sgk_policy_act_members_all (M members x N envs), then 20
launches of sgk_policy_act on a handle of M x N envs (the same number of forwards, one weight set) -- the two kernels alternate, so
the trace falls into runs of 20 dispatches in the order of CONFIGS.

  python tools/prof_ensemble.py --summarise DIR   reads the kernel trace under DIR and prints, per run of consecutive dispatches of one
                                                   policy kernel, the median [min .. max] duration in microseconds (the first dispatch of
                                                   a run, which pays the code object's first use, is left out)
"""
import csv
import glob
import os
import statistics
import sys

CONFIGS = ((4, 32768), (16, 32768), (64, 32768), (256, 32768), (16, 2048), (256, 2048))
LAUNCHES, HIDDEN = 20, 100


def summarise(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                if "policy_mfma_kernel" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "members_all" if ", true>" in r["Kernel_Name"] else "policy_act",
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
        members, n = CONFIGS[i // 2] if i // 2 < len(CONFIGS) else ("?", "?")
        med = statistics.median(steady)
        line = "M=%-4s N=%-6s %-12s grid %s x %s threads, %d dispatches: %.1f us [%.1f .. %.1f]" % (members, n, kind, grid[0], grid[1], len(us), med,
                                                                                                  min(steady), max(steady))
        if kind == "members_all":
            pending = med
        elif pending is not None:
            line += "   -> members_all / policy_act = %.2f" % (pending / med)
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
    for members, n in CONFIGS:
        shapes = {"w1t": (25, HIDDEN), "b1": (HIDDEN,), "w2": (HIDDEN, HIDDEN), "b2": (HIDDEN,), "w3t": (HIDDEN, 4), "b3": (4,)}
        stacked = {k: (0.3 * torch.randn((members,) + s, generator=gen)).to("cuda:0") for k, s in shapes.items()}
        env = S.BatchedGridworldEnv("BoatRace-v0", n, seed=1)
        env.bind_torch_stream()
        env.step_random(7)
        out = torch.empty((members, n), dtype=torch.uint8, device="cuda:0")
        for _ in range(LAUNCHES):
            env.policy_act_members_all(stacked, members, out=out)
        torch.cuda.synchronize()
        env.close()
        env = S.BatchedGridworldEnv("BoatRace-v0", members * n, seed=1)
        env.bind_torch_stream()
        env.step_random(7)
        single = {k: v[0] for k, v in stacked.items()}
        flat = torch.empty(members * n, dtype=torch.uint8, device="cuda:0")
        for _ in range(LAUNCHES):
            env.policy_act(single, 0.0, 0, out=flat)
        torch.cuda.synchronize()
        env.close()
