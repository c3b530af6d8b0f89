"""Time the three grid planners on the same scenes: B = 256 seeded 51 x 51 circle fields (40 circles each, the
shape of the Dijkstra / BreadthFirst drivers: (0, 0) -> (120, 120) on [0, 120]^2), mp_astar_plan, mp_dka_plan and
mp_bfs_plan as whole calls with their copies, each the median of --runs timed calls after warm-up, with the total
and the largest pop count per planner.  Prints one JSON line; --out FILE also writes it there (profiles/)."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from motionplanning_amd.abi import ptr
from motionplanning_amd.context import default_context

B, NX, NY = 256, 51, 51


def med(f, runs):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = default_context(0)
    r = np.random.default_rng(53)
    obs = np.ascontiguousarray(np.stack([np.c_[r.uniform(8, 112, 40), r.uniform(8, 112, 40), r.uniform(3, 9, 40)]
                                         for _ in range(B)]))
    bound = np.tile([0.0, 120.0, 0.0, 120.0], (B, 1))
    start, goal = np.zeros((B, 2)), np.full((B, 2), 120.0)
    M = NX * NY + 1
    cost, plen = np.zeros(B), np.zeros(B)
    found, pops, nn, pn = (np.zeros(B, np.int32) for _ in range(4))
    seq, path = np.zeros((B, 2 * M), np.int32), np.zeros((B, M), np.int32)
    head = (ctx.handle, B, NX, NY, ptr(bound), ptr(start), ptr(goal))
    tail = (ptr(found), ptr(pops), ptr(nn), ptr(seq), ptr(path), ptr(pn), ptr(plen))
    calls = {
        "astar": lambda: ctx.check(ctx.lib.mp_astar_plan(*head, 3, 40, ptr(obs), ptr(cost), *tail)),
        "dka": lambda: ctx.check(ctx.lib.mp_dka_plan(*head, 40, ptr(obs), ptr(cost), *tail)),
        "bfs": lambda: ctx.check(ctx.lib.mp_bfs_plan(*head, 40, ptr(obs), *tail)),
    }
    for _ in range(4):  # warm-up (workspaces, LDS attributes, clocks)
        for f in calls.values():
            f()
    out = {"workload": "256 seeded 51 x 51 circle fields (40 circles), (0, 0) -> (120, 120), one MI355X", "runs": a.runs}
    for name, f in calls.items():
        t, runs = med(f, a.runs)
        out.update({f"{name}_ms": t, f"{name}_ms_runs": runs, f"{name}_us_per_search": t * 1e3 / B,
                    f"{name}_pops": int(pops.sum()), f"{name}_max_pops": int(pops.max()),
                    f"{name}_found": int(found.sum())})
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
