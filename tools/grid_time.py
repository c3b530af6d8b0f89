"""Time the three grid planners on the same scenes: B = 256 seeded 51 x 51 circle fields (40 circles each, the
shape of the Dijkstra / BreadthFirst drivers: (0, 0) -> (120, 120) on [0, 120]^2), mp_astar_plan, mp_dka_plan and
mp_bfs_plan as whole calls with their copies, each the median of --runs timed calls after warm-up, with the total
and the largest pop count per planner.

Two more measurements of mp_grid_plan (the global-memory kernels of gridbig.hip), taken the same way:
  (a) "{planner}_global_*": the same 51 x 51 scenes with MP_GRID_FORCE_GLOBAL, beside the LDS kernels' figures above
      (what the global node tables cost at the size where both run);
  (b) "{planner}_256_*": the same circle fields on 256 x 256 grids (the same world at a 0.47 m cell), B = 256, as a
      whole call with every output ("_256_ms"), and without the pop sequence and the path ("_256_lean_ms": the
      searches, their masks and B-sized copies).
"us_per_pop" is the call divided by the longest search's pops (one search runs per CU, so the call lasts about as
long as its longest search), "ns_per_pop_all" the call divided by all pops of the batch.

Prints one JSON line; --out FILE also writes it there (profiles/)."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from motionplanning_amd.abi import ptr
from motionplanning_amd.context import default_context

B, NX, NY = 256, 51, 51
BIG = 256
FORCE_GLOBAL = 1  # MP_GRID_FORCE_GLOBAL
PLANNER = {"astar": 0, "dka": 1, "bfs": 2}  # MP_GRID_*


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
    if a.runs < 5:
        ap.error("--runs must be at least 5")
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

    def grid_call(name, flags, n, tail):
        return lambda: ctx.check(ctx.lib.mp_grid_plan(ctx.handle, PLANNER[name], flags, B, n, n, ptr(bound), ptr(start),
                                                      ptr(goal), 3, 40, ptr(obs), ptr(cost), *tail))

    MB = BIG * BIG + 1
    seq_b, path_b = np.zeros((B, 2 * MB), np.int32), np.zeros((B, MB), np.int32)
    tail_b = (ptr(found), ptr(pops), ptr(nn), ptr(seq_b), ptr(path_b), ptr(pn), ptr(plen))
    tail_lean = (ptr(found), ptr(pops), ptr(nn), None, None, None, ptr(plen))
    for name in PLANNER:
        calls[f"{name}_global"] = grid_call(name, FORCE_GLOBAL, NX, tail)
    for name in PLANNER:
        calls[f"{name}_256"] = grid_call(name, 0, BIG, tail_b)
        calls[f"{name}_256_lean"] = grid_call(name, 0, BIG, tail_lean)
    for _ in range(4):  # warm-up (workspaces, LDS attributes, clocks)
        for f in calls.values():
            f()
    out = {"workload": "256 seeded circle fields (40 circles), (0, 0) -> (120, 120) on [0, 120]^2, one MI355X: 51 x 51 "
                       "cells (LDS kernels; _global: mp_grid_plan with MP_GRID_FORCE_GLOBAL) and 256 x 256 cells (_256)",
           "runs": a.runs}
    for name, f in calls.items():
        t, runs = med(f, a.runs)
        out.update({f"{name}_ms": t, f"{name}_ms_runs": runs, f"{name}_us_per_search": t * 1e3 / B,
                    f"{name}_pops": int(pops.sum()), f"{name}_max_pops": int(pops.max()),
                    f"{name}_found": int(found.sum()), f"{name}_us_per_pop": t * 1e3 / int(pops.max()),
                    f"{name}_ns_per_pop_all": t * 1e6 / int(pops.sum())})
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
