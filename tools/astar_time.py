"""Time the grid-A* heuristic of Hybrid A* on configs[3] (256 scenarios): the table build alone
(mp_ha_astar_table: 256 scenes x 121 searches, the whole call with its copies) and the plan with
use_astar = 1 next to the plan with use_astar = 0, each the median of --runs timed calls after warm-up.
Prints one JSON line; --out FILE also writes it there (profiles/)."""
import argparse
import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from motionplanning_amd import hybrid_astar as ha
from motionplanning_amd.abi import ptr
from motionplanning_amd.context import default_context


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
    off, on = ha.scenario_batch(256, seed=4), ha.scenario_batch(256, seed=4, use_astar=True)
    p = ha.params_of(off[0])
    goal = np.array([h.s.ending_states for h in off])
    walls = np.array([h.s.obstacle_list for h in off], np.float64)
    tab = np.zeros((256, 121))

    def table():
        ctx.check(ctx.lib.mp_ha_astar_table(ctx.handle, ctypes.byref(p), 256, ptr(goal), ptr(walls), ptr(tab)))

    for _ in range(4):  # warm-up, as bench.py's Hybrid A* leg (workspaces, clocks)
        ha.plan_batch(ha.scenario_batch(256, seed=5), ctx=ctx)
        ha.plan_batch(ha.scenario_batch(256, seed=5, use_astar=True), ctx=ctx)
        table()
    t_tab, r_tab = med(table, a.runs)
    t_off, r_off = med(lambda: ha.plan_batch(off, ctx=ctx), a.runs)
    t_on, r_on = med(lambda: ha.plan_batch(on, ctx=ctx), a.runs)
    out = {"workload": "scenario_batch(256, seed=4), one MI355X", "runs": a.runs,
           "table_build_ms": t_tab, "table_build_ms_runs": r_tab, "table_searches": 256 * 121,
           "plan_ms_use_astar_0": t_off, "plan_ms_use_astar_0_runs": r_off,
           "plan_ms_use_astar_1": t_on, "plan_ms_use_astar_1_runs": r_on,
           "table_share_of_use_astar_1_plan": t_tab / t_on,
           "pops_use_astar_0": int(sum(h.r.loop_count for h in off)), "pops_use_astar_1": int(sum(h.r.loop_count for h in on)),
           "max_pops_use_astar_0": int(max(h.r.loop_count for h in off)), "max_pops_use_astar_1": int(max(h.r.loop_count for h in on)),
           "found_use_astar_0": int(sum(h.r.found for h in off)), "found_use_astar_1": int(sum(h.r.found for h in on))}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
