"""Time mp_rrtnh_plan on the driver shape of PathPlanning/RRTNonholonomic/main.jl: 10 000 samples, rrt_star, bias
0.2, buffer 100, the 120 x 120 field with obstacle field 53, start pose (0, 0, 0), goal (120, 120); B = 1, 64 and
256 trees (every tree its own seed).  Per B: --warmup untimed calls, then --runs calls timed by the library's HIP
events around rrtnh_plan_kernel (mp_ctx_kernel_timing) and by the host clock around the whole call, which ends
with a stream synchronisation (copies included).  For context only, mp_rrt_plan (the Euclidean planner, its own
settings otherwise) is timed at the same n_iter and B in the same run.  Prints one JSON line per B as it finishes
and one summary line; --out FILE also writes the summary (profiles/)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motionplanning_amd import rrt, rrt_nonholonomic as nh  # noqa: E402
from motionplanning_amd.context import default_context  # noqa: E402

COUNTERS = ["rejected_bound", "rejected_kinematics", "rejected_circle", "rewired", "capped", "in_range",
            "drew_ang_ratio", "radius_below_cap"]


def field53():
    """Obstacle field 53 of Scenarios/obstacle_field.mat (tests/golden/obstacle_fields_64.npz keeps the first 64
    fields in MPPI's frame: x' = x / 1.2 + 10, y' = (y - 60) / 3, r' = r / 3)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "obstacle_fields_64.npz"))
    c = z["circles"][52][: int(z["count"][52])]
    return [[(x - 10.0) * 1.2, 3.0 * y + 60.0, 3.0 * r] for x, y, r in c]


def timed(ctx, call, warmup, runs):
    """(kernel ms per run, whole-call ms per run) of call()."""
    for _ in range(warmup):
        call()
    ctx.check(ctx.lib.mp_ctx_kernel_timing(ctx.handle, 1))
    kern, wall = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
        ctx.check(ctx.lib.mp_ctx_kernel_ms(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)))
        assert cnt.value == 1, cnt.value
        kern.append(ms.value)
    ctx.check(ctx.lib.mp_ctx_kernel_timing(ctx.handle, 0))
    return kern, wall


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 256])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-rrt", action="store_true", help="skip the mp_rrt_plan context rows")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = default_context(0)
    obs = field53()
    rows = []
    for B in a.batches:
        ss = []
        for b in range(B):
            s = nh.defineRRT(a.iters, [0.0, 0.0], 0.0, [120.0, 120.0], 0.0, 100, [0, 120, 0, 120], True, 0.2, seed=b)
            nh.defineRRTobs_(s, obs)
            ss.append(s)
        uni = np.stack([np.random.default_rng(b).random((a.iters, 6)) for b in range(B)])
        kern, wall = timed(ctx, lambda: nh.plan_batch(ss, ctx=ctx, uniforms=uni), a.warmup, a.runs)
        cn = np.array([s.r.counters for s in ss])
        row = {"B": B, "iters": a.iters, "kernel_ms_median": median(kern), "kernel_ms_runs": kern,
               "call_ms_median": median(wall), "call_ms_runs": wall,
               "us_per_iteration": 1e3 * median(kern) / a.iters,
               "solved": int(sum(s.r.status == "Solved" for s in ss)),
               "nodes_mean": float(np.mean([s.r.n_nodes for s in ss])),
               "counters_mean": {k: float(cn[:, i].mean()) for i, k in enumerate(COUNTERS)},
               "best_cost_tree0": ss[0].r.cost}
        if not a.no_rrt:
            es = []
            for b in range(B):
                s = rrt.defineRRT(a.iters, [0.0, 0.0], [120.0, 120.0], 100, [0, 120, 0, 120], True, 0.2, seed=b)
                rrt.defineRRTobs_(s, obs)
                es.append(s)
            kern, wall = timed(ctx, lambda: rrt.plan_batch(es, uniforms=uni[:, :, :3].copy(), ctx=ctx), a.warmup, a.runs)
            row["mp_rrt_plan_context"] = {"kernel_ms_median": median(kern), "call_ms_median": median(wall),
                                          "us_per_iteration": 1e3 * median(kern) / a.iters,
                                          "nodes_mean": float(np.mean([s.r.n_nodes for s in es]))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"workload": "RRTNonholonomic/main.jl driver shape: rrt_star, bias 0.2, buffer 100, field 53, "
                       "(0,0,0) -> (120,120)", "warmup": a.warmup, "runs": a.runs, "rows": rows}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
