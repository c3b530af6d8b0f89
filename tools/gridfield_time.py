"""Time mp_grid_field (goal-distance fields, motionplanning_amd/csrc/gridfield.hip) on one MI355X:

  circle_256, circle_2048   the first circle field of tools/grid_time.py (40 seeded circles on [0, 120]^2, source (0, 0))
                            rasterised at 256 x 256 and 2048 x 2048 cells;
  serpentine_2048           the serpentine of tests/gridfield_cases.py scaled to 2048 x 1055 cells: the adversarial case of
                            a tiled scheme, a round moves the front one tile along a corridor.

For each: the relaxation rounds, the kernel time (the sum over the rounds' launches, HIP events, mp_ctx_kernel_timing) and
the whole call with its copies (field and n_reached out), the median of --runs calls after warm-up; "_every{K}_call_ms" is
the whole call when the host reads the change stamp every K rounds (MPGPU_FIELD_CHECK_EVERY) instead of every round.
On the two large maps also the walk: one query at the far end, "_walk_us_per_cell" the kernel time it adds per path cell.

The yardstick "dka_exhausted_256_*" is the only other route to the same labels: mp_grid_plan(MP_GRID_DKA), lean outputs,
with a goal off the grid on the same 256 x 256 map, so that the search runs until its open list is empty.

circle_256 is checked against the restatement of tests/gridfield_ref.py before anything is timed; whether the exhausted
search's n_nodes equals n_reached is recorded.  Prints one JSON line; --out FILE also writes it there (profiles/)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gridfield_cases as C  # noqa: E402
import gridfield_ref as F  # noqa: E402
from astar_ref import Grid  # noqa: E402
from motionplanning_amd import gridfield  # noqa: E402
from motionplanning_amd.abi import ptr  # noqa: E402
from motionplanning_amd.context import default_context  # noqa: E402

BOUND = [0.0, 120.0, 0.0, 120.0]


def med(f, runs):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def circle_mask(ctx, n):
    r = np.random.default_rng(53)  # tools/grid_time.py's scenes; the first of them
    obs = np.ascontiguousarray(np.c_[r.uniform(8, 112, 40), r.uniform(8, 112, 40), r.uniform(3, 9, 40)][None])
    mask, bound = np.zeros((1, n, n), np.uint8), np.array([BOUND])
    ctx.check(ctx.lib.mp_grid_rasterize(ctx.handle, 1, n, n, ptr(bound), 3, 40, ptr(obs), ptr(mask)))
    return mask[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one of circle_256, circle_2048, serpentine_2048")
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs must be at least 3")
    ctx = default_context(0)
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    out = {"workload": "mp_grid_field, one map a call, field and n_reached copied back, one MI355X", "runs": a.runs}
    serp = C.serpentine(2048, 1055)
    maps = {"circle_256": (circle_mask(ctx, 256), BOUND, (0.0, 0.0)), "circle_2048": (circle_mask(ctx, 2048), BOUND, (0.0, 0.0)),
            "serpentine_2048": (serp["mask"], serp["bound"], C.real(serp, serp["source"]))}
    m256, n256 = maps["circle_256"][0], None
    for name, (mask, bound, src) in maps.items():
        if a.only not in (None, name):
            continue
        call = lambda: gridfield.cost_field(mask, bound, src, ctx=ctx)  # noqa: E731
        os.environ.pop("MPGPU_FIELD_CHECK_EVERY", None)
        field, n = call()
        if name == "circle_256":
            g = Grid(bound, 256, 256)
            ref = F.field_jacobi(g, mask, g.cell(src))[0]
            assert np.array_equal(field.view(np.uint64), ref.view(np.uint64)) and n == int(np.isfinite(ref).sum())
            n256 = n
        call()
        ctx.lib.mp_ctx_kernel_timing(ctx.handle, 1)
        ks = []
        for _ in range(3):
            call()
            ctx.check(ctx.lib.mp_ctx_kernel_ms(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)))
            ks.append(ms.value)
        ctx.lib.mp_ctx_kernel_timing(ctx.handle, 0)
        out.update({f"{name}_cells": int(mask.size), f"{name}_n_reached": int(n), f"{name}_rounds": int(cnt.value),
                    f"{name}_kernel_ms": sorted(ks)[1], f"{name}_call_ms": med(call, a.runs)})
        if name != "circle_256":
            # the walk: one query at the far end of the map, the path cut at one entry (so nothing but path_n comes
            # back); its kernel time is the call's kernel time beyond the relaxation's
            far = C.real(serp, (2048, 1055)) if name == "serpentine_2048" else (119.0, 119.0)
            walk = lambda: gridfield.field_paths(mask, bound, src, None, [far], stride=1, ctx=ctx)  # noqa: E731
            walk()
            ctx.lib.mp_ctx_kernel_timing(ctx.handle, 1)
            ws = []
            for _ in range(3):
                q = walk()
                ctx.check(ctx.lib.mp_ctx_kernel_ms(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)))
                ws.append(ms.value)
            ctx.lib.mp_ctx_kernel_timing(ctx.handle, 0)
            cells = int(q["path_n"][0])
            out.update({f"{name}_walk_cells": cells, f"{name}_with_walk_kernel_ms": sorted(ws)[1],
                        f"{name}_walk_us_per_cell": (sorted(ws)[1] - sorted(ks)[1]) * 1e3 / max(cells, 1)})
        for every in (4, 16):
            os.environ["MPGPU_FIELD_CHECK_EVERY"] = str(every)
            call()
            out[f"{name}_every{every}_call_ms"] = med(call, a.runs)
        os.environ.pop("MPGPU_FIELD_CHECK_EVERY", None)
    if a.only in (None, "circle_256"):
        # the yardstick: planDKA! to exhaustion on the same map (goal off the grid), lean outputs
        bound, start, goal = np.array([BOUND]), np.zeros((1, 2)), np.full((1, 2), -10.0)
        cost, plen = np.zeros(1), np.zeros(1)
        found, pops, nn = (np.zeros(1, np.int32) for _ in range(3))
        dka = lambda: ctx.check(ctx.lib.mp_grid_plan(ctx.handle, 1, 0, 1, 256, 256, ptr(bound), ptr(start), ptr(goal), 1, 0,  # noqa: E731
                                                     ptr(m256), ptr(cost), ptr(found), ptr(pops), ptr(nn), None, None, None,
                                                     ptr(plen)))
        dka()
        out["dka_exhausted_256_n_nodes_is_n_reached"] = bool(found[0] == 0 and nn[0] == n256)
        t = med(dka, a.runs)
        out.update({"dka_exhausted_256_ms": t, "dka_exhausted_256_pops": int(pops[0]), "dka_exhausted_256_us_per_pop": t * 1e3 / int(pops[0]),
                    "circle_256_speedup_over_dka": t / out["circle_256_call_ms"]})
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
