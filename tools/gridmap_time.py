"""Time the occupancy-map tools (mp_grid_distance, mp_grid_inflate) on seeded maps of blocked discs at two settings:
1 map of 2048 x 2048 inflated by r2 = 4, and 64 maps of 512 x 512 inflated by r2 = 100.

For each setting and call: the kernel time (row pass + column pass, mp_ctx_kernel_timing) and the whole call with its
copies, each the median of --runs timed calls after warm-up; the bytes a perfect pass would move (N read, 4N written
for the distance, N for the inflation) over the kernel time as a fraction of HBM bandwidth; and a CPU baseline on the
same machine: scipy.ndimage.distance_transform_edt on the same maps where scipy imports, else the numpy restatement of
tests/gridmap_ref.py on one 512 x 512 map, labelled as such.  The outputs are checked against the restatement on one
512 x 512 map before anything is timed.

Prints one JSON line; --out FILE also writes it there (profiles/)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gridmap_ref as R  # noqa: E402
from motionplanning_amd import gridmap  # noqa: E402
from motionplanning_amd.context import default_context  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak (spec)
SETTINGS = [("1x2048", 1, 2048, 4), ("64x512", 64, 512, 100)]


def disc_maps(B, n, seed):
    """B maps of n x n: n/10 blocked discs each, radius n/512 .. n/50 cells, at seeded places (2 % of the cells blocked at
    n = 512, 9 % at n = 2048; the fraction is printed)."""
    r = np.random.default_rng(seed)
    m = np.ones((B, n, n), np.uint8)
    for b in range(B):
        for _ in range(n // 10):
            cx, cy, rad = r.integers(0, n), r.integers(0, n), r.uniform(n / 512, n / 50)
            x0, x1, y0, y1 = max(0, int(cx - rad)), min(n, int(cx + rad) + 1), max(0, int(cy - rad)), min(n, int(cy + rad) + 1)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            m[b, y0:y1, x0:x1][(xx - cx) ** 2 + (yy - cy) ** 2 <= rad * rad] = 0
    return m


def med(f, runs):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--setting", default=None, choices=[s[0] for s in SETTINGS], help="only this setting (for a profiler run)")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    ctx = default_context(0)
    out = {"workload": "seeded maps of blocked discs, one MI355X; kernel = row pass + column pass", "runs": a.runs}
    probe = disc_maps(1, 512, 7)
    ref = R.d2_separable(probe[0])
    assert np.array_equal(gridmap.distance2(probe, ctx=ctx)[0], ref)
    assert np.array_equal(gridmap.inflate(probe, r2=100, ctx=ctx)[0], R.inflate(probe[0], 100, d2=ref))
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    ms, cnt = ctypes.c_double(), ctypes.c_int32()

    def kernel_ms(f):
        """median kernel time of a.runs calls (one timed region a call)"""
        ks = []
        for _ in range(a.runs):
            f()
            ctx.check(ctx.lib.mp_ctx_kernel_ms(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)))
            assert cnt.value == 1
            ks.append(ms.value)
        return sorted(ks)[len(ks) // 2]

    for name, B, n, r2 in SETTINGS:
        if a.setting not in (None, name):
            continue
        maps = disc_maps(B, n, 2048 + B)
        cells = B * n * n
        calls = {"distance": (lambda: gridmap.distance2(maps, ctx=ctx), 5 * cells),
                 "inflate": (lambda: gridmap.inflate(maps, r2=r2, ctx=ctx), 2 * cells)}
        out[f"{name}_blocked_fraction"] = float((maps == 0).mean())
        out[f"{name}_r2"] = r2
        for what, (f, ideal_bytes) in calls.items():
            for _ in range(3):  # warm-up: workspaces, code objects, clocks
                f()
            ctx.lib.mp_ctx_kernel_timing(ctx.handle, 0)
            call = med(f, a.runs)
            ctx.lib.mp_ctx_kernel_timing(ctx.handle, 1)
            k = kernel_ms(f)
            ctx.lib.mp_ctx_kernel_timing(ctx.handle, 0)
            out.update({f"{name}_{what}_kernel_ms": k, f"{name}_{what}_call_ms": call, f"{name}_{what}_ideal_bytes": ideal_bytes,
                        f"{name}_{what}_hbm_fraction": ideal_bytes / (k * 1e-3) / HBM_BYTES_PER_S})
        if ndimage is not None:
            t = med(lambda: [ndimage.distance_transform_edt(m != 0) for m in maps], 3)
            out[f"{name}_cpu_scipy_edt_ms"] = t
        else:
            t = med(lambda: R.d2_separable(maps[0][:512, :512]), 3)
            out[f"{name}_cpu_numpy_restatement_one_512x512_map_ms"] = t
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
