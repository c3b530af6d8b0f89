"""Time mp_path_collision (kernel time by HIP events, mp_ctx_kernel_ms) at two shapes:

  sweep   64 scenes x 4,096 poses x 64 walls, stride 1
  hastar  256 scenes x 501 poses x 3 walls, stride 5 (Hybrid A*'s own block_collision_check shape)

on two fields each: `apart` (walls below y = 0, poses above y = 6: every pair is free, so every (pose, wall)
ConvexCollision runs) and `mixed` (walls scattered among the poses: a pose stops at its first hit).  The CPU
figure is the oracle's or_ha_block_free -- its or_ha_convex_free loop in C, one thread -- on the `apart` field,
where it runs every pair too; the oracle's stride is fixed at 5, so the stride-1 shape is handed to it with
each pose at every fifth row.  Results are compared before anything is timed."""
import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import oracle  # noqa: E402
from motionplanning_amd import collision as C  # noqa: E402
from motionplanning_amd.abi import HAParams  # noqa: E402
from motionplanning_amd.context import default_context  # noqa: E402

VEH = (3.0, 2.0)
REPS = 20


def field(kind, B, n, nw, seed):
    r = np.random.default_rng(seed)
    poses = np.c_[r.uniform(-40, 40, B * n), r.uniform(6, 60, B * n), r.uniform(-7, 7, B * n)].reshape(B, n, 3)
    wy = r.uniform(-60, -6, B * nw) if kind == "apart" else r.uniform(6, 60, B * nw)
    walls = np.c_[r.uniform(-40, 40, B * nw), wy, r.uniform(-3, 3, B * nw), r.uniform(0.5, 3, (B * nw, 2))]
    return poses, walls.reshape(B, nw, 5)


def gpu_ms(ctx, p, poses, walls):
    C.path_collision(p, poses, walls, ctx=ctx)  # warm-up: code object, workspaces
    ctx.lib.mp_ctx_kernel_timing(ctx.handle, 1)
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    ctx.check(ctx.lib.mp_ctx_kernel_ms(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)))
    times = []
    for _ in range(REPS):
        out = C.path_collision(p, poses, walls, ctx=ctx)
        ctx.check(ctx.lib.mp_ctx_kernel_ms(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)))
        times.append(ms.value)
    ctx.lib.mp_ctx_kernel_timing(ctx.handle, 0)
    return out, float(np.median(times)), float(min(times)), float(max(times))


def cpu_block_free(poses, walls, stride):
    """or_ha_block_free per scene (stride 5 inside): (booleans, seconds)."""
    B, n, _ = poses.shape
    hp = HAParams()
    hp.vehicle_len, hp.vehicle_wid = VEH
    hp.n_walls = walls.shape[1]
    if stride == 1:  # pose k at row 5k, the rows between are never read
        rows = np.zeros((B, 5 * (n - 1) + 1, 3))
        rows[:, ::5] = poses
    else:
        assert stride == 5
        rows = poses
    rows = np.ascontiguousarray(rows)
    t0 = time.perf_counter()
    free = [oracle.ha_block_free(hp, rows[b], walls[b]) for b in range(B)]
    return np.array(free), time.perf_counter() - t0


def main():
    ctx = default_context(0)
    for name, B, n, nw, stride in (("sweep", 64, 4096, 64, 1), ("hastar", 256, 501, 3, 5)):
        p = C.collide_params(VEH, stride=stride)
        checked = len(range(0, n, stride))
        for kind in ("apart", "mixed"):
            poses, walls = field(kind, B, n, nw, seed=3)
            out, med, lo, hi = gpu_ms(ctx, p, poses, walls)
            rec = dict(shape=name, field=kind, scenes=B, poses=n, walls=nw, stride=stride,
                       pairs=B * checked * nw, gpu_kernel_ms_median=round(med, 4), gpu_kernel_ms_min=round(lo, 4),
                       gpu_kernel_ms_max=round(hi, 4), reps=REPS, scenes_free=int(out["scene_free"].sum()),
                       poses_hit=int(out["n_hit"].sum()))
            if kind == "apart":
                free, sec = cpu_block_free(poses, walls, stride)
                assert np.array_equal(free, out["scene_free"].astype(bool)) and free.all()
                rec.update(cpu_oracle_ms=round(sec * 1e3, 2), cpu_ns_per_pair=round(sec * 1e9 / rec["pairs"], 2),
                           gpu_ps_per_pair=round(med * 1e9 / rec["pairs"], 2))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
