"""Time the Reeds-Shepp roadmap build against the route that existed before it (whole calls by the host clock; every
call here is synchronous and ends in a stream synchronise, and the copies are what the two sides differ in).

  fused     roadmap.build: mp_roadmap_build, one call; nbr[n][k] and w[n][k] come back (12 bytes a candidate).
  composed  reeds_shepp.cost_matrix(nodes, nodes) -> top-k on the host (a stable argsort on d, so ties go to the
            lower index) -> reeds_shepp.connect of the n*k pairs in calls of CONNECT_CHUNK, route="auto": with the
            scene's 3 walls that is mp_ha_rs_connect, with 33 walls the three composed calls (route "compose").

Scene: the Hybrid A* driver's perpendicular scene and settings; nodes from roadmap.sample_poses in the driver's bounds.
The 33-wall scene adds 30 small walls where they block nothing.  Shapes (n, k) = (1024, 16) and (4096, 32).  Every
shape is run once on both sides first (warm-up), the two roadmaps are compared bit for bit, and only then the sides are
timed, alternating, REPS times each in this one process.  Per side: median, minimum and maximum; `spread` is
(max - min) / median of identical repeated calls, the yardstick for fused/composed.  Then 256 queries on the fused
roadmap (no counterpart: nothing answered them before).  One JSON line per measurement, then the table."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from motionplanning_amd import hybrid_astar as ha  # noqa: E402
from motionplanning_amd import reeds_shepp as rs  # noqa: E402
from motionplanning_amd import roadmap  # noqa: E402
from motionplanning_amd.context import default_context  # noqa: E402

REPS = 5
CONNECT_CHUNK = 16384  # pairs per connect call (its path output: 197 MB)
BOUND = [[-4.5, 9.5], [0.5, 9.5]]
SHAPES = [(1024, 16), (4096, 32)]
N_QUERIES = 256


def scenes():
    walls = np.array(ha.PERPENDICULAR["walls"], np.float64)
    far = np.array([[40.0 + 3 * (q % 6), 40.0 + 3 * (q // 6), 0.3 * q, 0.5, 0.25] for q in range(30)])
    return [("3 walls", walls), ("33 walls", np.ascontiguousarray(np.r_[walls, far]))]


def composed_build(ctx, nodes, walls, minR, vehicle, k):
    n = len(nodes)
    dist, _ = rs.cost_matrix(nodes, nodes, minR, want_best=False, ctx=ctx)
    d = np.where(np.isfinite(dist), dist, np.inf)
    d[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    dk = np.take_along_axis(d, order, axis=1)
    nbr = np.where(np.isfinite(dk), order, -1).astype(np.int32)
    w = np.full((n, k), np.inf)
    rows, cols = np.nonzero(nbr >= 0)
    init, term = nodes[rows], nodes[nbr[rows, cols]]
    free = np.zeros(len(rows), bool)
    for lo in range(0, len(rows), CONNECT_CHUNK):
        hi = min(lo + CONNECT_CHUNK, len(rows))
        wl = np.ascontiguousarray(np.broadcast_to(walls, (hi - lo,) + walls.shape))
        free[lo:hi], _ = rs.connect(init[lo:hi], term[lo:hi], minR, wl, vehicle, route="auto", ctx=ctx)
    w[rows[free], cols[free]] = dk[rows[free], cols[free]]
    return nbr, w


def clock(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def side(t):
    t = np.array(t)
    return dict(median_ms=round(float(np.median(t)), 3), min_ms=round(float(t.min()), 3),
                max_ms=round(float(t.max()), 3), spread=round(float((t.max() - t.min()) / np.median(t)), 4))


def main():
    ctx = default_context(0)
    st = ha.driver_settings()
    minR, vehicle = st["minR"], st["vehicle_size"]
    recs = []
    for name, walls in scenes():
        for n, k in SHAPES:
            nodes = roadmap.sample_poses(BOUND, n, 2026 + n)
            rm = roadmap.build(nodes, walls, minR, vehicle, k=k, ctx=ctx)
            nbr, w = composed_build(ctx, nodes, walls, minR, vehicle, k)
            assert np.array_equal(rm.nbr, nbr), (name, n, k)
            assert np.array_equal(rm.w.view(np.uint64), w.view(np.uint64)), (name, n, k)
            tf, tc = [], []
            for _ in range(REPS):
                tf.append(clock(lambda: roadmap.build(nodes, walls, minR, vehicle, k=k, ctx=ctx)))
                tc.append(clock(lambda: composed_build(ctx, nodes, walls, minR, vehicle, k)))
            rec = dict(what="build", scene=name, n=n, k=k, edges=int((nbr >= 0).sum()),
                       free=int(np.isfinite(w).sum()), reps=REPS, fused=side(tf), composed=side(tc),
                       fused_over_composed=round(float(np.median(tf) / np.median(tc)), 5))
            print(json.dumps(rec), flush=True)
            recs.append(rec)
            starts = roadmap.sample_poses(BOUND, N_QUERIES, 7)
            goals = np.tile(ha.PERPENDICULAR["ending_real"], (N_QUERIES, 1))
            res = roadmap.query(rm, starts, goals, want_paths=False, ctx=ctx)
            tq = [clock(lambda: roadmap.query(rm, starts, goals, want_paths=False, ctx=ctx)) for _ in range(REPS)]
            rec = dict(what="query", scene=name, n=n, k=k, queries=N_QUERIES, found=sum(r.found for r in res),
                       settled_mean=round(float(np.mean([r.settled for r in res])), 1), reps=REPS, fused=side(tq))
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    print("\nbuild     scene      n     k   edges    fused ms (min..max)         composed ms (min..max)         "
          "fused/composed  spread fused / composed")
    for q in recs:
        if q["what"] == "build":
            f, c = q["fused"], q["composed"]
            print("build     %-8s %5d %4d %7d %9.3f (%.3f..%.3f)  %10.3f (%.3f..%.3f)  %9.5f       %.4f / %.4f" % (
                q["scene"], q["n"], q["k"], q["edges"], f["median_ms"], f["min_ms"], f["max_ms"], c["median_ms"],
                c["min_ms"], c["max_ms"], q["fused_over_composed"], f["spread"], c["spread"]))
    print("\nquery     scene      n     k  queries  found  settled (mean)  ms (min..max)               spread")
    for q in recs:
        if q["what"] == "query":
            f = q["fused"]
            print("query     %-8s %5d %4d %8d %6d %15.1f %9.3f (%.3f..%.3f)  %.4f" % (
                q["scene"], q["n"], q["k"], q["queries"], q["found"], q["settled_mean"], f["median_ms"], f["min_ms"],
                f["max_ms"], f["spread"]))


if __name__ == "__main__":
    main()
