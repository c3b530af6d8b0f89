"""Batched Reeds-Shepp curves on the device (PathPlanning/ReedsSheppsCurves/main.jl and
src/ReedsSheppsUtils.jl; rs_heuristic and RS_connected of HybridAstar/src/hybrid_astar_utils.jl) through
mp_rs_allpath, mp_rs_create_path and mp_rs_cost_matrix.

`rs_allpath`, `create_path` and `cost_matrix` are the batched calls in the C layout.  The functions with the
reference's names take and return the reference's shapes (a command table is 5 x 3 with columns
[length, gear, steer], all of them 5 x 3 x 48, a path 3 x n; candidate indices are 0-based).
`candidate_paths` is the data behind the driver's plotpaths / plotActpaths, `connect` is RS_connected without a
searcher.  Every value is the reference's in fp64; changeBasis runs on the device with the library's sin/cos
(hybrid_astar.changeBasis is host arithmetic).
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import collision
from .abi import HAParams, f64, ptr
from .context import default_context

__all__ = ["rs_allpath", "create_path", "cost_matrix", "changeBasis", "allpath", "createPath", "createActPath",
           "candidate_paths", "CandidatePaths", "connect", "N_CANDIDATES", "MAX_PATH", "PATH_TILE"]

N_CANDIDATES = 48
MAX_PATH = 501   # 100 steps x 5 segments + the start
PATH_TILE = 16   # command tables per workgroup of mp_rs_create_path (RS_PT, csrc/rs_device.hpp)


# ------------------------------------------------------------------ batched calls, C layout
def rs_allpath(init, term, minR, want_norm=True, want_cmds=True, ctx=None):
    """mp_rs_allpath for init[B][3], term[B][3], minR[B] (a scalar: the same for all): dict(norm[B][3] or None,
    cost[B][48], cmds[B][48][5][3] or None, best[B], act_cost[B])."""
    ctx = ctx or default_context()
    init, term = f64(init).reshape(-1, 3), f64(term).reshape(-1, 3)
    B = len(init)
    assert len(term) == B, "init and term hold different pair counts"
    minR = np.ascontiguousarray(np.broadcast_to(f64(minR).reshape(-1), (B,)))
    out = dict(norm=np.zeros((B, 3)) if want_norm else None, cost=np.zeros((B, N_CANDIDATES)),
               cmds=np.zeros((B, N_CANDIDATES, 5, 3)) if want_cmds else None, best=np.zeros(B, np.int32),
               act_cost=np.zeros(B))
    ctx.check(ctx.lib.mp_rs_allpath(ctx.handle, B, ptr(init), ptr(term), ptr(minR), ptr(out["norm"]), ptr(out["cost"]),
                                    ptr(out["cmds"]), ptr(out["best"]), ptr(out["act_cost"])))
    return out


def create_path(cmds, init=None, minR=None, ctx=None):
    """mp_rs_create_path for cmds[n][5][3]: (path[n][501][3], path_len[n]).  init[n][3] and minR[n] (or a scalar)
    both given: createActPath; both None: createPath."""
    ctx = ctx or default_context()
    cmds = f64(cmds).reshape(-1, 5, 3)
    n = len(cmds)
    if init is not None:
        init = f64(init).reshape(-1, 3)
        assert len(init) == n, "init and cmds hold different counts"
    if minR is not None:
        minR = np.ascontiguousarray(np.broadcast_to(f64(minR).reshape(-1), (n,)))
    path = np.zeros((n, MAX_PATH, 3))
    path_len = np.zeros(n, np.int32)
    ctx.check(ctx.lib.mp_rs_create_path(ctx.handle, n, ptr(init), ptr(minR), ptr(cmds), ptr(path), ptr(path_len)))
    return path, path_len


def cost_matrix(a, b, minR, want_best=True, ctx=None):
    """mp_rs_cost_matrix: the Reeds-Shepp distance opt_cost*minR from every a[na][3] to every b[nb][3] ->
    (dist[na][nb], best[na][nb] uint8 or None)."""
    ctx = ctx or default_context()
    a, b = f64(a).reshape(-1, 3), f64(b).reshape(-1, 3)
    dist = np.zeros((len(a), len(b)))
    best = np.zeros((len(a), len(b)), np.uint8) if want_best else None
    ctx.check(ctx.lib.mp_rs_cost_matrix(ctx.handle, len(a), ptr(a), len(b), ptr(b), float(minR), ptr(dist), ptr(best)))
    return dist, best


# ------------------------------------------------------------------ the reference's names and shapes
def changeBasis(init, term, minR, ctx=None):
    """ReedsSheppsUtils.jl:2-11 on the device: the goal in the start's frame, lengths in turning radii."""
    return rs_allpath(init, term, minR, want_cmds=False, ctx=ctx)["norm"][0]


def allpath(norm_states, ctx=None):
    """ReedsSheppsUtils.jl:468-511 for one normalised state: (opt_cmd 5 x 3, opt_cost, cmds 5 x 3 x 48, costs[48])
    (mp_ha_allpath, which takes the state as it is)."""
    ctx = ctx or default_context()
    ns = f64(norm_states).reshape(1, 3)
    cost, tab, best = np.zeros((1, N_CANDIDATES)), np.zeros((1, N_CANDIDATES, 5, 3)), np.zeros(1, np.int32)
    ctx.check(ctx.lib.mp_ha_allpath(ctx.handle, 1, ptr(ns), ptr(cost), ptr(tab), ptr(best)))
    cmds = np.ascontiguousarray(tab[0].transpose(1, 2, 0))
    b = int(best[0])
    return cmds[:, :, b].copy(), float(cost[0, b]), cmds, cost[0].copy()


def _table(cmds):
    cmds = f64(cmds)
    assert cmds.ndim == 2 and cmds.shape[1] == 3 and cmds.shape[0] <= 5, "a command table is m x 3, m <= 5"
    t = np.zeros((1, 5, 3))
    t[0, : cmds.shape[0]] = cmds
    return t


def createPath(cmds, ctx=None):
    """ReedsSheppsUtils.jl:411-437: the 3 x (100 nseg + 1) path of one command table from [0, 0, 0]."""
    path, n = create_path(_table(cmds), ctx=ctx)
    return np.ascontiguousarray(path[0, : n[0]].T)


def createActPath(init, minR, cmds, ctx=None):
    """ReedsSheppsUtils.jl:440-466: the same from init, lengths scaled by minR."""
    path, n = create_path(_table(cmds), f64(init).reshape(1, 3), float(minR), ctx=ctx)
    return np.ascontiguousarray(path[0, : n[0]].T)


@dataclass
class CandidatePaths:
    """What plotpaths / plotActpaths (ReedsSheppsUtils.jl:515-550) draw for one pose pair."""
    norm: np.ndarray      # changeBasis(init, term, minR)
    costs: np.ndarray     # [48]
    cmds: np.ndarray      # 5 x 3 x 48
    feasible: np.ndarray  # findall(costs .< Inf), 0-based (NaN is not feasible)
    paths: list           # createPath of each feasible candidate, 3 x n
    act_paths: list       # createActPath(init, minR, .) of each
    best: int             # argmin(costs), 0-based
    opt_cost: float
    act_opt_cost: float   # opt_cost*minR
    best_path: np.ndarray      # createPath of the winner
    best_act_path: np.ndarray  # createActPath of the winner


def candidate_paths(init, term, minR, ctx=None):
    """main.jl:15-23 for B pose pairs: one rs_allpath call, then one create_path call over the feasible candidates'
    and the winners' tables of all pairs (createPath and createActPath rows together).  Returns a CandidatePaths per
    pair (one, not a list, for a single pair given as vectors)."""
    single = np.ndim(init) == 1
    init, term = f64(init).reshape(-1, 3), f64(term).reshape(-1, 3)
    B = len(init)
    mr = np.ascontiguousarray(np.broadcast_to(f64(minR).reshape(-1), (B,)))
    r = rs_allpath(init, term, mr, ctx=ctx)
    feas = r["cost"] < np.inf
    pb, pc = np.nonzero(feas)
    # rows: every feasible (pair, candidate), then every pair's winner
    rows_b = np.concatenate([pb, np.arange(B)])
    rows_c = np.concatenate([pc, r["best"].astype(np.int64)])
    tables = r["cmds"][rows_b, rows_c]
    m = len(rows_b)
    # one call: createPath is createActPath from the origin at minR = 1 (a product with 1.0 is exact)
    path, plen = create_path(np.concatenate([tables, tables]), np.concatenate([np.zeros((m, 3)), init[rows_b]]),
                             np.concatenate([np.ones(m), mr[rows_b]]), ctx=ctx)
    cut = [np.ascontiguousarray(path[i, : plen[i]].T) for i in range(2 * m)]
    first = np.concatenate([[0], np.cumsum(feas.sum(1))])
    out = []
    for b in range(B):
        lo, hi = int(first[b]), int(first[b + 1])
        w = len(pb) + b
        bi = int(r["best"][b])
        out.append(CandidatePaths(r["norm"][b].copy(), r["cost"][b].copy(),
                                  np.ascontiguousarray(r["cmds"][b].transpose(1, 2, 0)), pc[lo:hi].copy(), cut[lo:hi],
                                  cut[m + lo:m + hi], bi, float(r["cost"][b, bi]), float(r["act_cost"][b]), cut[w],
                                  cut[m + w]))
    return out[0] if single else out


HA_MAX_WALLS = 16  # walls per scene mp_ha_rs_connect takes (MAXW, csrc/hastar.hip)


def _connect_ha(ctx, init, term, minR, walls, vehicle_size):
    """RS_connected through mp_ha_rs_connect: one launch, one workgroup per pair, one copy back."""
    B, n_walls = len(init), walls.shape[1]
    p = HAParams()
    p.vehicle_len, p.vehicle_wid = float(vehicle_size[0]), float(vehicle_size[1])
    p.minR, p.expand_time = minR, 1.0
    for i in range(3):
        p.res[i] = 1.0
    p.n_walls, p.n_prim, p.n_col, p.max_pops = n_walls, 1, 1, 1
    ok, path, plen = np.zeros(B, np.uint8), np.zeros((B, MAX_PATH, 3)), np.zeros(B, np.int32)
    ctx.check(ctx.lib.mp_ha_rs_connect(ctx.handle, ctypes.byref(p), B, ptr(init), ptr(term),
                                       ptr(walls) if n_walls else None, ptr(ok), ptr(path), ptr(plen)))
    return ok.astype(bool), path, plen


def connect(init, term, minR, walls, vehicle_size, route="auto", ctx=None):
    """RS_connected (hybrid_astar_utils.jl:224-233) without a searcher: the optimal Reeds-Shepp path from init to
    term and block_collision_check of it at sparcity_num = 5.  One pair (init, term vectors, walls [n_walls][5] of
    [x, y, ψ, l/2, w/2]) -> (free, path 3 x n); B pairs (init[B][3], walls[B][n_walls][5]) -> (free[B], list of
    paths, each a 3 x n view of one result buffer).
    route "compose": rs_allpath -> create_path of the winners -> collision.path_collision, for any minR[B] and any
    number of walls.  Its kernels take a quarter of mp_ha_rs_connect's time, but as three synchronous host-pointer
    calls it copies every pair's 48 command tables back and the paths up again, and a whole call takes longer at
    every batch size measured.  route "ha": mp_ha_rs_connect, which needs one finite minR > 0
    and at most 16 walls.  route "auto" (default): "ha" where it applies, else "compose".  Same values either way."""
    ctx = ctx or default_context()
    single = np.ndim(init) == 1
    init, term = f64(init).reshape(-1, 3), f64(term).reshape(-1, 3)
    B = len(init)
    mr = np.ascontiguousarray(np.broadcast_to(f64(minR).reshape(-1), (B,)))
    walls = f64(walls).reshape(B, -1, 5)
    ha_ok = bool((mr == mr[0]).all() and np.isfinite(mr[0]) and mr[0] > 0 and walls.shape[1] <= HA_MAX_WALLS)
    if route not in ("auto", "compose", "ha") or (route == "ha" and not ha_ok):
        raise ValueError("connect: route %r does not apply (ha needs one finite minR > 0 and <= 16 walls)" % (route,))
    if route == "ha" or (route == "auto" and ha_ok):
        free, path, plen = _connect_ha(ctx, init, term, float(mr[0]), walls, vehicle_size)
    else:
        r = rs_allpath(init, term, mr, want_norm=False, ctx=ctx)
        path, plen = create_path(r["cmds"][np.arange(B), r["best"]], init, mr, ctx=ctx)
        hit = collision.path_collision(collision.collide_params(vehicle_size, stride=5), path, walls,
                                       pose_count=plen, want_pose_free=False, ctx=ctx)
        free = hit["scene_free"].astype(bool)
    paths = [path[b, : plen[b]].T for b in range(B)]
    return (bool(free[0]), paths[0]) if single else (free, paths)
