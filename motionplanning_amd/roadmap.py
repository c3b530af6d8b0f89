"""A multi-query roadmap planner for a car: PRM under the Reeds-Shepp metric, through mp_roadmap_build and
mp_roadmap_query (csrc/roadmap.hip).  A build extension: the reference has no such planner, but every edge has its
semantics.  The distance d(a -> b) is `reeds_shepp.cost_matrix`'s value (rs_heuristic, hybrid_astar_utils.jl:361-373)
and an edge is free iff RS_connected (:224-233) holds for the pose pair, which is `reeds_shepp.connect`'s flag.

`build` ranks, for every node, the k nodes nearest from it and checks those edges on the device; only nbr[n][k]
and w[n][k] come back (12 bytes a candidate).  `query` joins each start and goal to the roadmap in the same way,
runs Dijkstra per query on the device and, when asked, returns the driven path of every edge of every found
sequence from one rs_allpath and one create_path call.
"""
from dataclasses import dataclass, field

import numpy as np

from . import reeds_shepp
from .abi import f64, ptr
from .context import default_context

__all__ = ["Roadmap", "QueryResult", "build", "query", "sample_poses", "MAX_NODES", "MAX_K"]

MAX_NODES = 4096  # MP_ROADMAP_MAX_NODES: a node's distances are ranked in 32 KB of LDS
MAX_K = 64        # MP_ROADMAP_MAX_K


@dataclass
class Roadmap:
    nodes: np.ndarray         # [n][3] poses [x, y, ψ]
    walls: np.ndarray         # [n_walls][5] blocks [x, y, ψ, l/2, w/2]
    minR: float
    vehicle_size: tuple       # (length, width)
    k: int
    nbr: np.ndarray           # [n][k] int32: row i's candidates by (d(i -> j), j), -1 past the last
    w: np.ndarray             # [n][k]: d where the edge is free, +Inf where blocked or padding


@dataclass
class QueryResult:
    found: bool
    cost: float               # the sum of the edge lengths along seq, +Inf when not found
    seq: np.ndarray           # vertices from start to goal: 0 = start, 1..n = nodes, n + 1 = goal
    settled: int              # vertices Dijkstra settled
    direct_free: bool         # the direct edge start -> goal is free
    edge_paths: list = field(default_factory=list)  # 3 x m path of each edge on seq (want_paths)
    Path: np.ndarray = None   # their hstack, 3 x sum(m); None when not found or not wanted


def _scene(nodes, walls, vehicle_size):
    nodes = f64(nodes).reshape(-1, 3)
    walls = f64(walls).reshape(-1, 5)
    return nodes, walls, (float(vehicle_size[0]), float(vehicle_size[1]))


def build(nodes, walls, minR, vehicle_size, k=16, ctx=None):
    """mp_roadmap_build: the Roadmap of nodes[n][3] among walls[n_walls][5] for a vehicle [length, width]."""
    ctx = ctx or default_context()
    nodes, walls, vs = _scene(nodes, walls, vehicle_size)
    n, k = len(nodes), int(k)
    nbr, w = np.zeros((n, k), np.int32), np.zeros((n, k))
    ctx.check(ctx.lib.mp_roadmap_build(ctx.handle, n, ptr(nodes), len(walls), ptr(walls) if len(walls) else None,
                                       float(minR), vs[0], vs[1], k, ptr(nbr), ptr(w)))
    return Roadmap(nodes, walls, float(minR), vs, k, nbr, w)


def query(rm, starts, goals, want_paths=True, ctx=None):
    """mp_roadmap_query for starts[B][3] -> goals[B][3] on rm: a list of QueryResult (one, not a list, for a single
    query given as vectors).  want_paths: the paths of all edges of all found sequences from one rs_allpath and one
    create_path call, so each is `reeds_shepp.connect`'s path for its pose pair."""
    ctx = ctx or default_context()
    single = np.ndim(starts) == 1
    starts, goals = f64(starts).reshape(-1, 3), f64(goals).reshape(-1, 3)
    B, n = len(starts), len(rm.nodes)
    assert len(goals) == B, "starts and goals hold different query counts"
    found, cost, direct = np.zeros(B, np.uint8), np.zeros(B), np.zeros(B, np.uint8)
    seq, seq_len, settled = np.zeros((B, n + 2), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    nbr, w = np.ascontiguousarray(rm.nbr, np.int32), f64(rm.w)
    ctx.check(ctx.lib.mp_roadmap_query(ctx.handle, n, ptr(rm.nodes), len(rm.walls),
                                       ptr(rm.walls) if len(rm.walls) else None, rm.minR, rm.vehicle_size[0],
                                       rm.vehicle_size[1], rm.k, ptr(nbr), ptr(w), B, ptr(starts), ptr(goals),
                                       ptr(found), ptr(cost), ptr(seq), ptr(seq_len), ptr(settled), ptr(direct)))
    out = [QueryResult(bool(found[q]), float(cost[q]), seq[q, : seq_len[q]].copy(), int(settled[q]), bool(direct[q]))
           for q in range(B)]
    if want_paths and found.any():
        a, b = [], []
        for q, r in enumerate(out):
            pose = np.vstack([starts[q], rm.nodes, goals[q]])
            a.append(pose[r.seq[:-1]])
            b.append(pose[r.seq[1:]])
        a, b = np.vstack(a), np.vstack(b)
        win = reeds_shepp.rs_allpath(a, b, rm.minR, want_norm=False, ctx=ctx)
        path, plen = reeds_shepp.create_path(win["cmds"][np.arange(len(a)), win["best"]], a, rm.minR, ctx=ctx)
        e = 0
        for r in out:
            if r.found:
                m = len(r.seq) - 1
                r.edge_paths = [np.ascontiguousarray(path[i, : plen[i]].T) for i in range(e, e + m)]
                r.Path = np.hstack(r.edge_paths)
                e += m
    return out[0] if single else out


def sample_poses(bound, n, seed):
    """n poses for a roadmap: x and y uniform in bound = [[x0, x1], [y0, y1]], ψ uniform in ±π."""
    r = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = bound
    return np.c_[x0 + (x1 - x0) * r.random(n), y0 + (y1 - y0) * r.random(n), np.pi * (2 * r.random(n) - 1)]
