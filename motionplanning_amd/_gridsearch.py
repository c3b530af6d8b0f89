"""What dijkstra.py and bfs.py share: defineDKA / defineBFS are one function over two searcher types
(Dijkstra/src/setup.jl:3-25 and BreadthFirst/src/setup.jl:3-25 differ in the node they create), and
mp_dka_plan / mp_bfs_plan take the same arguments but for final_cost."""
import math
import time

import numpy as np

from .abi import f64, ptr
from .context import default_context


def define(searcher, realsize, mapbound, starting_real, ending_real):
    """setup.jl:11-19 (realsize = [xmin, xmax, ymin, ymax]); the drawing flags have no counterpart."""
    s = searcher.s
    s.actualbound = np.asarray(realsize, np.float64)
    s.mapbound = np.asarray(mapbound, np.float64)
    s.starting_real = np.asarray(starting_real, np.float64)
    s.ending_real = np.asarray(ending_real, np.float64)
    s.x_factor = (s.actualbound[1] - s.actualbound[0]) / (s.mapbound[0] - 1)
    s.y_factor = (s.actualbound[3] - s.actualbound[2]) / (s.mapbound[1] - 1)
    s.starting_pos = np.array([math.floor((s.starting_real[0] - s.actualbound[0]) / s.x_factor + 1),
                               math.floor((s.starting_real[1] - s.actualbound[2]) / s.y_factor + 1)], np.int64)
    s.ending_pos = np.array([math.floor((s.ending_real[0] - s.actualbound[0]) / s.x_factor + 1),
                             math.floor((s.ending_real[1] - s.actualbound[2]) / s.y_factor + 1)], np.int64)
    return searcher


def transfer(searcher, pos):
    """TransferCoordinate (dka_utils.jl:217-220, bfs_utils.jl:163-166)."""
    s = searcher.s
    return np.array([(pos[0] - 1.0) * s.x_factor + s.actualbound[0], (pos[1] - 1.0) * s.y_factor + s.actualbound[2]])


def plan_batch(searchers, entry, path_field, with_cost, ctx=None):
    """B searchers sharing mapbound through mp_dka_plan / mp_bfs_plan (entry).  Obstacle counts may differ: the
    shorter lists are padded with [0, 0, 0] circles, which the strict < against r^2 = 0 never hits, so a padded
    scene is the unpadded one bit for bit."""
    ctx = ctx or default_context()
    a0 = searchers[0]
    nx, ny = int(a0.s.mapbound[0]), int(a0.s.mapbound[1])
    for a in searchers:
        if (int(a.s.mapbound[0]), int(a.s.mapbound[1])) != (nx, ny):
            raise ValueError("plan_batch: every search needs the same mapbound")
        if any(len(o) != 3 for o in a.s.obstacle_list):
            raise ValueError("plan_batch: obstacles are circles [x, y, r]")
    B, M = len(searchers), nx * ny + 1
    n_obs = max(len(a.s.obstacle_list) for a in searchers)
    bound = f64([a.s.actualbound for a in searchers])
    start = f64([a.s.starting_real for a in searchers])
    goal = f64([a.s.ending_real for a in searchers])
    obs = None
    if n_obs:
        obs = np.zeros((B, n_obs, 3))
        for b, a in enumerate(searchers):
            if a.s.obstacle_list:
                obs[b, : len(a.s.obstacle_list)] = a.s.obstacle_list
    cost, plen = np.zeros(B), np.zeros(B)
    found, pops, nn, pn = (np.zeros(B, np.int32) for _ in range(4))
    seq = np.zeros((B, 2 * M), np.int32)
    path = np.zeros((B, M), np.int32)
    outs = ([ptr(cost)] if with_cost else []) + [ptr(found), ptr(pops), ptr(nn), ptr(seq), ptr(path), ptr(pn), ptr(plen)]
    t0 = time.time()
    ctx.check(getattr(ctx.lib, entry)(ctx.handle, B, nx, ny, ptr(bound), ptr(start), ptr(goal), n_obs, ptr(obs), *outs))
    dt = time.time() - t0
    for b, a in enumerate(searchers):
        r = a.r
        if with_cost:
            r.final_cost = float(cost[b])
        r.path_length = float(plen[b])
        r.found, r.loop_count, r.n_nodes = bool(found[b]), int(pops[b]), int(nn[b])
        r.pop_sequence = seq[b, : pops[b]].copy()
        enc = path[b, : pn[b]].astype(np.int64)
        # Encode index -> [x y] rows; index 0 is a start cell off the grid
        cells = np.c_[(enc - 1) % nx + 1, (enc - 1) // nx + 1]
        cells[enc == 0] = a.s.starting_pos
        setattr(r, path_field, cells)
        r.actualpath = np.array([transfer(a, c) for c in cells]).reshape(-1, 2)
        r.planning_time = dt
    return searchers
