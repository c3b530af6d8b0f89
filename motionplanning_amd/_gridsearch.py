"""What dijkstra.py and bfs.py share: defineDKA / defineBFS are one function over two searcher types
(Dijkstra/src/setup.jl:3-25 and BreadthFirst/src/setup.jl:3-25 differ in the node they create), and
mp_dka_plan / mp_bfs_plan take the same arguments but for final_cost; and what all three grid planners share:
the call itself (run), which goes to mp_grid_plan above 51 x 51 cells and for searchers that carry a mask."""
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


LDS_MAX_CELLS = 51 * 51  # above it, and for masks, mp_grid_plan (mpgpu.h)
PLANNER = {"astar": 0, "dka": 1, "bfs": 2}  # MP_GRID_ASTAR, MP_GRID_DKA, MP_GRID_BFS
OBS_MASK = 1  # MP_GRID_OBS_MASK


def define_mask(searcher, mask):
    """A free-cell mask in place of the obstacle list: uint8 [ny, nx], cell (ix, iy) at mask[iy-1, ix-1], nonzero
    = free (an extension: the reference's planners with checkObsSafety replaced by the lookup)."""
    s = searcher.s
    m = np.asarray(mask)
    if m.dtype != np.uint8 or m.shape != (int(s.mapbound[1]), int(s.mapbound[0])):
        raise ValueError("the mask must be a uint8 array of shape [ny, nx] = [mapbound[1], mapbound[0]]")
    s.free_mask = np.ascontiguousarray(m)
    s.obstacle_list = []


def batch_masks(searchers):
    """None for a batch of listed searchers, [B, ny, nx] for a batch of masked ones; a mix is an error."""
    masks = [getattr(a.s, "free_mask", None) for a in searchers]
    if all(m is None for m in masks):
        return None
    if any(m is None for m in masks):
        raise ValueError("plan_batch: searchers with a mask and searchers with an obstacle list cannot share a batch")
    return np.ascontiguousarray(np.stack(masks), np.uint8)


def run(ctx, planner, searchers, nx, ny, kind, n_obs, obs, masks, path_field):
    """One library call for B searchers and their result fields.  A batch within LDS_MAX_CELLS and without masks
    makes the planner's own call (mp_astar_plan / mp_dka_plan / mp_bfs_plan), any other mp_grid_plan."""
    B, M = len(searchers), nx * ny + 1
    bound = f64([a.s.actualbound for a in searchers])
    start = f64([a.s.starting_real for a in searchers])
    goal = f64([a.s.ending_real for a in searchers])
    cost, plen = np.zeros(B), np.zeros(B)
    found, pops, nn, pn = (np.zeros(B, np.int32) for _ in range(4))
    seq = np.zeros((B, 2 * M), np.int32)
    path = np.zeros((B, M), np.int32)
    with_cost = planner != "bfs"
    head = (ctx.handle, B, nx, ny, ptr(bound), ptr(start), ptr(goal))
    outs = ([ptr(cost)] if with_cost else []) + [ptr(found), ptr(pops), ptr(nn), ptr(seq), ptr(path), ptr(pn), ptr(plen)]
    t0 = time.time()
    if masks is not None or nx * ny > LDS_MAX_CELLS:
        obs_args = (OBS_MASK, 0, ptr(masks)) if masks is not None else (kind, n_obs, ptr(obs))
        ctx.check(ctx.lib.mp_grid_plan(ctx.handle, PLANNER[planner], 0, *head[1:], *obs_args, ptr(cost), *outs[-7:]))
    elif planner == "astar":
        ctx.check(ctx.lib.mp_astar_plan(*head, kind, n_obs, ptr(obs), *outs))
    else:
        ctx.check(getattr(ctx.lib, f"mp_{planner}_plan")(*head, n_obs, ptr(obs), *outs))
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


def plan_batch(searchers, planner, path_field, ctx=None):
    """B searchers sharing mapbound through mp_dka_plan / mp_bfs_plan, or through mp_grid_plan above 51 x 51 cells
    and for masked searchers.  Obstacle counts may differ: the shorter lists are padded with [0, 0, 0] circles,
    which the strict < against r^2 = 0 never hits, so a padded scene is the unpadded one bit for bit."""
    ctx = ctx or default_context()
    a0 = searchers[0]
    nx, ny = int(a0.s.mapbound[0]), int(a0.s.mapbound[1])
    for a in searchers:
        if (int(a.s.mapbound[0]), int(a.s.mapbound[1])) != (nx, ny):
            raise ValueError("plan_batch: every search needs the same mapbound")
        if any(len(o) != 3 for o in a.s.obstacle_list):
            raise ValueError("plan_batch: obstacles are circles [x, y, r]")
    masks = batch_masks(searchers)
    B = len(searchers)
    n_obs = max(len(a.s.obstacle_list) for a in searchers)
    obs = None
    if n_obs:
        obs = np.zeros((B, n_obs, 3))
        for b, a in enumerate(searchers):
            if a.s.obstacle_list:
                obs[b, : len(a.s.obstacle_list)] = a.s.obstacle_list
    return run(ctx, planner, searchers, nx, ny, 3, n_obs, obs, masks, path_field)
