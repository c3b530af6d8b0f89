"""Occupancy-map tools over the libmpgpu C-ABI (mp_grid_rasterize, mp_grid_distance, mp_grid_inflate,
mp_grid_path_clearance; include/mpgpu.h, "occupancy maps") -- an extension: the reference has none of them.

A map is the grid planners' free-cell mask: uint8 [ny, nx], cell (ix, iy) (1-based) at mask[iy-1, ix-1], any nonzero
byte = free.  ``distance2`` is the exact squared Euclidean distance, in cells, to the nearest blocked cell (int32, 0 on a
blocked cell, D2_NONE on a map without one); ``border=True`` counts a one-cell frame around the map as blocked.
``inflate`` grows the blocked cells by a robot radius: a cell stays free iff it is free and its distance2 exceeds r2.
Every function takes one map [ny, nx] or a batch [B, ny, nx] and returns the same rank.

``r2_of_radius``, ``inflate_searcher_`` and ``mppi_grid`` tie the maps to the planners: a searcher's obstacle list
or mask inflated by a radius in metres, and a mask as the occupied-polarity grid ``defineMPPIgrid_`` takes.
"""
import math
from fractions import Fraction

import numpy as np

from . import _gridsearch
from .abi import MP_MAP_BORDER, MP_MAP_D2_NONE, MP_MAP_OUT_OCCUPIED, ptr
from .context import default_context

D2_NONE = MP_MAP_D2_NONE


def _batch(masks):
    m = np.asarray(masks)
    if m.dtype != np.uint8 or m.ndim not in (2, 3):
        raise ValueError("a map is a uint8 array [ny, nx], a batch [B, ny, nx]")
    return np.ascontiguousarray(m.reshape((-1,) + m.shape[-2:])), m.ndim == 2


def _flags(border, occupied=False):
    return (MP_MAP_BORDER if border else 0) | (MP_MAP_OUT_OCCUPIED if occupied else 0)


def r2_of_radius(radius_cells):
    """The r2 of a disc of radius_cells cells: a cell is taken when d2 <= radius^2, and d2 is an integer, so
    r2 = floor(radius^2) (formed exactly, capped at INT32_MAX)."""
    r = float(radius_cells)
    if not math.isfinite(r) or r < 0.0:
        raise ValueError("the radius must be finite and >= 0")
    return min(math.floor(Fraction(r) ** 2), 2 ** 31 - 1)


def rasterize(searchers, ctx=None):
    """The free-cell masks [B, ny, nx] the planners build for these searchers (A*, Dijkstra or BFS, sharing
    mapbound): one mp_grid_rasterize call for the searchers with an obstacle list (circles or blocks, one kind a
    batch; a shorter list is padded with repeats of its first obstacle, which change nothing).  A searcher with an
    empty list is all free, one that carries a mask gives that mask."""
    a0 = searchers[0]
    nx, ny = int(a0.s.mapbound[0]), int(a0.s.mapbound[1])
    out = np.ones((len(searchers), ny, nx), np.uint8)
    listed = []
    for b, a in enumerate(searchers):
        if (int(a.s.mapbound[0]), int(a.s.mapbound[1])) != (nx, ny):
            raise ValueError("rasterize: every searcher needs the same mapbound")
        if getattr(a.s, "free_mask", None) is not None:
            out[b] = a.s.free_mask
        elif a.s.obstacle_list:
            listed.append(b)
    if not listed:
        return out
    kind = len(searchers[listed[0]].s.obstacle_list[0])
    n_obs = max(len(searchers[b].s.obstacle_list) for b in listed)
    obs = np.zeros((len(listed), n_obs, kind))
    for i, b in enumerate(listed):
        ol = searchers[b].s.obstacle_list
        if kind not in (3, 5) or any(len(o) != kind for o in ol):
            raise ValueError("rasterize: obstacles are circles [x, y, r] or blocks [x, y, psi, l/2, w/2], one kind a batch")
        obs[i, : len(ol)] = ol
        obs[i, len(ol):] = ol[0]
    bound = np.ascontiguousarray([searchers[b].s.actualbound for b in listed], np.float64)
    masks = np.zeros((len(listed), ny, nx), np.uint8)
    ctx = ctx or default_context()
    ctx.check(ctx.lib.mp_grid_rasterize(ctx.handle, len(listed), nx, ny, ptr(bound), kind, n_obs, ptr(obs), ptr(masks)))
    out[listed] = masks
    return out


def distance2(masks, border=False, ctx=None):
    """int32 squared distance, in cells, from each cell to the nearest blocked cell (mp_grid_distance)."""
    m, single = _batch(masks)
    ctx = ctx or default_context()
    d2 = np.zeros(m.shape, np.int32)
    ctx.check(ctx.lib.mp_grid_distance(ctx.handle, _flags(border), m.shape[0], m.shape[2], m.shape[1], ptr(m), ptr(d2)))
    return d2[0] if single else d2


def inflate(masks, radius=None, r2=None, border=False, occupied=False, ctx=None):
    """The maps with their blocked cells grown (mp_grid_inflate): 1 = free iff the cell is free and its distance2
    exceeds r2.  Give either ``radius`` in cells (r2_of_radius) or ``r2`` itself, a scalar or one value per map.
    ``occupied=True`` writes the opposite polarity, 1 = occupied (MPPI's grid)."""
    if (radius is None) == (r2 is None):
        raise ValueError("inflate: give either radius or r2")
    m, single = _batch(masks)
    B = m.shape[0]
    if r2 is None:
        r2 = [r2_of_radius(r) for r in np.broadcast_to(np.asarray(radius, np.float64), (B,))]
    r2 = np.ascontiguousarray(np.broadcast_to(np.asarray(r2, np.int64), (B,)))
    if (r2 < 0).any() or (r2 > 2 ** 31 - 1).any():
        raise ValueError("inflate: r2 must be 0 .. 2^31 - 1")
    r2 = r2.astype(np.int32)
    ctx = ctx or default_context()
    out = np.zeros(m.shape, np.uint8)
    ctx.check(ctx.lib.mp_grid_inflate(ctx.handle, _flags(border, occupied), B, m.shape[2], m.shape[1], ptr(m), ptr(r2),
                                      ptr(out)))
    return out[0] if single else out


def path_clearance(masks, paths, path_n, border=False, ctx=None):
    """(min_d2, at) of paths as mp_grid_plan writes them (Encode values 1..nx*ny, [B, stride] with path_n [B] valid
    entries each; an entry of 0 is skipped): the least distance2 over a path's cells and the index of the first
    entry that attains it; (D2_NONE, -1) for an empty path (mp_grid_path_clearance)."""
    m, single = _batch(masks)
    B = m.shape[0]
    p = np.ascontiguousarray(np.asarray(paths, np.int32).reshape(B, -1))
    n = np.ascontiguousarray(np.asarray(path_n, np.int32).reshape(B))
    ctx = ctx or default_context()
    md, at = np.zeros(B, np.int32), np.zeros(B, np.int32)
    ctx.check(ctx.lib.mp_grid_path_clearance(ctx.handle, _flags(border), B, m.shape[2], m.shape[1], ptr(m), ptr(p), ptr(n),
                                             p.shape[1], ptr(md), ptr(at)))
    return (int(md[0]), int(at[0])) if single else (md, at)


def inflate_searcher_(a, radius_m, border=False, ctx=None):
    """Plan for a disc robot of radius_m metres: the searcher's obstacle list (rasterised) or mask, inflated by
    radius_m / x_factor cells, becomes its mask (_gridsearch.define_mask).  Distances are in cells, so the cells must
    be square."""
    if a.s.x_factor != a.s.y_factor:
        raise ValueError("inflate_searcher_: x_factor != y_factor, the cells are not square")
    mask = getattr(a.s, "free_mask", None)
    if mask is None:
        mask = rasterize([a], ctx=ctx)[0]
    _gridsearch.define_mask(a, inflate(mask, radius=float(radius_m) / a.s.x_factor, border=border, ctx=ctx))


def mppi_grid(a, mask):
    """(grid, spec) for defineMPPIgrid_ from a searcher's geometry and a free-cell mask: the occupied polarity, and
    cells that start at the searcher's bound -- x0 = xmin, y0 = ymin, dx = x_factor, dy = y_factor -- so that a point
    the planners put in cell (ix, iy) reads grid[iy-1, ix-1]."""
    m = np.asarray(mask)
    ny, nx = int(a.s.mapbound[1]), int(a.s.mapbound[0])
    if m.shape != (ny, nx):
        raise ValueError("the mask must have shape [ny, nx] = [mapbound[1], mapbound[0]]")
    spec = dict(nx=nx, ny=ny, x0=float(a.s.actualbound[0]), y0=float(a.s.actualbound[2]), dx=float(a.s.x_factor),
                dy=float(a.s.y_factor))
    return np.ascontiguousarray(m == 0, np.uint8), spec
