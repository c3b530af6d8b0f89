"""Goal-distance fields on occupancy maps over the libmpgpu C-ABI (mp_grid_field; include/mpgpu.h, "goal-distance
fields") -- an extension: the labels planDKA! would leave in nodes_collection if it ran until its open list were empty.

A map is the grid planners' free-cell mask (uint8 [ny, nx], nonzero = free) with their geometry: ``bound`` =
[xmin, xmax, ymin, ymax] per map, cells by defineAstar's floor.  ``cost_field`` gives, for every cell, the cost of the
cheapest way from the source cell to it over the moves in ``moves`` ("ref": the reference's seven, "8", "4", or a bit
set, see MOVES); float64, +Inf on blocked and unreached cells, and n_reached, the number of finite cells.
``to_source=True`` gives the cost of travelling from each cell to the source instead.  ``field_paths`` reads costs and
paths for query points off the field; a path is in travel order, as Encode indices, the form ``gridmap.path_clearance``
takes.  Every function takes one map [ny, nx] or a batch [B, ny, nx] and returns the same rank.
"""
import numpy as np

from . import gridmap
from .abi import (MP_FIELD_MOVES_4, MP_FIELD_MOVES_8, MP_FIELD_MOVES_REF, MP_FIELD_TO_SOURCE, f64, ptr)
from .context import default_context

# the neighbour (dx, dy) of each bit of a move set
MOVES = [(-1, 0), (-1, -1), (1, -1), (1, 0), (1, 1), (0, -1), (0, 1), (-1, 1)]
MOVE_SETS = {"ref": MP_FIELD_MOVES_REF, "8": MP_FIELD_MOVES_8, "4": MP_FIELD_MOVES_4}


def _moves(moves):
    return MOVE_SETS[moves] if isinstance(moves, str) else int(moves)


def _maps(masks, bound, source_real):
    m = np.asarray(masks)
    if m.dtype != np.uint8 or m.ndim not in (2, 3):
        raise ValueError("a map is a uint8 array [ny, nx], a batch [B, ny, nx]")
    single = m.ndim == 2
    m = np.ascontiguousarray(m.reshape((-1,) + m.shape[-2:]))
    B = m.shape[0]
    bound = np.ascontiguousarray(np.broadcast_to(f64(bound).reshape(-1, 4), (B, 4)))
    src = np.ascontiguousarray(np.broadcast_to(f64(source_real).reshape(-1, 2), (B, 2)))
    return m, bound, src, single


def cost_field(masks, bound, source_real, moves="ref", to_source=False, ctx=None):
    """(field, n_reached) of mp_grid_field: float64 [ny, nx] and an int for one map, [B, ny, nx] and int32 [B] for a
    batch.  ``bound`` and ``source_real`` are one per map, or one for all."""
    m, bound, src, single = _maps(masks, bound, source_real)
    B, ny, nx = m.shape
    ctx = ctx or default_context()
    field, n = np.zeros(m.shape, np.float64), np.zeros(B, np.int32)
    ctx.check(ctx.lib.mp_grid_field(ctx.handle, MP_FIELD_TO_SOURCE if to_source else 0, _moves(moves), B, nx, ny,
                                    ptr(bound), ptr(src), ptr(m), ptr(field), ptr(n), 0, None, None, 0, None, None,
                                    None, None))
    return (field[0], int(n[0])) if single else (field, n)


def field_paths(masks, bound, source_real, q_map, q_real, stride=None, moves="ref", to_source=False, want_field=False,
                ctx=None):
    """Costs and paths of Q queries: query q reads map q_map[q] (ignored for one map) at the cell of q_real[q].
    Returns a dict: q_cost [Q] (+Inf off the grid or unreached), path int32 [Q, stride] (Encode indices in travel order:
    source -> query, with to_source query -> source; entries past a path's end are -1), path_n [Q] (the full length,
    which may exceed stride: the path is then cut), path_length [Q]; and field, n_reached with want_field.
    ``stride=None`` takes the bound of any path, the largest number of free cells of a queried map plus one; give a
    stride on large open maps."""
    m, bound, src, single = _maps(masks, bound, source_real)
    B, ny, nx = m.shape
    qr = np.ascontiguousarray(f64(q_real).reshape(-1, 2))
    Q = qr.shape[0]
    qm = np.zeros(Q, np.int32) if single and q_map is None else np.ascontiguousarray(np.asarray(q_map, np.int32).reshape(Q))
    if Q == 0:
        raise ValueError("field_paths: no query; cost_field gives the field alone")
    if stride is None:
        used = np.unique(qm[(qm >= 0) & (qm < B)])
        stride = min(nx * ny, 1 + max((int(np.count_nonzero(m[b])) for b in used), default=0))
    ctx = ctx or default_context()
    out = dict(q_cost=np.zeros(Q), path=np.full((Q, int(stride)), -1, np.int32), path_n=np.zeros(Q, np.int32),
               path_length=np.zeros(Q))
    field = n = None
    if want_field:
        field, n = np.zeros(m.shape, np.float64), np.zeros(B, np.int32)
    ctx.check(ctx.lib.mp_grid_field(ctx.handle, MP_FIELD_TO_SOURCE if to_source else 0, _moves(moves), B, nx, ny,
                                    ptr(bound), ptr(src), ptr(m), ptr(field), ptr(n), Q, ptr(qm), ptr(qr), int(stride),
                                    ptr(out["q_cost"]), ptr(out["path"]), ptr(out["path_n"]), ptr(out["path_length"])))
    if want_field:
        out["field"], out["n_reached"] = (field[0], int(n[0])) if single else (field, n)
    return out


def field_of_searcher_(a, source_real=None, moves="ref", to_source=False, ctx=None):
    """(field, n_reached) on the map of a grid searcher (A*, Dijkstra or BFS): its bound and mapbound, its mask, or
    its obstacle list rasterised (gridmap.rasterize), and its starting_real as the source unless one is given."""
    mask = gridmap.rasterize([a], ctx=ctx)[0]
    src = a.s.starting_real if source_real is None else source_real
    return cost_field(mask, a.s.actualbound, src, moves=moves, to_source=to_source, ctx=ctx)
