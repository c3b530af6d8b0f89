"""Batched collision detection on the device (PathPlanning/CollisionDetection/src/utils.jl and Hybrid A*'s
block_collision_check, HybridAstar/src/hybrid_astar_utils.jl:180-204) through mp_block_pts,
mp_convex_collision and mp_path_collision.

The functions with the reference's names take and return the reference's shapes (a polygon is a 2 x m
matrix, a path 3 x n, Block2Pts returns 2 x 5 x n); `block_pts`, `convex_collision` and `path_collision`
are the batched calls in the C layout.  `check_path` answers the question the planners' outputs raise:
does `actualpath` (hybrid_astar.retrieve_batch) or `states_his` (tracker.track_batch) touch a wall?
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from .abi import MP_COLLIDE_MAX_COLS, MP_SAT_BASE_A, MP_SAT_BOTH, MP_SAT_EITHER, CollideParams, f64, ptr
from .context import default_context

__all__ = ["GetRectanglePts", "Block2Pts", "SeparatingAxisTheorem", "ConvexCollision", "collision_matrix",
           "block_collision_check", "check_path", "PathCheck", "block_pts", "convex_collision", "path_collision",
           "collide_params", "MP_SAT_BOTH", "MP_SAT_EITHER", "MP_SAT_BASE_A", "MP_COLLIDE_MAX_COLS"]


# ------------------------------------------------------------------ batched calls, C layout
def block_pts(blocks, ctx=None):
    """GetRectanglePts of blocks[n][5] ([x, y, ψ, l, w]) -> pts[n][5][2]."""
    ctx = ctx or default_context()
    blocks = f64(blocks).reshape(-1, 5)
    pts = np.zeros((len(blocks), 5, 2))
    ctx.check(ctx.lib.mp_block_pts(ctx.handle, len(blocks), ptr(blocks), ptr(pts)))
    return pts


def convex_collision(polys_a, polys_b, a_cols=None, b_cols=None, mode=MP_SAT_BOTH, ctx=None):
    """free[B][na][nb] (1 = no collision) for polys_a[B][na][ma][2], polys_b[B][nb][mb][2] and the column
    counts a_cols[B][na], b_cols[B][nb] (None: ma / mb each)."""
    ctx = ctx or default_context()
    polys_a, polys_b = f64(polys_a), f64(polys_b)
    B, na, ma, _ = polys_a.shape
    Bb, nb, mb, _ = polys_b.shape
    assert B == Bb, "polys_a and polys_b hold different scene counts"
    ac = None if a_cols is None else np.ascontiguousarray(a_cols, np.int32).reshape(B, na)
    bc = None if b_cols is None else np.ascontiguousarray(b_cols, np.int32).reshape(B, nb)
    free = np.zeros((B, na, nb), np.uint8)
    ctx.check(ctx.lib.mp_convex_collision(ctx.handle, int(mode), B, na, ma, ptr(polys_a), ptr(ac), nb, mb,
                                          ptr(polys_b), ptr(bc), ptr(free)))
    return free


def collide_params(vehicle_size, stride=5, center_shift=None, mode=MP_SAT_BOTH):
    """mp_collide_params for a vehicle [length, width]; center_shift None: the reference's half length."""
    p = CollideParams()
    p.half_len = float(vehicle_size[0]) / 2
    p.half_wid = float(vehicle_size[1]) / 2
    p.center_shift = p.half_len if center_shift is None else float(center_shift)
    p.stride = int(stride)
    p.mode = int(mode)
    return p


def path_collision(p, poses, walls, pose_count=None, wall_count=None, want_pose_free=True, ctx=None):
    """mp_path_collision for poses[B][n_poses][3] against walls[B][n_walls][5]: dict(scene_free, first_pose,
    first_wall, n_hit, pose_free)."""
    ctx = ctx or default_context()
    poses = f64(poses)
    B, n_poses, _ = poses.shape
    walls = f64(walls).reshape(B, -1, 5)
    n_walls = walls.shape[1]
    pc = None if pose_count is None else np.ascontiguousarray(pose_count, np.int32).reshape(B)
    wc = None if wall_count is None else np.ascontiguousarray(wall_count, np.int32).reshape(B)
    out = dict(scene_free=np.zeros(B, np.uint8), first_pose=np.zeros(B, np.int32), first_wall=np.zeros(B, np.int32),
               n_hit=np.zeros(B, np.int32), pose_free=np.zeros((B, n_poses), np.uint8) if want_pose_free else None)
    ctx.check(ctx.lib.mp_path_collision(ctx.handle, ctypes.byref(p), B, n_poses, ptr(poses), ptr(pc), n_walls, ptr(wc),
                                        ptr(walls), ptr(out["scene_free"]), ptr(out["first_pose"]),
                                        ptr(out["first_wall"]), ptr(out["n_hit"]), ptr(out["pose_free"])))
    return out


# ------------------------------------------------------------------ the reference's names and shapes
def GetRectanglePts(block, ctx=None):
    """utils.jl:14-25: the 2 x 5 corner matrix of block [x, y, ψ, l, w]."""
    return block_pts(f64(block).reshape(1, 5), ctx)[0].T.copy()


def Block2Pts(block_info, ctx=None):
    """utils.jl:28-34: 2 x 5 x n for a list of n blocks."""
    return np.ascontiguousarray(block_pts(block_info, ctx).transpose(2, 1, 0))


def _cols(pts):
    pts = f64(pts)
    assert pts.ndim == 2 and pts.shape[0] == 2, "a polygon is a 2 x m matrix"
    return np.ascontiguousarray(pts.T)


def SeparatingAxisTheorem(pts_base, pts_other, ctx=None):
    """utils.jl:37-62: True when an edge normal of pts_base separates the two (no collision)."""
    a, b = _cols(pts_base), _cols(pts_other)
    return bool(convex_collision(a[None, None], b[None, None], mode=MP_SAT_BASE_A, ctx=ctx)[0, 0, 0])


def ConvexCollision(pts1, pts2, either=False, ctx=None):
    """utils.jl:64-74: SeparatingAxisTheorem(pts1, pts2) && SeparatingAxisTheorem(pts2, pts1); True = no
    collision.  either=True is the geometric test, || in place of && (an extension)."""
    a, b = _cols(pts1), _cols(pts2)
    mode = MP_SAT_EITHER if either else MP_SAT_BOTH
    return bool(convex_collision(a[None, None], b[None, None], mode=mode, ctx=ctx)[0, 0, 0])


def _pack(scenes):
    """Scenes of ragged 2 x m polygons -> (polys[B][n][mmax][2] with NaN padding, cols[B][n])."""
    n = len(scenes[0])
    assert all(len(s) == n for s in scenes), "every scene holds the same number of polygons"
    cols = np.array([[np.shape(q)[1] for q in s] for s in scenes], np.int32).reshape(len(scenes), n)
    polys = np.full((len(scenes), n, int(cols.max()) if cols.size else 2, 2), np.nan)
    for b, s in enumerate(scenes):
        for i, q in enumerate(s):
            polys[b, i, : cols[b, i]] = _cols(q)
    return polys, cols


def collision_matrix(polys_a, polys_b, mode=MP_SAT_BOTH, ctx=None):
    """All pairs in one call.  polys_a / polys_b: lists of 2 x m polygons (m may differ from polygon to
    polygon) -> bool[na][nb]; or lists of such lists, one per scene, -> bool[B][na][nb].  True = no collision."""
    single = np.ndim(polys_a[0][0]) == 1  # polys_a[0] is a 2 x m matrix, not a scene's list of them
    sa, sb = ([polys_a], [polys_b]) if single else (polys_a, polys_b)
    pa, ca = _pack(sa)
    pb, cb = _pack(sb)
    free = convex_collision(pa, pb, ca, cb, mode, ctx).astype(bool)
    return free[0] if single else free


def block_collision_check(vehicle_size, path, block_list, sparcity_num=5, ctx=None):
    """hybrid_astar_utils.jl:180-204 for one 3 x n path: True when no checked pose hits a block."""
    return check_path(vehicle_size, path, block_list, stride=sparcity_num, ctx=ctx).free


@dataclass
class PathCheck:
    free: bool              # block_collision_check's return value
    first_pose: int         # lowest checked column that hits a block, -1 if none
    first_wall: int         # lowest block that column hits, -1 if none
    n_hit: int              # checked columns that hit at least one block
    pose_free: np.ndarray   # per column: 1 free, 0 hit, 2 not checked


def check_path(vehicle_size, states, block_list, stride=1, center_shift=None, ctx=None):
    """Sweep the vehicle along states (3 x n: x, y, ψ per column, as actualpath and states_his are) against
    block_list ([x, y, ψ, l/2, w/2] each) with the reference's test, every stride-th column."""
    states = f64(states)
    assert states.ndim == 2 and states.shape[0] == 3, "states is a 3 x n matrix"
    walls = f64(block_list).reshape(1, -1, 5)
    p = collide_params(vehicle_size, stride, center_shift)
    r = path_collision(p, np.ascontiguousarray(states.T)[None], walls, ctx=ctx)
    return PathCheck(bool(r["scene_free"][0]), int(r["first_pose"][0]), int(r["first_wall"][0]), int(r["n_hit"][0]),
                     r["pose_free"][0])
