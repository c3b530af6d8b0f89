"""CPU restatement of PathPlanning/CollisionDetection/src/utils.jl and of Hybrid A*'s block_collision_check
(PathPlanning/HybridAstar/src/hybrid_astar_utils.jl:180-204), written from the Julia, line by line.

Test infrastructure only: what tests/test_gpu_collide.py compares mp_block_pts, mp_convex_collision and
mp_path_collision with.  tests/test_collide_ref.py pins it against the C oracle (oracle/or_hastar.c), against
OpenBLAS's dgemv for the projections, and against the reference driver's two answers (main.jl:12, :19).

Rounding: the two BLAS-dispatched products round as oracle/or_blas.h states -- R*pts (utils.jl:24) is dgemm with
K = 2, fma(a1, b1, a0*b0); transpose(pts .- bg_pt)*normal_vec (utils.jl:48-49) is dgemv 'T' on two rows,
fma(A[0,j], x0, A[1,j]*x1).  `fma` is exact: the definition is `fma_exact` (rational arithmetic, as in
tests/astar_ref.py); libm's correctly rounded fma stands in for it when it is there (the pin test compares the
two), since the path tests make a few hundred thousand of them.  cos, sin and modπ are the library's Julia
restatements (include/mp_jlmath.h through oracle.m).
"""
import ctypes
import ctypes.util
import math
from fractions import Fraction

import numpy as np

import oracle

MP_SAT_BOTH, MP_SAT_EITHER, MP_SAT_BASE_A = 0, 1, 2


def fma_exact(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _libm_fma():
    try:
        f = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").fma
    except (OSError, AttributeError):
        return None
    f.restype = ctypes.c_double
    f.argtypes = [ctypes.c_double] * 3
    return f


fma = _libm_fma() or fma_exact


def jl_minimum(v):
    """Julia's minimum: a NaN element makes the result NaN."""
    return math.nan if any(x != x for x in v) else min(v)


def jl_maximum(v):
    return math.nan if any(x != x for x in v) else max(v)


def GetRectanglePts(block):
    """utils.jl:14-25 -> 2 x 5.  R = [cos ψ  -sin ψ; sin ψ  cos ψ] (:23); R*pts .+ [ox; oy] (:24)."""
    ox, oy, psi, length, width = (float(v) for v in block)
    pts = [(-length, width), (-length, -width), (length, -width), (length, width), (-length, width)]  # :22, columns
    c, s = oracle.m("cos", psi), oracle.m("sin", psi)
    out = np.zeros((2, 5))
    for j, (px, py) in enumerate(pts):
        out[0, j] = fma(-s, py, c * px) + ox
        out[1, j] = fma(c, py, s * px) + oy
    return out


def Block2Pts(block_info):
    """utils.jl:28-34 -> 2 x 5 x n."""
    pts = np.zeros((2, 5, len(block_info)))
    for i, b in enumerate(block_info):
        pts[:, :, i] = GetRectanglePts(b)
    return pts


def projections(pts, bg, n):
    """transpose(pts .- bg_pt) * normal_vec (utils.jl:48-49)."""
    return [fma(float(pts[0, j]) - bg[0], n[0], (float(pts[1, j]) - bg[1]) * n[1]) for j in range(pts.shape[1])]


def SeparatingAxisTheorem(pts_base, pts_other):
    """utils.jl:37-62: True = an edge normal of pts_base separates (no collision)."""
    for e in range(pts_base.shape[1] - 1):                                     # :39
        bg = (float(pts_base[0, e]), float(pts_base[1, e]))                    # :41
        ed = (float(pts_base[0, e + 1]), float(pts_base[1, e + 1]))            # :42
        base_vec = (ed[0] - bg[0], ed[1] - bg[1])                              # :44
        normal = (-base_vec[1], base_vec[0])                                   # :46
        base_dps = projections(pts_base, bg, normal)                           # :48
        other_dps = projections(pts_other, bg, normal)                         # :49
        min_base, max_base = jl_minimum(base_dps), jl_maximum(base_dps)        # :51-52
        min_other, max_other = jl_minimum(other_dps), jl_maximum(other_dps)    # :54-55
        if max_other <= min_base or max_base <= min_other:                     # :57
            return True
    return False


def ConvexCollision(pts1, pts2, mode=MP_SAT_BOTH):
    """utils.jl:64-74 (True = no collision); MP_SAT_EITHER and MP_SAT_BASE_A as include/mpgpu.h defines them."""
    a = SeparatingAxisTheorem(pts1, pts2)
    if mode == MP_SAT_BASE_A:
        return a
    if mode == MP_SAT_BOTH:
        return a and SeparatingAxisTheorem(pts2, pts1)
    return a or SeparatingAxisTheorem(pts2, pts1)


def sat_pair(pts1, pts2):
    """(SAT(1, 2), SAT(2, 1)): the three modes of one pair are functions of these two."""
    return SeparatingAxisTheorem(pts1, pts2), SeparatingAxisTheorem(pts2, pts1)


def mode_of(s12, s21, mode):
    return s12 if mode == MP_SAT_BASE_A else (s12 and s21) if mode == MP_SAT_BOTH else (s12 or s21)


def checked_indices(n, sparcity_num):
    """hybrid_astar_utils.jl:182-190: 1:sparcity_num:end when size(path, 2) > sparcity_num, else column 1."""
    if n <= 0:
        return []
    return list(range(0, n, sparcity_num)) if n > sparcity_num else [0]


def vehicle_block(pose, half_len, half_wid, center_shift):
    """hybrid_astar_utils.jl:193 with vehicle_size[1]/2 as center_shift."""
    x, y, psi = (float(v) for v in pose)
    return [x + center_shift * oracle.m("cos", psi), y + center_shift * oracle.m("sin", psi), oracle.m("modpi", psi),
            half_len, half_wid]


def path_check(half_len, half_wid, path, block_list, sparcity_num=5, center_shift=None, mode=MP_SAT_BOTH):
    """block_collision_check (:180-204) on path[n][3] with the per-pose detail mp_path_collision returns:
    dict(scene_free, first_pose, first_wall, n_hit, pose_free[n])."""
    path = np.asarray(path, float).reshape(-1, 3)
    shift = half_len if center_shift is None else center_shift
    wall_pts = Block2Pts(block_list) if len(block_list) else np.zeros((2, 5, 0))    # :194
    pose_free = np.full(len(path), 2, np.uint8)
    first_pose = first_wall = -1
    n_hit = 0
    for j in checked_indices(len(path), sparcity_num):
        veh = GetRectanglePts(vehicle_block(path[j], half_len, half_wid, shift))    # :195
        hit = -1
        for i in range(wall_pts.shape[2]):
            if not ConvexCollision(wall_pts[:, :, i], veh, mode):                   # :198
                hit = i
                break
        pose_free[j] = 0 if hit >= 0 else 1
        if hit >= 0:
            n_hit += 1
            if first_pose < 0:
                first_pose, first_wall = j, hit
    return dict(scene_free=first_pose < 0, first_pose=first_pose, first_wall=first_wall, n_hit=n_hit,
                pose_free=pose_free)


def block_collision_check(vehicle_size, path, block_list, sparcity_num=5):
    """:180-204 for a 3 x n path: the reference's boolean."""
    path = np.asarray(path, float)
    return path_check(vehicle_size[0] / 2, vehicle_size[1] / 2, path.T, block_list, sparcity_num)["scene_free"]
