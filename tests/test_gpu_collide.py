"""GPU parity of the collision calls (mp_block_pts, mp_convex_collision, mp_path_collision and their wrappers in
motionplanning_amd/collision.py) against the C oracle and the CPU restatement tests/collide_ref.py.  Every
comparison is exact equality: the outputs are booleans, indices and bit-exact doubles."""
import ctypes
import math

import numpy as np
import pytest

import collide_ref as R
import oracle
from motionplanning_amd import collision as C
from motionplanning_amd import hybrid_astar as ha
from motionplanning_amd import tracker
from motionplanning_amd.abi import MP_ERR_INVALID, CollideParams, ptr

pytestmark = pytest.mark.gpu

WALL_TILE = 32     # collide.hip: walls per LDS tile
POSE_CHUNK = 256   # collide.hip: checked poses per block
MODES = (C.MP_SAT_BOTH, C.MP_SAT_EITHER, C.MP_SAT_BASE_A)
PARKING = np.array(ha.PERPENDICULAR["walls"])
VEH = (3.0, 2.0)   # the driver's vehicle_size


def _ref_paths(p, poses, walls, pose_count=None, wall_count=None):
    """collide_ref.path_check per scene, stacked like path_collision's outputs."""
    B, n, _ = poses.shape
    out = dict(scene_free=np.zeros(B, np.uint8), first_pose=np.zeros(B, np.int32), first_wall=np.zeros(B, np.int32),
               n_hit=np.zeros(B, np.int32), pose_free=np.full((B, n), 2, np.uint8))
    for b in range(B):
        cnt = n if pose_count is None else pose_count[b]
        nw = walls.shape[1] if wall_count is None else wall_count[b]
        r = R.path_check(p.half_len, p.half_wid, poses[b, :cnt], walls[b, :nw], p.stride, p.center_shift, p.mode)
        for k in ("scene_free", "first_pose", "first_wall", "n_hit"):
            out[k][b] = r[k]
        out["pose_free"][b, :cnt] = r["pose_free"]
    return out


def _same(got, want):
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


# 1 ------------------------------------------------------------------------------------------------
def test_block_pts_bitexact(ctx):
    """1,000 blocks, ψ in ±4π, centres up to 1e5 m: or_ha_rect_pts and the restatement, bit for bit."""
    r = np.random.default_rng(1)
    n = 1000
    blocks = np.c_[r.uniform(-1e5, 1e5, (n, 2)), r.uniform(-4 * np.pi, 4 * np.pi, n), r.uniform(0.1, 5, (n, 2))]
    blocks[:4, 2] = [0.0, np.pi, -np.pi, 4 * np.pi]
    pts = C.block_pts(blocks, ctx)
    L = oracle._ha()
    want = np.zeros(10)
    for i in range(n):
        L.or_ha_rect_pts(ptr(blocks[i]), ptr(want))
        assert np.array_equal(pts[i].ravel(), want), i
    for i in range(0, n, 50):
        assert np.array_equal(pts[i].T, R.GetRectanglePts(blocks[i]))
    assert np.array_equal(C.Block2Pts(blocks[:7], ctx), R.Block2Pts(blocks[:7]))
    assert np.array_equal(C.GetRectanglePts(blocks[9], ctx), R.GetRectanglePts(blocks[9]))


# 2 ------------------------------------------------------------------------------------------------
def test_reference_driver_cases(ctx):
    """CollisionDetection/main.jl: true at :12 (vehicle beside the wall), false at :19 (triangle in the wall)."""
    block_info = [[0.0, -1.0, 0.0, 5.5 / 2 + 1.0, 1.0], [-5.5 / 2, 2.7432 / 2, 0.0, 1.0, 2.7432 / 2],
                  [5.5 / 2, 2.7432 / 2, 0.0, 1.0, 2.7432 / 2]]
    pts = C.Block2Pts(block_info, ctx)
    veh_pts = C.GetRectanglePts([5.5, 1.0, 0, 3 / 2, 2 / 2], ctx)
    assert C.ConvexCollision(pts[:, :, 0], veh_pts, ctx=ctx) is True
    cur, eps = [0.0, -1.0], 1e-1
    mypts = np.array([[cur[0], cur[1] + eps], [cur[0] - eps, cur[1]], [cur[0] + eps, cur[1]], [cur[0], cur[1] + eps]]).T
    assert C.ConvexCollision(pts[:, :, 0], mypts, ctx=ctx) is False


# 3 ------------------------------------------------------------------------------------------------
def test_rectangle_all_pairs_three_modes(ctx):
    """B = 1, na = nb = 64 rectangles in a 6 m box, half extents 0.5-2, under all three modes, against the oracle
    (BOTH) and the restatement (all)."""
    r = np.random.default_rng(7)
    n = 64

    def blocks():
        return np.c_[r.uniform(0, 6, (n, 2)), r.uniform(-np.pi, np.pi, n), r.uniform(0.5, 2, (n, 2))]

    pa, pb = C.block_pts(blocks(), ctx), C.block_pts(blocks(), ctx)
    s12 = np.zeros((n, n), bool)
    s21 = np.zeros((n, n), bool)
    orc = np.zeros((n, n), bool)
    for i in range(n):
        for j in range(n):
            s12[i, j], s21[i, j] = R.sat_pair(pa[i].T, pb[j].T)
            orc[i, j] = oracle.ha_convex_free(pa[i], pb[j])
    both, either = s12 & s21, s12 | s21
    assert np.array_equal(both, orc)
    assert 0.2 <= both.mean() <= 0.8
    assert (both != either).mean() >= 0.03
    want = {C.MP_SAT_BOTH: both, C.MP_SAT_EITHER: either, C.MP_SAT_BASE_A: s12}
    for mode in MODES:
        got = C.convex_collision(pa[None], pb[None], mode=mode, ctx=ctx)[0]
        assert np.array_equal(got.astype(bool), want[mode]), mode


# 4 ------------------------------------------------------------------------------------------------
def test_touching_rectangles(ctx):
    """Exactly touching is free (`<=` on both sides of utils.jl:57); one ulp inward is a hit."""
    a = C.GetRectanglePts([0, 0, 0, 1, 1], ctx)
    assert C.ConvexCollision(a, C.GetRectanglePts([2, 0, 0, 1, 1], ctx), ctx=ctx) is True
    inward = C.GetRectanglePts([math.nextafter(2.0, 0.0), 0, 0, 1, 1], ctx)
    assert inward[0, 0] < 1.0
    assert C.ConvexCollision(a, inward, ctx=ctx) is False
    # under || the rounding of the shifted rectangle's far corners (2.9999999999999998 -> 3.0) lets its own far
    # edge separate: the restatement's answer, whatever it is
    assert C.ConvexCollision(a, inward, either=True, ctx=ctx) is R.ConvexCollision(a, inward, R.MP_SAT_EITHER)


# 5 ------------------------------------------------------------------------------------------------
def _polygon(r, cols):
    """A closed convex polygon of `cols` columns (cols - 1 vertices on an ellipse + the first again); cols = 2 is a
    segment."""
    k = max(cols - 1, 2) if cols > 2 else 2
    c = r.uniform(0, 6, 2)
    ang = np.sort(r.uniform(0, 2 * np.pi, k)) + r.uniform(0, 1)
    v = c[:, None] + np.array([np.cos(ang), np.sin(ang)]) * r.uniform(0.5, 2.5, (2, 1))
    return np.ascontiguousarray(np.c_[v, v[:, :1]] if cols > 2 else v)


def test_ragged_general_polygons(ctx):
    """cols 2 ... 32 in one call, NaN in the padding, na != nb, B = 3, all three modes, against the restatement."""
    r = np.random.default_rng(9)
    B, na, nb = 3, 12, 7
    ca = np.array([[2, 3, 32] + list(r.integers(3, 33, na - 3)) for _ in range(B)])
    cb = np.array([[31, 2, 4] + list(r.integers(3, 33, nb - 3)) for _ in range(B)])
    sa = [[_polygon(r, c) for c in row] for row in ca]
    sb = [[_polygon(r, c) for c in row] for row in cb]
    assert all(q.shape == (2, c) for row, cr in zip(sa, ca) for q, c in zip(row, cr))
    s12 = np.array([[[R.SeparatingAxisTheorem(a, b) for b in sb[s]] for a in sa[s]] for s in range(B)])
    s21 = np.array([[[R.SeparatingAxisTheorem(b, a) for b in sb[s]] for a in sa[s]] for s in range(B)])
    assert s12.any() and not s12.all() and (s12 != s21).any()
    for mode, want in ((C.MP_SAT_BOTH, s12 & s21), (C.MP_SAT_EITHER, s12 | s21), (C.MP_SAT_BASE_A, s12)):
        got = C.collision_matrix(sa, sb, mode=mode, ctx=ctx)
        assert got.shape == (B, na, nb) and np.array_equal(got, want), mode
    one = C.collision_matrix(sa[1], sb[1], ctx=ctx)
    assert np.array_equal(one, (s12 & s21)[1])


def test_polygons_beyond_the_lds_budget(ctx):
    """A scene whose polygons do not fit the LDS staging (2 x 200 polygons of 32 columns) takes the kernel that
    reads them where they lie: the same answers, on a sample of the pairs."""
    r = np.random.default_rng(10)
    n = 200
    sa, sb = [_polygon(r, 32) for _ in range(n)], [_polygon(r, 32) for _ in range(n)]
    got = C.collision_matrix(sa, sb, ctx=ctx)
    for i, j in zip(r.integers(0, n, 60), r.integers(0, n, 60)):
        assert got[i, j] == R.ConvexCollision(sa[i], sb[j]), (i, j)
    assert got.any() and not got.all()


# 6 ------------------------------------------------------------------------------------------------
def test_repeated_base_vertex_and_nan_projection(ctx):
    """A repeated vertex gives a zero normal: every projection is 0 and the edge `separates` (free although
    overlapping).  A NaN projection (an overflow) leaves neither comparison true, as Julia's minimum does."""
    d = np.array([[0, 0], [0, 0], [1, 0], [1, 1], [0, 0]], float).T
    inside = C.GetRectanglePts([0.5, 0.3, 0, 0.1, 0.1], ctx)
    assert C.SeparatingAxisTheorem(d, inside, ctx=ctx) is True
    assert C.SeparatingAxisTheorem(inside, d, ctx=ctx) is False
    assert C.ConvexCollision(d, inside, ctx=ctx) is False and C.ConvexCollision(d, inside, either=True, ctx=ctx) is True
    big = np.array([[-1e308, 0], [0, 0]], float).T
    far = np.array([[0, 1], [1e308, 1]], float).T
    assert R.SeparatingAxisTheorem(big, far) is False
    assert C.SeparatingAxisTheorem(big, far, ctx=ctx) is False


# 7 ------------------------------------------------------------------------------------------------
def test_paths_at_the_reference_stride(ctx):
    """sparcity_num = 5 on paths of 1, 5, 6, 250 and 501 poses against the driver's three parking walls:
    scene_free is oracle.ha_block_free's boolean, the detail the restatement's; both outcomes present."""
    h = ha.driver_searcher(ha.PERPENDICULAR)
    hp = ha.params_of(h)
    p = C.collide_params(h.s.vehicle_size)
    r = np.random.default_rng(5)
    seen = set()
    for n in (1, 5, 6, 250, 501):
        B = 6
        t = np.linspace(0, 1, n)[None, :, None]
        a = np.c_[r.uniform(-4, 8, B), r.uniform(3.2, 8, B), r.uniform(-7, 7, B)][:, None, :]
        d = np.c_[r.uniform(-6, 6, B), -r.uniform(0, 7, B), r.uniform(-2, 2, B)][:, None, :]
        d[0] = 0.0
        a[0] = [7.0, 5.0, 1.0]  # an aisle pose that stays: free
        poses = np.ascontiguousarray(a + t * d)
        walls = np.tile(PARKING, (B, 1, 1))
        got = C.path_collision(p, poses, walls, ctx=ctx)
        _same(got, _ref_paths(p, poses, walls))
        for b in range(B):
            want = oracle.ha_block_free(hp, poses[b], PARKING)
            assert bool(got["scene_free"][b]) == want
            seen.add(want)
        assert C.block_collision_check(h.s.vehicle_size, poses[1].T, PARKING, ctx=ctx) == bool(got["scene_free"][1])
    assert seen == {True, False}


# 8 ------------------------------------------------------------------------------------------------
def test_ragged_paths_at_stride_1(ctx):
    """Ragged pose_count and wall_count at stride 1.  The padding walls cover the whole field and the padding
    poses sit inside a wall, so a read of either shows; every output is checked, under all three modes."""
    r = np.random.default_rng(12)
    B, n, nw = 5, 40, 6
    pose_count = np.array([40, 0, 1, 17, 33], np.int32)
    wall_count = np.array([6, 3, 0, 2, 5], np.int32)
    poses = np.zeros((B, n, 3))
    walls = np.zeros((B, nw, 5))
    for b in range(B):
        poses[b] = np.c_[r.uniform(-3, 9, n), r.uniform(3.5, 9, n), r.uniform(-4, 4, n)]
        poses[b, pose_count[b]:] = [0.0, -1.0, 0.3]                    # inside the lower parking wall
        walls[b, :3] = PARKING
        walls[b, 3:] = np.c_[r.uniform(-3, 9, 3), r.uniform(4, 9, 3), r.uniform(-3, 3, 3), r.uniform(0.3, 1, (3, 2))]
        walls[b, wall_count[b]:] = [0.0, 0.0, 0.2, 100.0, 100.0]       # covers everything
    for mode in MODES:
        p = C.collide_params(VEH, stride=1, mode=mode)
        got = C.path_collision(p, poses, walls, pose_count, wall_count, ctx=ctx)
        want = _ref_paths(p, poses, walls, pose_count, wall_count)
        _same(got, want)
    assert want["scene_free"][1] == 1 and want["scene_free"][2] == 1      # no poses; no walls
    assert (want["pose_free"][1] == 2).all() and want["pose_free"][2, 0] == 1
    assert 0 < want["n_hit"][0] < 40
    quiet = C.path_collision(p, poses, walls, pose_count, wall_count, want_pose_free=False, ctx=ctx)
    assert quiet["pose_free"] is None and np.array_equal(quiet["n_hit"], want["n_hit"])
    nowalls = C.path_collision(p, poses, np.zeros((B, 0, 5)), pose_count, ctx=ctx)
    assert nowalls["scene_free"].all() and (nowalls["first_pose"] == -1).all() and not nowalls["n_hit"].any()


# 9 ------------------------------------------------------------------------------------------------
def test_wall_tile_edges(ctx):
    """tile - 1, tile, tile + 1 and 3 tile + 5 walls with the only colliding wall last (one scene each, ragged)."""
    counts = np.array([WALL_TILE - 1, WALL_TILE, WALL_TILE + 1, 3 * WALL_TILE + 5], np.int32)
    B, nw, n = len(counts), int(counts.max()), 3
    poses = np.tile(np.array([[0.0, 0.0, 0.4], [1.0, 0.5, -0.2], [30.0, 30.0, 1.0]]), (B, 1, 1))
    walls = np.zeros((B, nw, 5))
    for b, c in enumerate(counts):
        k = np.arange(nw)
        walls[b] = np.c_[20.0 + 3 * k, -15.0 - k, 0.1 * k, np.full(nw, 1.0), np.full(nw, 0.5)]   # far from every pose
        walls[b, c - 1] = [1.5, 0.5, 0.3, 1.0, 1.0]                                            # hits poses 0 and 1
        walls[b, c:] = [0.0, 0.0, 0.0, 100.0, 100.0]                                           # padding: hits all
    p = C.collide_params(VEH, stride=1)
    got = C.path_collision(p, poses, walls, wall_count=counts, ctx=ctx)
    _same(got, _ref_paths(p, poses, walls, wall_count=counts))
    assert np.array_equal(got["first_wall"], counts - 1) and (got["first_pose"] == 0).all()
    assert (got["n_hit"] == 2).all() and np.array_equal(got["pose_free"][0], [0, 0, 1])


# 10 -----------------------------------------------------------------------------------------------
def test_pose_chunk_edges(ctx):
    """chunk - 1, chunk, chunk + 1 and 4 chunk + 1 poses with the only hit last; then two hits in different
    chunks: first_pose is the lower, n_hit counts both."""
    counts = np.array([POSE_CHUNK - 1, POSE_CHUNK, POSE_CHUNK + 1, 4 * POSE_CHUNK + 1, 4 * POSE_CHUNK + 1], np.int32)
    B, n = len(counts), int(counts.max())
    k = np.arange(n)
    poses = np.tile(np.c_[7.0 + 0.001 * k, 6.0 + 0.001 * k, 0.01 * k], (B, 1, 1))   # the aisle: free
    inside = [0.0, -1.0, 0.3]                                                       # inside the lower wall
    for b, c in enumerate(counts[:4]):
        poses[b, c - 1] = inside
        poses[b, c:] = inside   # padding
    poses[4, 3 * POSE_CHUNK + 7] = inside
    poses[4, POSE_CHUNK + 3] = [-2.75, 1.0, 0.0]                                    # on the left wall: walls 1 and 0
    walls = np.tile(PARKING, (B, 1, 1))
    p = C.collide_params(VEH, stride=1)
    got = C.path_collision(p, poses, walls, pose_count=counts, ctx=ctx)
    for b in range(B):
        # the restatement on the poses that can differ from the aisle's, the aisle itself once
        idx = sorted({0, int(counts[b]) - 1, POSE_CHUNK + 3, 3 * POSE_CHUNK + 7} & set(range(int(counts[b]))))
        sub = R.path_check(p.half_len, p.half_wid, poses[b, idx], PARKING, 1, p.center_shift)
        want_hit = [i for i, f in zip(idx, sub["pose_free"]) if f == 0]
        assert got["n_hit"][b] == len(want_hit) and got["first_pose"][b] == want_hit[0]
        assert np.array_equal(np.nonzero(got["pose_free"][b] == 0)[0], want_hit)
        assert (got["pose_free"][b, counts[b]:] == 2).all() and got["scene_free"][b] == 0
        j = idx.index(want_hit[0])
        one = R.path_check(p.half_len, p.half_wid, poses[b, idx[j]:idx[j] + 1], PARKING, 1, p.center_shift)
        assert got["first_wall"][b] == one["first_wall"]
    assert np.array_equal(got["first_pose"][:4], counts[:4] - 1)
    assert got["first_pose"][4] == POSE_CHUNK + 3 and got["n_hit"][4] == 2
    aisle = R.path_check(p.half_len, p.half_wid, poses[0, :POSE_CHUNK - 2:17], PARKING, 1, p.center_shift)
    assert aisle["scene_free"]


# 11 -----------------------------------------------------------------------------------------------
def test_angles_and_center_shift(ctx):
    """ψ = 3π, -π and π (modπ's branches; cos and sin of the reduced angle turn the rectangle) and
    center_shift = 0 (the pose is the rectangle's centre)."""
    psis = [3 * np.pi, -np.pi, np.pi, 3 * np.pi + 0.3, -3 * np.pi, 0.0]
    poses = np.array([[[x, y, q] for q in psis for (x, y) in ((0.9, 2.0), (4.4, 1.9), (-4.4, 1.9), (7.0, 5.0))]])
    walls = PARKING[None]
    for shift in (None, 0.0, -0.75):
        p = C.collide_params(VEH, stride=1, center_shift=shift)
        got = C.path_collision(p, poses, walls, ctx=ctx)
        want = _ref_paths(p, poses, walls)
        _same(got, want)
        assert 0 < want["n_hit"][0] < poses.shape[1]
    free0 = C.path_collision(C.collide_params(VEH, 1, 0.0), poses, walls, ctx=ctx)["pose_free"]
    free1 = C.path_collision(C.collide_params(VEH, 1), poses, walls, ctx=ctx)["pose_free"]
    assert not np.array_equal(free0, free1)
    r = C.check_path(VEH, poses[0].T, PARKING, stride=1, center_shift=0.0, ctx=ctx)
    assert np.array_equal(r.pose_free, free0[0]) and r.n_hit == int((free0 == 0).sum()) and r.free is False


# 12 -----------------------------------------------------------------------------------------------
def _path_call(ctx, p, B, n_poses, poses, pc, n_walls, wc, walls, outs):
    return ctx.lib.mp_path_collision(ctx.handle, ctypes.byref(p) if p is not None else None, B, n_poses, ptr(poses),
                                     ptr(pc), n_walls, ptr(wc), ptr(walls), *[ptr(o) for o in outs])


def test_errors_leave_the_outputs_untouched(ctx):
    """Every MP_ERR_INVALID case, the outputs as they were; zero-sized calls return MP_OK."""
    lib = ctx.lib
    # mp_block_pts
    pts = np.full((2, 5, 2), 7.0)
    bad = np.array([[0, 0, 0, 1, 1], [0, np.inf, 0, 1, 1]], float)
    assert lib.mp_block_pts(ctx.handle, 2, ptr(bad), ptr(pts)) == MP_ERR_INVALID
    assert lib.mp_block_pts(ctx.handle, -1, ptr(bad), ptr(pts)) == MP_ERR_INVALID
    assert lib.mp_block_pts(ctx.handle, 0, None, None) == 0
    assert (pts == 7.0).all()

    # mp_convex_collision
    pa = np.full((1, 2, 5, 2), np.nan)
    pa[0, :, :4] = [[0, 0], [1, 0], [1, 1], [0, 0]]
    pb = pa.copy()
    cols = np.array([[4, 4]], np.int32)
    fr = np.full((1, 2, 2), 9, np.uint8)

    def convex(mode=0, B=1, na=2, ma=5, a=pa, ac=cols, nb=2, mb=5, b=pb, bc=cols):
        return lib.mp_convex_collision(ctx.handle, mode, B, na, ma, ptr(a), ptr(ac), nb, mb, ptr(b), ptr(bc), ptr(fr))

    assert convex() == 0 and (fr != 9).all()
    fr[:] = 9
    assert convex(ac=None) == MP_ERR_INVALID                                  # the NaN padding row becomes a read row
    nanrow = pa.copy()
    nanrow[0, 1, 2, 1] = np.nan
    assert convex(a=nanrow) == MP_ERR_INVALID
    infrow = pb.copy()
    infrow[0, 0, 0, 0] = -np.inf
    assert convex(b=infrow) == MP_ERR_INVALID
    for c in ([[1, 4]], [[4, 6]], [[4, 0]], [[-2, 4]]):
        assert convex(ac=np.array(c, np.int32)) == MP_ERR_INVALID
        assert convex(bc=np.array(c, np.int32)) == MP_ERR_INVALID
    wide = np.zeros((1, 1, 40, 2))
    wide[0, 0, :, 0] = np.arange(40)
    assert convex(na=1, ma=40, a=wide, ac=None) == MP_ERR_INVALID             # 40 columns > MP_COLLIDE_MAX_COLS
    assert convex(na=1, ma=40, a=wide, ac=np.array([[33]], np.int32)) == MP_ERR_INVALID
    for mode in (3, -1):
        assert convex(mode=mode) == MP_ERR_INVALID
    for kw in (dict(B=-1), dict(na=-1), dict(nb=-2), dict(ma=-1), dict(mb=-5)):
        assert convex(**kw) == MP_ERR_INVALID
    assert (fr == 9).all()
    for kw in (dict(B=0), dict(na=0), dict(nb=0)):
        assert convex(**kw) == 0
    assert (fr == 9).all()

    # mp_path_collision
    poses = np.tile(np.array([[7.0, 5.0, 0.1]]), (2, 12, 1))
    walls = np.tile(PARKING, (2, 1, 1))
    outs = [np.full(2, 9, np.uint8), np.full(2, 9, np.int32), np.full(2, 9, np.int32), np.full(2, 9, np.int32),
            np.full((2, 12), 9, np.uint8)]

    def path(p=None, B=2, n=12, po=poses, pc=None, nw=3, wc=None, wl=walls, **kw):
        q = C.collide_params(VEH, **kw) if p is None else p
        return _path_call(ctx, q, B, n, po, pc, nw, wc, wl, outs)

    assert path(stride=0) == MP_ERR_INVALID and path(stride=-3) == MP_ERR_INVALID
    assert path(mode=3) == MP_ERR_INVALID and path(mode=-1) == MP_ERR_INVALID
    assert path(B=-1) == MP_ERR_INVALID and path(n=-1) == MP_ERR_INVALID and path(nw=-1) == MP_ERR_INVALID
    q = C.collide_params(VEH)
    q.half_wid = math.nan
    assert path(p=q) == MP_ERR_INVALID
    q = C.collide_params(VEH, center_shift=math.inf)
    assert path(p=q) == MP_ERR_INVALID
    bad = poses.copy()
    bad[1, 10, 2] = np.nan                                                    # checked at stride 5 (0, 5, 10)
    assert path(po=bad) == MP_ERR_INVALID
    assert path(po=bad, pc=np.array([12, 11], np.int32)) == MP_ERR_INVALID    # 11 > 5: 0, 5, 10 still checked
    bw = walls.copy()
    bw[0, 2, 3] = np.inf
    assert path(wl=bw) == MP_ERR_INVALID
    assert path(pc=np.array([12, 13], np.int32)) == MP_ERR_INVALID
    assert path(pc=np.array([-1, 3], np.int32)) == MP_ERR_INVALID
    assert path(wc=np.array([4, 3], np.int32)) == MP_ERR_INVALID
    assert path(wc=np.array([0, -1], np.int32)) == MP_ERR_INVALID
    assert all((o == 9).all() for o in outs)
    assert path(B=0) == 0 and all((o == 9).all() for o in outs)
    # values that are not read may be anything: pose 11 is not checked at stride 5, pose 10 not below a count of 10,
    # wall 2 not below a count of 2
    ok = poses.copy()
    ok[0, 11] = np.nan
    ok[1, 10] = np.inf
    assert path(po=ok, pc=np.array([12, 10], np.int32), wl=bw, wc=np.array([2, 3], np.int32)) == 0
    assert outs[0].tolist() == [1, 1] and outs[1].tolist() == [-1, -1] and outs[3].tolist() == [0, 0]
    assert outs[4][0].tolist() == [1, 2, 2, 2, 2, 1, 2, 2, 2, 2, 1, 2]
    assert outs[4][1].tolist() == [1, 2, 2, 2, 2, 1, 2, 2, 2, 2, 2, 2]
    with pytest.raises(Exception, match="stride"):
        C.check_path(VEH, poses[0].T, PARKING, stride=0, ctx=ctx)


# 13 -----------------------------------------------------------------------------------------------
def test_pipeline_checks_the_planners_own_outputs(ctx):
    """Plan the perpendicular driver scene, retrievePath, track it with his_stride = 1, then check_path on
    actualpath (whose cubic_fit pieces the reference never collision-checks) and on states_his, against the
    restatement."""
    h = ha.driver_searcher(ha.PERPENDICULAR)
    ha.plan_batch([h], ctx=ctx)
    assert h.r.found
    ha.retrieve_batch([h], ctx=ctx)
    tracker.track_batch([h], ctx=ctx, his_stride=1, his_cap=60000)
    walls = np.array(h.s.obstacle_list)
    vs = h.s.vehicle_size
    ap = h.r.actualpath
    his = h.r.tracking["states_his"]
    assert ap.shape[0] == 3 and his.shape[0] == 3 and his.shape[1] == h.r.tracking["n_steps"] > 1000
    for states, stride in ((ap, 1), (ap, 5), (his, 50)):
        got = C.check_path(vs, states, walls, stride=stride, ctx=ctx)
        want = R.path_check(vs[0] / 2, vs[1] / 2, states.T, walls, stride)
        assert got.free == want["scene_free"] and got.first_pose == want["first_pose"]
        assert got.first_wall == want["first_wall"] and got.n_hit == want["n_hit"]
        assert np.array_equal(got.pose_free, want["pose_free"])
    dense = C.check_path(vs, his, walls, stride=1, ctx=ctx)   # every tracked state; the strided answer is its subset
    assert np.array_equal(dense.pose_free[::50], got.pose_free[::50]) and (dense.pose_free != 2).all()
    assert C.block_collision_check(vs, h.r.RSpath_final, walls, ctx=ctx) is True   # the planner accepted it
