"""GPU parity of the occupancy-map tools (motionplanning_amd/csrc/gridmap.hip: mp_grid_distance, mp_grid_inflate,
mp_grid_path_clearance; astar.hip: mp_grid_rasterize; motionplanning_amd/gridmap.py) against the CPU restatements
tests/gridmap_ref.py and tests/astar_ref.py on the case set tests/gridmap_cases.py.  Everything is an integer: all
parity is byte equality."""
import functools

import numpy as np
import pytest

import astar_ref as A
import gridmap_cases as C
import gridmap_ref as R
import test_gpu_astar as TA
import test_gpu_grid_large as TL
import test_gpu_gridsearch as TG
from motionplanning_amd import astar, gridmap
from motionplanning_amd.abi import ptr

pytestmark = pytest.mark.gpu

BORDER, OCCUPIED, NONE = R.BORDER, R.OUT_OCCUPIED, R.D2_NONE
INVALID, NOMEM = 1, 3
MAX_CELLS, MAX_BATCH_CELLS = 1 << 22, 1 << 28  # MP_GRID_MAX_CELLS, MP_MAP_MAX_BATCH_CELLS
BATCHES = C.by_shape()


def distance(ctx, masks, flags=0):
    masks = np.ascontiguousarray(masks, np.uint8)
    B, ny, nx = masks.shape
    d2 = np.full(masks.shape, -7, np.int32)
    ctx.check(ctx.lib.mp_grid_distance(ctx.handle, flags, B, nx, ny, ptr(masks), ptr(d2)))
    return d2


def inflate(ctx, masks, r2, flags=0):
    masks, r2 = np.ascontiguousarray(masks, np.uint8), np.ascontiguousarray(r2, np.int32)
    B, ny, nx = masks.shape
    assert r2.shape == (B,)
    out = np.full(masks.shape, 9, np.uint8)
    ctx.check(ctx.lib.mp_grid_inflate(ctx.handle, flags, B, nx, ny, ptr(masks), ptr(r2), ptr(out)))
    return out


def clearance(ctx, masks, paths, path_n, flags=0):
    masks = np.ascontiguousarray(masks, np.uint8)
    paths, path_n = np.ascontiguousarray(paths, np.int32), np.ascontiguousarray(path_n, np.int32)
    B, ny, nx = masks.shape
    assert paths.shape[0] == B and path_n.shape == (B,)
    md, at = np.full(B, -7, np.int32), np.full(B, -7, np.int32)
    ctx.check(ctx.lib.mp_grid_path_clearance(ctx.handle, flags, B, nx, ny, ptr(masks), ptr(paths), ptr(path_n),
                                             paths.shape[1], ptr(md), ptr(at)))
    return md, at


def rasterize(ctx, nx, ny, bounds, kind, obstacles):
    """mp_grid_rasterize; lists of unlike length are padded with [0, 0, 0] circles (never hit), as TL.grid_plan pads."""
    bounds = np.ascontiguousarray(bounds, np.float64)
    B, n_obs = len(bounds), max(len(o) for o in obstacles)
    obs = np.zeros((B, n_obs, kind))
    for b, o in enumerate(obstacles):
        if len(o):
            obs[b, : len(o)] = o
    mask = np.full((B, ny, nx), 9, np.uint8)
    ctx.check(ctx.lib.mp_grid_rasterize(ctx.handle, B, nx, ny, ptr(bounds), kind, n_obs, ptr(obs) if n_obs else None,
                                        ptr(mask)))
    return mask


@functools.lru_cache(maxsize=None)
def ref_d2(shape, border):
    """[B, ny, nx]: the separable restatement of every map of the shape's batch, computed once."""
    d = np.stack([R.d2_separable(m, border) for m in BATCHES[shape][1]])
    d.setflags(write=False)
    return d


# ---- 1. mp_grid_distance on the whole case set, one call per shape
@pytest.mark.parametrize("border", [False, True])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_distance_case_set(ctx, shape, border):
    names, masks = BATCHES[shape]
    flags = BORDER if border else 0
    d2, ref = distance(ctx, masks, flags), ref_d2(shape, border)
    for b, name in enumerate(names):
        assert np.array_equal(d2[b], ref[b]), (name, np.argwhere(d2[b] != ref[b])[:5])
    # a map's bytes do not depend on its position in the batch
    assert np.array_equal(distance(ctx, masks[::-1], flags)[::-1], d2)
    assert np.array_equal(distance(ctx, masks[3:4], flags)[0], d2[3])


# ---- 2. mp_grid_inflate: every r2 on every map in one call (so the r2 differ from map to map), both polarities
@pytest.mark.parametrize("occupied", [False, True])
@pytest.mark.parametrize("border", [False, True])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_inflate_case_set(ctx, shape, border, occupied):
    names, masks = BATCHES[shape]
    B, R2 = len(names), C.INFLATE_R2
    flags = (BORDER if border else 0) | (OCCUPIED if occupied else 0)
    # map b with r2 j at b*len(R2) + j: neighbouring maps of the batch never share an r2
    big = np.repeat(masks, len(R2), axis=0)
    r2 = np.tile(np.array(R2, np.int32), B)
    out = inflate(ctx, big, r2, flags)
    assert set(np.unique(out).tolist()) <= {0, 1}
    own = distance(ctx, masks, BORDER if border else 0)  # the capped instance against the full one
    ref = ref_d2(shape, border)
    for b, name in enumerate(names):
        for j, r in enumerate(R2):
            got = out[b * len(R2) + j]
            assert np.array_equal(got, R.inflate(masks[b], r, occupied=occupied, d2=ref[b])), (name, r)
            free = (masks[b] != 0) & (own[b] > r)
            assert np.array_equal(got, (~free if occupied else free).astype(np.uint8)), (name, r)
            if r == 0:  # the input normalised to 0 / 1
                assert np.array_equal(got, ((masks[b] == 0) if occupied else (masks[b] != 0)).astype(np.uint8)), name
    # one r2 for the whole batch is the same bytes
    assert np.array_equal(inflate(ctx, masks, np.full(B, 4, np.int32), flags), out[R2.index(4)::len(R2)])


# ---- 3. mp_grid_rasterize is the planners' own mask
def _rows(name):
    if name in TA.GROUPS:
        nx, ny, kind, rows = TA.GROUPS[name]
    else:
        (nx, ny, rows), kind = TG.GROUPS[name], 3
    return nx, ny, kind, rows


@functools.lru_cache(maxsize=None)
def ref_masks(name):
    nx, ny, kind, rows = _rows(name)
    return np.stack([A.free_mask(A.Grid(r[0], nx, ny), r[3], kind) for r in rows])


@pytest.mark.parametrize("name", list(TA.GROUPS) + list(TG.GROUPS))
def test_rasterize_is_the_planners_mask(ctx, name):
    nx, ny, kind, rows = _rows(name)
    masks = rasterize(ctx, nx, ny, [r[0] for r in rows], kind, [r[3] for r in rows])
    ref = ref_masks(name)
    for b in range(len(rows)):
        assert np.array_equal(masks[b], ref[b]), (name, b)
    if name == "unit3":
        assert (masks == 1).all()  # empty lists: all free
    # mp_grid_plan over the rasterised mask returns the bytes it returns over the list, in every output
    args = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    for planner in (["astar"] if kind == 5 else TL.PLANNERS):
        listed = TL.grid_plan(ctx, planner, nx, ny, *args, kind, [r[3] for r in rows])
        assert TL.same_bytes(listed, TL.grid_plan(ctx, planner, nx, ny, *args, TL.MASK, masks)), (name, planner)


# ---- 4. full size: 2048 x 2048 with one blocked cell at (2048, 1), against the analytic field
@pytest.mark.parametrize("border", [False, True])
def test_2048x2048_point(ctx, border):
    n, flags = 2048, BORDER if border else 0
    assert n * n == MAX_CELLS
    mask = np.ones((1, n, n), np.uint8)
    mask[0, 0, n - 1] = 0
    field = R.point_field(n, n, n - 1, 0, border)
    assert np.array_equal(distance(ctx, mask, flags)[0], field)
    r2 = 10 ** 6
    assert (field == r2).any() and (field > r2).any() and (field < r2).any()
    assert np.array_equal(inflate(ctx, mask, [r2], flags)[0], (field > r2).astype(np.uint8))
    assert np.array_equal(inflate(ctx, mask, [r2], flags | OCCUPIED)[0], (field <= r2).astype(np.uint8))


# ---- 5. mp_grid_path_clearance
B65 = [0.0, 64.0, 0.0, 66.0]  # 65 x 67 cells of 1 x 1
PLANNED = ["tie_65x67", "sparse_65x67", "diagonal_65x67", "dense_65x67"]


@functools.lru_cache(maxsize=None)
def planned_refs():
    g = A.Grid(B65, 65, 67)
    return [A.search(g, (1, 1), (65, 67), C.get(n)) for n in PLANNED[:3]] + [A.search(g, (2, 1), (9, 9), C.get(PLANNED[3]))]


@pytest.mark.parametrize("border", [False, True])
def test_clearance_of_planned_paths(ctx, border):
    g = A.Grid(B65, 65, 67)
    masks = np.stack([C.get(n) for n in PLANNED])
    starts = [TL.real_of(g, (1, 1))] * 3 + [TL.real_of(g, (2, 1))]
    goals = [TL.real_of(g, (65, 67))] * 3 + [TL.real_of(g, (9, 9))]
    out = TL.grid_plan(ctx, "astar", 65, 67, [B65] * 4, starts, goals, TL.MASK, masks)
    refs = planned_refs()
    assert all(r["found"] for r in refs[:3])
    for b, ref in enumerate(refs):  # the paths are the restatement's: the clearance below is of known paths
        assert list(out["path"][b, : out["pn"][b]]) == [g.encode(c) for c in ref["path"]]
    md, at = clearance(ctx, masks, out["path"], out["pn"], BORDER if border else 0)
    for b, name in enumerate(PLANNED):
        d2 = R.d2_separable(masks[b], border)
        assert (int(md[b]), int(at[b])) == R.clearance(d2, out["path"][b], out["pn"][b]), name
    assert md[0] > 0 and out["pn"][3] > 0
    # the Python wrapper, a batch and a single map
    pm, pa = gridmap.path_clearance(masks, out["path"], out["pn"], border=border, ctx=ctx)
    assert np.array_equal(pm, md) and np.array_equal(pa, at)
    assert gridmap.path_clearance(masks[1], out["path"][1], out["pn"][1:2], border=border, ctx=ctx) == (md[1], at[1])


def test_clearance_of_hand_made_paths(ctx):
    tie, free = C.get("tie_65x67"), C.get("all_free_65x67")
    d2 = R.d2_separable(tie)
    enc = lambda x, y: y * 65 + x + 1
    T = [enc(15, 30), enc(14, 10), 0, enc(16, 10), enc(15, 11)]  # (14, 10) and (16, 10) tie at 16: index 1 wins
    long_tie = [enc(60, 60)] * 130 + [enc(11, 10)] + [enc(60, 60)] * 60 + [enc(9, 10), enc(21, 10)]  # 1 at 130, 191, 192
    stride = len(long_tie)
    rows = [(tie, T, 5), (tie, T, 1), (tie, T, 0), (tie, [0, 0, 0], 3), (tie, [0] + T, 6), (tie, T[::-1], 5),
            (tie, long_tie, stride), (tie, long_tie[::-1], stride), (tie, [enc(10, 10), 65 * 67], 2), (free, [5, 6], 2),
            (tie, [enc(14, 10), 65 * 67 + 1, -3], 1)]  # entries past path_n are not read
    paths = np.zeros((len(rows), stride), np.int32)
    for b, (_, p, _) in enumerate(rows):
        paths[b, : len(p)] = p
        paths[b, len(p):] = -1  # mp_grid_plan's padding
    md, at = clearance(ctx, np.stack([r[0] for r in rows]), paths, [r[2] for r in rows])
    got = list(zip(md.tolist(), at.tolist()))
    assert got == [R.clearance(R.d2_separable(m), paths[b], n) for b, (m, _, n) in enumerate(rows)]
    assert got[0] == (16, 1) and got[2] == (NONE, -1) and got[3] == (NONE, -1) and got[4] == (16, 2)
    assert got[5] == (16, 1) and got[6] == (1, 130) and got[7] == (1, 0) and got[8] == (0, 0) and got[9] == (NONE, 0)
    assert got[1] == (int(d2[30, 15]), 0)


# ---- 6. end to end: planning on the inflated map keeps the robot's radius clear of the original one
B_E2E, NX_E2E, NY_E2E, R2_E2E = [0.0, 30.0, 0.0, 20.0], 31, 21, 4
START_E2E, GOAL_E2E = (1, 11), (31, 11)


def mask_e2e():
    m = np.ones((NY_E2E, NX_E2E), np.uint8)
    m[9:12, 15] = 0  # a short wall across the straight line from start to goal
    return m


@functools.lru_cache(maxsize=None)
def refs_e2e():
    """Chosen on the CPU: the plain search grazes the wall, the search on the inflated map does not."""
    g, m = A.Grid(B_E2E, NX_E2E, NY_E2E), mask_e2e()
    d2 = R.d2_separable(m)
    plain, safe = A.search(g, START_E2E, GOAL_E2E, m), A.search(g, START_E2E, GOAL_E2E, R.inflate(m, R2_E2E, d2=d2))
    enc = lambda r: [g.encode(c) for c in r["path"]]
    return plain, safe, R.clearance(d2, enc(plain), len(plain["path"])), R.clearance(d2, enc(safe), len(safe["path"]))


def test_astar_on_the_inflated_map_keeps_clear(ctx):
    plain, safe, c_plain, c_safe = refs_e2e()
    assert plain["found"] and safe["found"] and 0 < c_plain[0] <= R2_E2E < c_safe[0]
    g, m = A.Grid(B_E2E, NX_E2E, NY_E2E), mask_e2e()
    start, goal = TL.real_of(g, START_E2E), TL.real_of(g, GOAL_E2E)
    got = []
    for mask in (m, gridmap.inflate(m, r2=R2_E2E, ctx=ctx)):
        a = astar.defineAstar(B_E2E, [NX_E2E, NY_E2E], start, goal)
        astar.defineAstarmask_(a, mask)
        astar.planAstar_(a, ctx=ctx)
        assert a.r.found
        enc = np.array([[g.encode(tuple(c)) for c in a.r.astarpath]], np.int32)
        got.append(gridmap.path_clearance(m, enc, [enc.shape[1]], ctx=ctx))  # on the ORIGINAL mask
    assert got == [c_plain, c_safe] and got[0][0] <= R2_E2E < got[1][0]
    # the same through inflate_searcher_, from an obstacle list: a circle on each of the wall's cells
    b = astar.defineAstar(B_E2E, [NX_E2E, NY_E2E], start, goal)
    astar.defineAstarobs_(b, [[15.0, 9.0, 0.5], [15.0, 10.0, 0.5], [15.0, 11.0, 0.5]])
    assert np.array_equal(gridmap.rasterize([b], ctx=ctx)[0], m)
    gridmap.inflate_searcher_(b, 2.0, ctx=ctx)  # 2 m of 1 m cells: r2 = 4
    assert b.s.obstacle_list == [] and np.array_equal(b.s.free_mask, R.inflate(m, R2_E2E))
    astar.planAstar_(b, ctx=ctx)
    assert [tuple(c) for c in b.r.astarpath] == safe["path"]
    # and as MPPI's grid: the occupied polarity of the same bytes
    grid, spec = gridmap.mppi_grid(b, b.s.free_mask)
    assert np.array_equal(grid, gridmap.inflate(m, radius=2.0, occupied=True, ctx=ctx)) and spec["dx"] == 1.0
    assert np.array_equal(gridmap.distance2(m, ctx=ctx), R.d2_separable(m))
    assert np.array_equal(gridmap.distance2(m[None], border=True, ctx=ctx)[0], R.d2_separable(m, True))


# ---- 7. refusals: the status, and the outputs keep their canary bytes
def test_refusals_leave_the_outputs_alone(ctx):
    lib, h = ctx.lib, ctx.handle
    m = np.ones((1, 4, 4), np.uint8)
    d2, out = np.full((1, 4, 4), 0x5A5A5A5A, np.int32), np.full((1, 4, 4), 0xA5, np.uint8)
    md, at = np.full(1, 0x5A5A5A5A, np.int32), np.full(1, 0x5A5A5A5A, np.int32)
    r2, neg, four = np.array([1], np.int32), np.array([-1], np.int32), np.array([4], np.int32)
    path, pn = np.array([[1, 16, 17]], np.int32), np.array([3], np.int32)
    bound, circle = np.array([[0.0, 3.0, 0.0, 3.0]]), np.array([[[1.0, 1.0, 0.6]]])
    dist = lambda flags=0, B=1, nx=4, ny=4, mk=ptr(m), o=ptr(d2): lib.mp_grid_distance(h, flags, B, nx, ny, mk, o)
    infl = lambda flags=0, B=1, nx=4, ny=4, mk=ptr(m), r=ptr(r2), o=ptr(out): lib.mp_grid_inflate(h, flags, B, nx, ny, mk, r, o)
    clr = lambda flags=0, nx=4, ny=4, mk=ptr(m), p=ptr(path), n=ptr(pn), s=3, a=ptr(md), b=ptr(at): \
        lib.mp_grid_path_clearance(h, flags, 1, nx, ny, mk, p, n, s, a, b)
    rast = lambda B=1, nx=4, ny=4, bd=ptr(bound), kind=3, n=1, ob=ptr(circle), o=ptr(out): \
        lib.mp_grid_rasterize(h, B, nx, ny, bd, kind, n, ob, o)
    refused = [
        dist(nx=1), infl(nx=1), clr(nx=1), rast(nx=1), dist(ny=1),                      # a side below 2
        dist(nx=2049, ny=2048), infl(nx=2049, ny=2048), clr(nx=2049, ny=2048), rast(nx=2049, ny=2048),  # nx*ny
        dist(B=MAX_BATCH_CELLS // 16 + 1), infl(B=MAX_BATCH_CELLS // 16 + 1), rast(B=MAX_BATCH_CELLS // 16 + 1),
        dist(B=0), infl(B=0), rast(B=0),
        dist(nx=65536, ny=2), infl(nx=2, ny=32769),                                     # MP_MAP_MAX_SIDE
        dist(mk=None), dist(o=None), infl(mk=None), infl(r=None), infl(o=None),         # NULL pointers
        clr(mk=None), clr(p=None), clr(n=None), clr(a=None), clr(b=None), rast(bd=None), rast(ob=None), rast(o=None),
        infl(r=ptr(neg)),                                                                # r2 = -1
        dist(flags=2), dist(flags=4), infl(flags=4), infl(flags=-1), clr(flags=2),      # unknown flag bits
        clr(),                                                                           # a path entry of N + 1
        clr(n=ptr(four)), clr(n=ptr(neg)), clr(s=0),                  # path_n outside 0 .. stride
        rast(kind=4), rast(kind=1), rast(n=-1),
    ]
    assert refused == [INVALID] * len(refused)
    assert clr() == INVALID and b"outside" in lib.mp_last_error(h)
    # a workspace that cannot be had, on a context of its own (the cap applies when a workspace grows)
    from motionplanning_amd.context import Context

    c = Context(0)
    try:
        c.set_workspace_limit(1 << 20)
        n = 1024
        bm = np.ones((1, n, n), np.uint8)
        bd2, bout = np.full((1, n, n), 0x5A5A5A5A, np.int32), np.full((1, n, 2 * n), 0xA5, np.uint8)
        bpath = np.array([[1, 2]], np.int32)
        two = np.array([2], np.int32)
        assert c.lib.mp_grid_distance(c.handle, 0, 1, n, n, ptr(bm), ptr(bd2)) == NOMEM
        assert c.lib.mp_grid_inflate(c.handle, 0, 1, n, n, ptr(bm), ptr(r2), ptr(bout)) == NOMEM
        assert c.lib.mp_grid_path_clearance(c.handle, 0, 1, n, n, ptr(bm), ptr(bpath), ptr(two), 2, ptr(md), ptr(at)) == NOMEM
        big_bound = np.array([[0.0, n - 1.0, 0.0, n - 1.0]])
        assert c.lib.mp_grid_rasterize(c.handle, 1, 2 * n, n, ptr(big_bound), 3, 1, ptr(circle), ptr(bout)) == NOMEM
        assert (bd2 == 0x5A5A5A5A).all() and (bout == 0xA5).all()
        c.set_workspace_limit(0)
        assert c.lib.mp_grid_distance(c.handle, 0, 1, n, n, ptr(bm), ptr(bd2)) == 0 and (bd2 == NONE).all()
    finally:
        c.close()
    assert (d2 == 0x5A5A5A5A).all() and (out == 0xA5).all() and md[0] == 0x5A5A5A5A and at[0] == 0x5A5A5A5A
    # the same buffers are written once the call is accepted
    path[0, 2] = 0
    assert dist() == 0 and infl() == 0 and clr() == 0 and rast() == 0
    assert (d2 == NONE).all() and md[0] == NONE and at[0] == 0 and out.sum() == 15
