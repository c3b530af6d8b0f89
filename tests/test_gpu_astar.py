"""GPU parity of the grid A* kernel (motionplanning_amd/csrc/astar.hip: mp_astar_plan, mp_ha_astar_table) and of
Hybrid A* with use_astar (mp_ha_plan_astar) against the CPU restatement tests/astar_ref.py -- BIT-EXACT costs,
pop order, node counts and paths."""
import ctypes
import functools
import os

import numpy as np
import pytest

import astar_ref as R
import oracle
from motionplanning_amd import astar
from motionplanning_amd import hybrid_astar as ha
from motionplanning_amd.abi import ptr

pytestmark = pytest.mark.gpu

PI = np.pi
ROTATED = [[0.0, -1.0, 0.3, 5.5 / 2 + 1.0, 1.0], [-2.0, 4.0, -0.7, 1.5, 0.6], [6.0, 6.0, 1.1, 2.0, 0.8]]


def gpu_plan(ctx, nx, ny, bound, start, goal, kind, obstacles):
    """mp_astar_plan for B searches; obstacles [B][n_obs][kind]."""
    bound, start, goal = (np.ascontiguousarray(a, np.float64) for a in (bound, start, goal))
    B, M = len(bound), nx * ny + 1
    obs = np.ascontiguousarray(obstacles, np.float64)
    n_obs = obs.size // (B * kind)
    obs = obs.reshape(B, n_obs, kind)
    cost, plen = np.zeros(B), np.zeros(B)
    found, pops, nn, pn = (np.zeros(B, np.int32) for _ in range(4))
    seq, path = np.zeros((B, 2 * M), np.int32), np.zeros((B, M), np.int32)
    ctx.check(ctx.lib.mp_astar_plan(ctx.handle, B, nx, ny, ptr(bound), ptr(start), ptr(goal), kind, n_obs,
                                    ptr(obs) if n_obs else None, ptr(cost), ptr(found), ptr(pops), ptr(nn), ptr(seq),
                                    ptr(path), ptr(pn), ptr(plen)))
    return dict(cost=cost, plen=plen, found=found, pops=pops, nn=nn, pn=pn, seq=seq, path=path)


def check_against_ref(out, b, ref, grid):
    assert out["cost"][b].tobytes() == np.float64(ref["final_cost"]).tobytes(), (b, out["cost"][b], ref["final_cost"])
    assert bool(out["found"][b]) == ref["found"] and out["pops"][b] == ref["pops"] and out["nn"][b] == ref["n_nodes"]
    assert list(out["seq"][b, : ref["pops"]]) == ref["pop_seq"] and (out["seq"][b, ref["pops"]:] == -1).all()
    assert list(out["path"][b, : out["pn"][b]]) == [grid.encode(c) for c in ref["path"]]
    assert out["plen"][b].tobytes() == np.float64(ref["path_length"]).tobytes()


# ---- mp_astar_plan: (nx, ny, kind) groups, one call each; rows = (bound, start, goal, obstacles)
HA_BOX = [-5.0, 10.0, 0.0, 10.0]
BLOCKS_11 = [
    (HA_BOX, [7.0, 0.0], [0.0, 0.5], ha.PERPENDICULAR["walls"]),
    (HA_BOX, [7.0, 0.0], [-1.5, 2.0], ha.PARALLEL["walls"]),
    (HA_BOX, [9.9, 9.9], [-4.0, 2.5], ROTATED),                    # rotated blocks
    (HA_BOX, [3.2, 5.1], [3.4, 5.3], ROTATED),                     # start cell == goal cell
    (HA_BOX, [0.0, -0.9], [8.0, 9.0], ha.PERPENDICULAR["walls"]),  # start inside an obstacle (not checked)
    (HA_BOX, [7.0, 3.0], [12.5, 3.0], ha.PARALLEL["walls"]),       # goal outside the bound: never reached
    (HA_BOX, [-7.0, 3.0], [8.0, 3.0], ha.PARALLEL["walls"]),       # start two cells off the grid: one pop
    (HA_BOX, [-5.5, 3.0], [8.0, 3.0], ha.PARALLEL["walls"]),       # start one cell off the grid: steps onto it
]
CIRCLES_75 = [  # 7 x 5: nx != ny
    ([0.0, 6.0, 0.0, 4.0], [0.2, 0.1], [5.9, 3.9], [[3.0, 1.0, 1.2], [3.0, 3.2, 0.9]]),
    ([0.0, 12.0, -2.0, 2.0], [11.0, 1.9], [0.5, -1.5], [[6.0, 0.0, 1.1], [2.0, -2.0, 0.7]]),
    ([0.0, 6.0, 0.0, 4.0], [0.0, 0.0], [6.0, 4.0], [[5.0, 4.0, 0.5], [5.0, 3.0, 0.5]]),
    ([0.0, 6.0, 0.0, 4.0], [0.0, 0.0], [6.0, 4.0], [[5.0, 4.0, 0.5], [6.0, 3.0, 0.5]]),
]
BLOCKS_75 = [
    ([0.0, 6.0, 0.0, 4.0], [0.0, 0.0], [6.0, 4.0], [[3.0, 1.0, 0.4, 1.0, 0.3], [3.0, 3.5, -0.5, 0.8, 0.2]]),
    ([0.0, 6.0, 0.0, 4.0], [6.0, 0.0], [0.0, 4.0], [[3.0, 2.0, PI / 2, 1.2, 0.3], [1.0, 1.0, 0.0, 0.3, 0.3]]),
]
WALLED_75 = [([0.0, 6.0, 0.0, 4.0], [0.0, 0.0], [6.0, 4.0], [[5.0, 4.0, 0.5], [5.0, 3.0, 0.5], [6.0, 3.0, 0.5]])]
GROUPS = {"blocks11": (11, 11, 5, BLOCKS_11), "circles75": (7, 5, 3, CIRCLES_75), "blocks75": (7, 5, 5, BLOCKS_75),
          "walled75": (7, 5, 3, WALLED_75)}


@functools.lru_cache(maxsize=None)
def group_refs(name):
    nx, ny, kind, rows = GROUPS[name]
    return [R.plan(b, nx, ny, s, g, o, kind) for b, s, g, o in rows]


@pytest.mark.parametrize("name", list(GROUPS))
def test_astar_plan_bitexact(ctx, name):
    nx, ny, kind, rows = GROUPS[name]
    out = gpu_plan(ctx, nx, ny, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], kind,
                   [r[3] for r in rows])
    refs = group_refs(name)
    for b, (row, ref) in enumerate(zip(rows, refs)):
        check_against_ref(out, b, ref, R.Grid(row[0], nx, ny))
    if name == "blocks11":
        assert [r["found"] for r in refs] == [True, True, True, True, True, False, False, True]
        assert refs[3]["pops"] == 1 and refs[3]["final_cost"] == 0.0 and refs[6]["pops"] == 1
        assert refs[7]["pop_seq"][0] == 0  # the off-grid start is slot 0
    if name == "walled75":
        assert not refs[0]["found"] and refs[0]["pops"] == 35 - 3 - 1


def test_astar_plan_no_obstacles_and_limits(ctx):
    g = R.Grid([0, 2, 0, 2], 3, 3)
    out = gpu_plan(ctx, 3, 3, [[0, 2, 0, 2]] * 2, [[2.0, 0.0], [0.0, 0.0]], [[0.0, 2.0], [2.0, 2.0]], 3,
                   np.zeros((2, 0, 3)))
    m = np.ones((3, 3), np.uint8)
    check_against_ref(out, 0, R.search(g, (3, 1), (1, 3), m), g)
    check_against_ref(out, 1, R.search(g, (1, 1), (3, 3), m), g)
    assert out["cost"][0] == 4.0 and out["cost"][1] == 2 * np.sqrt(2.0)
    z, zi = np.zeros(1), np.zeros(1, np.int32)
    b, s = np.array([[0.0, 1, 0, 1]]), np.array([[0.0, 0.0]])
    st = ctx.lib.mp_astar_plan(ctx.handle, 1, 52, 51, ptr(b), ptr(s), ptr(s), 3, 0, None, ptr(z), ptr(zi), ptr(zi),
                               ptr(zi), None, None, None, None)
    assert st != 0 and b"51" in ctx.lib.mp_last_error(ctx.handle)


# ---- 51 x 51 circle field (Astar/main.jl's second scenario in shape; seeded circles)
def circle_field():
    r = np.random.default_rng(53)
    obs = np.c_[r.uniform(8, 112, 40), r.uniform(8, 112, 40), r.uniform(3, 9, 40)]
    return [0.0, 120.0, 0.0, 120.0], [0.0, 0.0], [120.0, 120.0], obs


@functools.lru_cache(maxsize=None)
def circle_field_ref():
    b, s, g, obs = circle_field()
    return R.plan(b, 51, 51, s, g, obs, 3)


def test_astar_plan_51x51_circle_field_bitexact(ctx):
    b, s, g, obs = circle_field()
    ref = circle_field_ref()
    assert ref["found"] and ref["pops"] > 200
    out = gpu_plan(ctx, 51, 51, [b], [s], [g], 3, [obs])
    check_against_ref(out, 0, ref, R.Grid(b, 51, 51))


def test_plan_astar_python_api(ctx):
    b, s, g, obs = circle_field()
    ref = circle_field_ref()
    a = astar.defineAstar(b, [51, 51], s, g)
    astar.defineAstarobs_(a, obs)
    astar.planAstar_(a, ctx=ctx)
    assert a.r.found and a.r.final_cost == ref["final_cost"] and a.r.loop_count == ref["pops"]
    assert a.r.path_length == ref["path_length"]
    assert [tuple(c) for c in a.r.astarpath] == ref["path"]
    assert np.array_equal(a.r.actualpath, np.array(ref["actualpath"]))


# ---- mp_ha_astar_table
def _table_scenes():
    out = []
    for scene in (ha.PERPENDICULAR, ha.PARALLEL, dict(ha.PERPENDICULAR, walls=ROTATED, ending_real=[8.0, 2.0, 0.0])):
        st = ha.driver_settings()
        h = ha.defineHybridAstar(st["vehicle_size"], st["gear_set"], st["steer_set"], st["minR"], st["expand_time"],
                                 st["resolutions"], st["stbound"], scene["starting_real"], scene["ending_real"])
        ha.defineHybridAstarobs_(h, scene["walls"])
        out.append(h)
    return out


@functools.lru_cache(maxsize=None)
def table_refs():
    hs = _table_scenes()
    p = ha.params_of(hs[0])
    return [R.ha_table(p, h.s.ending_states, np.array(h.s.obstacle_list))[0] for h in hs]


def gpu_table(ctx, p, goals, walls):
    goals, walls = np.ascontiguousarray(goals, np.float64), np.ascontiguousarray(walls, np.float64)
    tab = np.zeros((len(goals), 121))
    ctx.check(ctx.lib.mp_ha_astar_table(ctx.handle, ctypes.byref(p), len(goals), ptr(goals), ptr(walls), ptr(tab)))
    return tab


def test_ha_astar_table_bitexact(ctx):
    hs = _table_scenes()
    p = ha.params_of(hs[0])
    tab = gpu_table(ctx, p, [h.s.ending_states for h in hs], [h.s.obstacle_list for h in hs])
    refs = table_refs()
    g = R.ha_grid(p)
    for b, h in enumerate(hs):
        assert tab[b].tobytes() == refs[b].tobytes(), b
        # the same 121 numbers from 121 separate planAstar! searches, each started inside its cell
        starts = [[g.b[0] + (ix - 0.5) * g.xf, g.b[2] + (iy - 0.5) * g.yf] for iy in range(1, 12) for ix in range(1, 12)]
        assert [g.encode(g.cell(s)) for s in starts] == list(range(1, 122))
        out = gpu_plan(ctx, 11, 11, [g.b] * 121, starts, [list(h.s.ending_states[:2])] * 121, 5,
                       [h.s.obstacle_list] * 121)
        assert out["cost"].tobytes() == tab[b].tobytes(), b
    assert (refs[2] > 0).sum() > 60 and not np.array_equal(refs[0], refs[2])


# ---- mp_ha_plan_astar
def _plan_scenes(use_astar):
    return [ha.driver_searcher(ha.PERPENDICULAR, use_astar=use_astar), ha.driver_searcher(ha.PARALLEL, use_astar=use_astar)
            ] + ha.scenario_batch(4, seed=4, use_astar=use_astar)


def _tail_step_scenes():
    """15 scenes: with MPGPU_HA_PERSIST=0 one too many for the pipelined tail, so the non-pipelined tail step
    (ha_step_kernel<12, 4, true, true>) runs them until a live-count poll reports 14 or fewer."""
    return ha.scenario_batch(13, seed=4, use_astar=True) + [ha.driver_searcher(ha.PERPENDICULAR, use_astar=True),
                                                            ha.driver_searcher(ha.PARALLEL, use_astar=True)]


@functools.lru_cache(maxsize=None)
def plan_refs(tail_step=False):
    hs = _tail_step_scenes() if tail_step else _plan_scenes(True)
    p = ha.params_of(hs[0])
    sc, pc = oracle.ha_neighbor_origin(hs[0].s.expand_time, hs[0].s.steer_set, hs[0].s.gear_set)
    out = []
    for h in hs:
        walls = np.array(h.s.obstacle_list)
        tab = R.ha_table(p, h.s.ending_states, walls)[0]
        out.append(R.ha_plan(p, h.s.starting_states, h.s.ending_states, walls, sc, pc, tab))
    return out


def _check_plans(hs, refs):
    for i, (h, ref) in enumerate(zip(hs, refs)):
        assert h.r.found == ref["found"] and h.r.loop_count == ref["pops"] and h.r.n_nodes == ref["n_nodes"], i
        assert np.array_equal(h.r.pop_sequence, ref["pop_seq"]), i
        assert np.array_equal(h.r.hybrid_astar_states.T, ref["states"]), i
        assert np.array_equal(h.r.RSpath_final.T, ref["rs_path"]), i


@pytest.mark.parametrize("persist", [True, False])
def test_ha_plan_astar_bitexact(ctx, persist):
    """Both driver scenes and four of the seeded batch with the heuristic on, through every bookkeeping path the
    batch takes; persist=False: the per-iteration pipelined tail (MPGPU_HA_PERSIST=0)."""
    hs = _plan_scenes(True)
    refs = plan_refs()
    assert (refs[0]["pops"], refs[0]["n_nodes"], refs[1]["pops"], refs[1]["n_nodes"]) == (344, 1592, 112, 559)
    if not persist:
        os.environ["MPGPU_HA_PERSIST"] = "0"
    try:
        ha.plan_batch(hs, ctx=ctx)
    finally:
        if not persist:
            del os.environ["MPGPU_HA_PERSIST"]
    _check_plans(hs, refs)


def test_ha_plan_astar_tail_step_bitexact(ctx):
    """The 15-scene batch with the persistent launch off: the tail step's use_astar instance."""
    hs = _tail_step_scenes()
    refs = plan_refs(True)
    os.environ["MPGPU_HA_PERSIST"] = "0"
    try:
        ha.plan_batch(hs, ctx=ctx)
    finally:
        del os.environ["MPGPU_HA_PERSIST"]
    _check_plans(hs, refs)


def test_ha_plan_astar_flag_off_is_ha_plan(ctx):
    """use_astar = 0 through the new entry point: mp_ha_plan's outputs on the same batch."""
    hs = _plan_scenes(False)
    ha.plan_batch(hs, ctx=ctx)
    p = ha.params_of(hs[0])
    B, mp = len(hs), p.max_pops
    start = np.array([h.s.starting_states for h in hs])
    goal = np.array([h.s.ending_states for h in hs])
    walls = np.array([h.s.obstacle_list for h in hs], np.float64)
    found, pops, nn, ns, rl = (np.zeros(B, np.int32) for _ in range(5))
    seq, states, rs = np.zeros((B, mp), np.int64), np.zeros((B, mp, 3)), np.zeros((B, 501, 3))
    ctx.check(ctx.lib.mp_ha_plan_astar(ctx.handle, ctypes.byref(p), B, ptr(start), ptr(goal), ptr(walls), 0, ptr(found),
                                       ptr(pops), ptr(nn), ptr(seq), ptr(ns), ptr(states), ptr(rl), ptr(rs)))
    for b, h in enumerate(hs):
        assert bool(found[b]) == h.r.found and pops[b] == h.r.loop_count and nn[b] == h.r.n_nodes
        assert np.array_equal(seq[b, : pops[b]], h.r.pop_sequence) and (seq[b, pops[b]:] == -1).all()
        assert np.array_equal(states[b, : ns[b]].T, h.r.hybrid_astar_states)
        assert np.array_equal(rs[b, : rl[b]].T, h.r.RSpath_final)
    assert hs[0].r.loop_count == 275 and hs[1].r.loop_count == 120


def test_plan_hybrid_astar_python_api(ctx):
    h = ha.driver_searcher(ha.PERPENDICULAR, use_astar=True)
    ha.planHybridAstar_(h, ctx=ctx)
    _check_plans([h], plan_refs()[:1])
    assert h.r.loop_count == 344
