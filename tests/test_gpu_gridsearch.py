"""GPU parity of the Dijkstra and breadth-first grid planners (motionplanning_amd/csrc/astar.hip: mp_dka_plan,
mp_bfs_plan; motionplanning_amd/{dijkstra,bfs}.py) against the CPU restatement tests/gridsearch_ref.py -- BIT-EXACT
cost, path length, found, pops, node counts, pop order and paths, one call per group and planner."""
import functools
import math

import numpy as np
import pytest

import astar_ref as A
import gridsearch_ref as R
from motionplanning_amd import bfs, dijkstra
from motionplanning_amd.abi import ptr

pytestmark = pytest.mark.gpu

PLANNERS = ["dka", "bfs"]
REF = {"dka": R.plan_dka, "bfs": R.plan_bfs}


def gpu_plan(ctx, planner, nx, ny, rows):
    """mp_dka_plan / mp_bfs_plan for the searches rows = [(bound, start, goal, circles)].  The C call takes one
    circle count: shorter lists are padded with [0, 0, 0] (never hit), as dijkstra.plan_batch / bfs.plan_batch do."""
    B, M = len(rows), nx * ny + 1
    bound, start, goal = (np.ascontiguousarray([r[k] for r in rows], np.float64) for k in range(3))
    n_obs = max(len(r[3]) for r in rows)
    obs = np.zeros((B, n_obs, 3))
    for b, r in enumerate(rows):
        if len(r[3]):
            obs[b, : len(r[3])] = r[3]
    cost, plen = np.zeros(B), np.zeros(B)
    found, pops, nn, pn = (np.zeros(B, np.int32) for _ in range(4))
    seq, path = np.zeros((B, 2 * M), np.int32), np.zeros((B, M), np.int32)
    head = (ctx.handle, B, nx, ny, ptr(bound), ptr(start), ptr(goal), n_obs, ptr(obs) if n_obs else None)
    tail = (ptr(found), ptr(pops), ptr(nn), ptr(seq), ptr(path), ptr(pn), ptr(plen))
    if planner == "dka":
        ctx.check(ctx.lib.mp_dka_plan(*head, ptr(cost), *tail))
    else:
        ctx.check(ctx.lib.mp_bfs_plan(*head, *tail))
    return dict(cost=cost, plen=plen, found=found, pops=pops, nn=nn, pn=pn, seq=seq, path=path)


def check_against_ref(planner, out, b, ref, grid):
    if planner == "dka":
        assert out["cost"][b].tobytes() == np.float64(ref["final_cost"]).tobytes(), (b, out["cost"][b], ref["final_cost"])
    assert bool(out["found"][b]) == ref["found"] and out["pops"][b] == ref["pops"] and out["nn"][b] == ref["n_nodes"], b
    assert list(out["seq"][b, : ref["pops"]]) == ref["pop_seq"] and (out["seq"][b, ref["pops"]:] == -1).all(), b
    assert list(out["path"][b, : out["pn"][b]]) == [grid.encode(c) for c in ref["path"]], b
    assert out["plen"][b].tobytes() == np.float64(ref["path_length"]).tobytes(), b


# ---- (nx, ny) groups; rows = (bound, start, goal, circles)
U3 = [0.0, 2.0, 0.0, 2.0]
B75 = [0.0, 6.0, 0.0, 4.0]
HA_BOX = [-5.0, 10.0, 0.0, 10.0]
B21 = [0.0, 20.0, 0.0, 20.0]
TWO_11 = [[2.0, 3.0, 1.2], [5.0, 6.0, 1.0]]
GROUPS = {
    "unit3": (3, 3, [
        (U3, [0.0, 0.0], [2.0, 2.0], []),  # (1,1) -> (3,3)
        (U3, [2.0, 0.0], [0.0, 2.0], []),  # (3,1) -> (1,3): no (-1, +1) move for Dijkstra
        (U3, [1.0, 1.0], [1.2, 1.3], []),  # start cell == goal cell
    ]),
    "grid75": (7, 5, [  # nx != ny; rows 0-4 are test_gpu_astar.py's CIRCLES_75 and WALLED_75
        (B75, [0.2, 0.1], [5.9, 3.9], [[3.0, 1.0, 1.2], [3.0, 3.2, 0.9]]),
        ([0.0, 12.0, -2.0, 2.0], [11.0, 1.9], [0.5, -1.5], [[6.0, 0.0, 1.1], [2.0, -2.0, 0.7]]),
        (B75, [0.0, 0.0], [6.0, 4.0], [[5.0, 4.0, 0.5], [5.0, 3.0, 0.5]]),
        (B75, [0.0, 0.0], [6.0, 4.0], [[5.0, 4.0, 0.5], [6.0, 3.0, 0.5]]),  # the diagonal gap
        (B75, [0.0, 0.0], [6.0, 4.0], [[5.0, 4.0, 0.5], [5.0, 3.0, 0.5], [6.0, 3.0, 0.5]]),  # walled in
        (B75, [0.0, 0.0], [2.0, 1.0], []),  # BFS: the goal's level-mates are still queued when it pops
    ]),
    "box11": (11, 11, [
        (HA_BOX, [-5.5, 3.0], [8.0, 3.0], TWO_11),  # start one cell off the grid: steps onto it
        (HA_BOX, [-7.0, 3.0], [8.0, 3.0], TWO_11),  # start two cells off the grid: one pop
        (HA_BOX, [7.0, 3.0], [12.5, 3.0], TWO_11),  # goal outside the bound: never reached
    ]),
    "empty21": (21, 21, [  # BFS levels of up to 21 nodes = 84 candidates, the goal of row 0 mid-level
        (B21, [0.0, 0.0], [11.0, 10.0], []),
        (B21, [0.0, 0.0], [29.0, 29.0], []),
    ]),
}


@functools.lru_cache(maxsize=None)
def group_refs(name, planner):
    nx, ny, rows = GROUPS[name]
    return [REF[planner](b, nx, ny, s, g, o) for b, s, g, o in rows]


@pytest.mark.parametrize("planner", PLANNERS)
@pytest.mark.parametrize("name", list(GROUPS))
def test_plan_bitexact(ctx, name, planner):
    nx, ny, rows = GROUPS[name]
    out = gpu_plan(ctx, planner, nx, ny, rows)
    refs = group_refs(name, planner)
    for b, (row, ref) in enumerate(zip(rows, refs)):
        check_against_ref(planner, out, b, ref, A.Grid(row[0], nx, ny))
    if name == "unit3":  # the hand-derived rows, on the GPU's own outputs
        want = {"dka": ([1, 2, 4, 5, 3, 7, 6, 8, 9], [1, 5, 9], 2 * math.sqrt(2)),
                "bfs": ([1, 2, 4, 3, 5, 7, 6, 8, 9], [1, 2, 3, 6, 9], 4.0)}[planner]
        assert list(out["seq"][0, :9]) == want[0] and list(out["path"][0, : out["pn"][0]]) == want[1]
        assert out["plen"][0] == want[2] and out["pops"][0] == 9 and out["nn"][0] == 9
        if planner == "dka":
            assert out["cost"][0] == want[2] and out["cost"][1] == 4.0
            assert list(out["seq"][1, :9]) == [3, 2, 6, 1, 5, 9, 4, 8, 7] and list(out["path"][1, :5]) == [3, 2, 1, 4, 7]
        assert out["found"][2] == 1 and out["pops"][2] == 1 and out["pn"][2] == 1 and out["plen"][2] == 0.0
        assert out["nn"][2] == 1 and out["cost"][2] == 0.0
    if name == "grid75":
        assert [r["found"] for r in refs][2:5] == {"dka": [True, True, False], "bfs": [True, False, False]}[planner]
        assert refs[4]["pops"] == 31 and refs[3]["pops"] == {"dka": 33, "bfs": 32}[planner]
        if planner == "bfs":
            assert refs[5]["goal_depth"] in refs[5]["queue_left_depth"] and refs[5]["pops"] == 8
            assert out["nn"][5] == 12
    if name == "box11":
        assert [r["found"] for r in refs] == [True, False, False]
        assert refs[0]["pop_seq"][0] == 0 and refs[1]["pops"] == 1  # the off-grid start is slot 0
    if name == "empty21":
        assert refs[1]["pops"] == 441 and not refs[1]["found"]
        if planner == "bfs":
            assert (refs[0]["pops"], refs[0]["n_nodes"]) == (241, 260)
            assert refs[0]["queue_left_depth"].count(refs[0]["goal_depth"]) == 10
            assert 4 * max(np.bincount(refs[1]["depth"])) > 64


# ---- 51 x 51 circle field (test_gpu_astar.circle_field()'s generator): the largest LDS footprint, and for
# Dijkstra the dynamic-LDS attribute above 48 KB
def circle_field():
    r = np.random.default_rng(53)
    obs = np.c_[r.uniform(8, 112, 40), r.uniform(8, 112, 40), r.uniform(3, 9, 40)]
    return [0.0, 120.0, 0.0, 120.0], [0.0, 0.0], [120.0, 120.0], obs


@functools.lru_cache(maxsize=None)
def circle_field_ref(planner):
    b, s, g, obs = circle_field()
    return REF[planner](b, 51, 51, s, g, obs)


@pytest.mark.parametrize("planner", PLANNERS)
def test_plan_51x51_circle_field_bitexact(ctx, planner):
    b, s, g, obs = circle_field()
    ref = circle_field_ref(planner)
    assert ref["found"] and ref["pops"] == {"dka": 1873, "bfs": 1863}[planner]
    out = gpu_plan(ctx, planner, 51, 51, [(b, s, g, obs)])
    check_against_ref(planner, out, 0, ref, A.Grid(b, 51, 51))


# ---- Python API
def _searcher(planner, b, n, s, g, obs):
    if planner == "dka":
        a = dijkstra.defineDKA(b, [n, n], s, g)
        dijkstra.defineDKAobs_(a, obs)
    else:
        a = bfs.defineBFS(b, [n, n], s, g)
        bfs.defineBFSobs_(a, obs)
    return a


def _check_searcher(planner, a, ref):
    r = a.r
    assert r.found == ref["found"] and r.loop_count == ref["pops"] and r.n_nodes == ref["n_nodes"]
    assert list(r.pop_sequence) == ref["pop_seq"]
    assert r.path_length == ref["path_length"]
    assert [tuple(c) for c in (r.dkapath if planner == "dka" else r.bfspath)] == ref["path"]
    assert np.array_equal(r.actualpath, np.array(ref["actualpath"]).reshape(-1, 2))
    if planner == "dka":
        assert r.final_cost == ref["final_cost"]
    else:
        assert not hasattr(r, "final_cost")


@pytest.mark.parametrize("planner", PLANNERS)
def test_plan_python_api(ctx, planner):
    b, s, g, obs = circle_field()
    a = _searcher(planner, b, 51, s, g, obs)
    assert (dijkstra.planDKA_ if planner == "dka" else bfs.planBFS_)(a, ctx=ctx) is None
    assert a.r.found and a.r.planning_time > 0.0
    _check_searcher(planner, a, circle_field_ref(planner))


def mixed_fields():
    """Four seeded 21 x 21 fields with 2, 5, 5 and 9 circles."""
    r = np.random.default_rng(21)
    return [(B21, [0.0, 0.0], [13.0, 17.0], np.c_[r.uniform(3, 17, n), r.uniform(3, 17, n), r.uniform(1.0, 2.5, n)])
            for n in (2, 5, 5, 9)]


@functools.lru_cache(maxsize=None)
def mixed_refs(planner):
    return [REF[planner](b, 21, 21, s, g, o) for b, s, g, o in mixed_fields()]


@pytest.mark.parametrize("planner", PLANNERS)
def test_plan_batch_pads_mixed_obstacle_counts(ctx, planner):
    """plan_batch pads the shorter lists with [0, 0, 0] circles: each padded result is the unpadded
    single-searcher call's and the restatement's."""
    mod = dijkstra if planner == "dka" else bfs
    fields, refs = mixed_fields(), mixed_refs(planner)
    batch = [_searcher(planner, b, 21, s, g, o) for b, s, g, o in fields]
    assert [len(a.s.obstacle_list) for a in batch] == [2, 5, 5, 9]
    mod.plan_batch(batch, ctx=ctx)
    for (b, s, g, o), a, ref in zip(fields, batch, refs):
        _check_searcher(planner, a, ref)
        one = _searcher(planner, b, 21, s, g, o)
        mod.plan_batch([one], ctx=ctx)
        _check_searcher(planner, one, ref)
        assert np.array_equal(one.r.pop_sequence, a.r.pop_sequence) and one.r.path_length == a.r.path_length
    assert any(r["found"] for r in refs)


# ---- limits
@pytest.mark.parametrize("planner", PLANNERS)
def test_limits(ctx, planner):
    z, found, pops, nn = np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    b, s = np.array([[0.0, 1, 0, 1]]), np.array([[0.0, 0.0]])
    c = np.array([[[0.5, 0.5, 0.1]]])

    def call(nx, ny, n_obs, circles):
        head = (ctx.handle, 1, nx, ny, ptr(b), ptr(s), ptr(s), n_obs, circles)
        tail = (ptr(found), ptr(pops), ptr(nn), None, None, None, None)
        if planner == "dka":
            return ctx.lib.mp_dka_plan(*head, ptr(z), *tail)
        return ctx.lib.mp_bfs_plan(*head, *tail)

    assert call(52, 51, 0, None) != 0 and b"51" in ctx.lib.mp_last_error(ctx.handle)
    assert call(3, 3, 1, None) != 0 and b"obstacle" in ctx.lib.mp_last_error(ctx.handle)
    assert call(3, 3, 1, ptr(c)) == 0 and (found[0], pops[0], nn[0]) == (1, 1, 1)  # start == goal, every output optional
