"""The CPU restatement of the Dijkstra and breadth-first grid planners (tests/gridsearch_ref.py), pinned before
anything is compared with it: grids derived by hand from the reference's loops, the 7 x 5 scenes of the A* tests,
a 21 x 21 empty grid whose BFS levels outgrow 64 candidates, and two independent cross-checks on the 51 x 51
seeded circle field (Dijkstra's cost against A*'s, BFS's hop count against a numpy flood fill)."""
import functools
import math

import numpy as np

import astar_ref as A
import gridsearch_ref as R


def enc(g, cells):
    return [g.encode(c) for c in cells]


# ------------------------------------------------------------ 3 x 3, no obstacles (Encode indices)
def _unit3():
    return A.Grid([0, 2, 0, 2], 3, 3), np.ones((3, 3), np.uint8)


def test_dijkstra_3x3_up_right():
    g, m = _unit3()
    r = R.dka_search(g, (1, 1), (3, 3), m)
    assert r["found"] and r["pop_seq"] == [1, 2, 4, 5, 3, 7, 6, 8, 9] and r["pops"] == 9 and r["n_nodes"] == 9
    assert enc(g, r["path"]) == [1, 5, 9]
    assert r["path_length"] == math.sqrt(2) + math.sqrt(2) == r["final_cost"]


def test_dijkstra_3x3_missing_up_left_move():
    """(3,1) -> (1,3): there is no (-1, +1) in the direction list, so the cost is 4.0, not 2*sqrt(2)."""
    g, m = _unit3()
    r = R.dka_search(g, (3, 1), (1, 3), m)
    assert r["found"] and r["pop_seq"] == [3, 2, 6, 1, 5, 9, 4, 8, 7] and r["pops"] == 9 and r["n_nodes"] == 9
    assert enc(g, r["path"]) == [3, 2, 1, 4, 7]
    assert r["path_length"] == 4.0 and r["final_cost"] == 4.0


def test_bfs_3x3_up_right():
    g, m = _unit3()
    r = R.bfs_search(g, (1, 1), (3, 3), m)
    assert r["found"] and r["pop_seq"] == [1, 2, 4, 3, 5, 7, 6, 8, 9] and r["pops"] == 9 and r["n_nodes"] == 9
    assert enc(g, r["path"]) == [1, 2, 3, 6, 9] and r["path_length"] == 4.0
    assert r["queue"] == r["pop_seq"] and r["queue_left"] == []


def test_start_equals_goal_is_found_with_one_pop():
    g, m = _unit3()
    d, b = R.dka_search(g, (2, 2), (2, 2), m), R.bfs_search(g, (2, 2), (2, 2), m)
    for r in (d, b):
        assert r["found"] and r["pops"] == 1 and r["n_nodes"] == 1 and r["path"] == [(2, 2)]
        assert r["path_length"] == 0.0
    assert d["final_cost"] == 0.0


# ------------------------------------------------------------ 7 x 5, bound [0, 6, 0, 4]
B75 = [0.0, 6.0, 0.0, 4.0]


def test_7x5_walled_in_goal():
    obs = [[5.0, 4.0, 0.5], [5.0, 3.0, 0.5], [6.0, 3.0, 0.5]]
    d = R.plan_dka(B75, 7, 5, [0.0, 0.0], [6.0, 4.0], obs)
    b = R.plan_bfs(B75, 7, 5, [0.0, 0.0], [6.0, 4.0], obs)
    for r in (d, b):
        assert not r["found"] and r["pops"] == 31 and r["n_nodes"] == 31 and r["path"] == []
    assert d["final_cost"] == 0.0


def test_7x5_diagonal_gap_is_open_to_dijkstra_only():
    obs = [[5.0, 4.0, 0.5], [6.0, 3.0, 0.5]]
    d = R.plan_dka(B75, 7, 5, [0.0, 0.0], [6.0, 4.0], obs)
    assert d["found"] and d["pops"] == 33 and d["final_cost"] == 7.65685424949238
    assert d["path"][-2:] == [(6, 4), (7, 5)]  # through the gap by the (1, 1) move
    b = R.plan_bfs(B75, 7, 5, [0.0, 0.0], [6.0, 4.0], obs)
    assert not b["found"] and b["pops"] == 32


def test_7x5_bfs_goal_level_mates_stay_queued():
    r = R.plan_bfs(B75, 7, 5, [0.0, 0.0], [2.0, 1.0], [])
    assert r["found"] and r["pops"] == 8 and r["n_nodes"] == 12 and r["goal_depth"] == 3
    assert r["queue_left_depth"] == [3, 3, 4, 4]
    assert r["queue"][:8] == r["pop_seq"] and r["queue"][8:] == r["queue_left"]


# ------------------------------------------------------------ 21 x 21 empty, bound [0, 20, 0, 20]
B21 = [0.0, 20.0, 0.0, 20.0]


def test_21x21_bfs_goal_mid_level_and_wide_levels():
    r = R.plan_bfs(B21, 21, 21, [0.0, 0.0], [11.0, 10.0], [])
    assert r["path"][-1] == (12, 11)
    assert r["found"] and r["pops"] == 241 and r["n_nodes"] == 260 and r["goal_depth"] == 21
    assert r["queue_left_depth"].count(21) == 10
    full = R.plan_bfs(B21, 21, 21, [0.0, 0.0], [29.0, 29.0], [])  # goal off the grid
    assert not full["found"] and full["pops"] == 441 and full["n_nodes"] == 441
    widest = max(np.bincount(full["depth"]))
    assert widest == 21 and 4 * widest > 64  # 84 candidates: more than one 64-lane chunk


def test_21x21_dijkstra_goal_off_grid_exhausts():
    r = R.plan_dka(B21, 21, 21, [0.0, 0.0], [29.0, 29.0], [])
    assert not r["found"] and r["pops"] == 441 and r["n_nodes"] == 441 and not r["capped"]


# ------------------------------------------------------------ 51 x 51 seeded circle field
def circle_field():
    """test_gpu_astar.circle_field()'s generator."""
    r = np.random.default_rng(53)
    obs = np.c_[r.uniform(8, 112, 40), r.uniform(8, 112, 40), r.uniform(3, 9, 40)]
    return [0.0, 120.0, 0.0, 120.0], [0.0, 0.0], [120.0, 120.0], obs


@functools.lru_cache(maxsize=None)
def field_refs():
    b, s, g, obs = circle_field()
    return R.plan_dka(b, 51, 51, s, g, obs), R.plan_bfs(b, 51, 51, s, g, obs), A.plan(b, 51, 51, s, g, obs, 3)


def test_dijkstra_cost_equals_astar_cost_on_the_circle_field():
    """Both planners are optimal on the same directed graph; a path sums at most 2,601 terms of relative error
    2^-53 each (2.9e-13), so the two costs agree within rtol 1e-12."""
    d, _, a = field_refs()
    assert d["found"] and a["found"]
    assert abs(d["final_cost"] - a["final_cost"]) <= 1e-12 * abs(a["final_cost"])
    assert d["final_cost"] == 196.41748904055837
    assert (d["pops"], d["n_nodes"], d["max_open"]) == (1873, 1878, 73) and a["pops"] == 1006


def test_bfs_hops_equal_flood_fill_distance_on_the_circle_field():
    b, s, g, obs = circle_field()
    _, r, _ = field_refs()
    grid = A.Grid(b, 51, 51)
    free = A.free_mask(grid, obs, 3).astype(bool)
    sx, sy = grid.cell(s)
    gx, gy = grid.cell(g)
    dist = np.full((51, 51), -1)
    dist[sy - 1, sx - 1] = 0  # (the start cell is never tested against the circles)
    front = np.zeros((51, 51), bool)
    front[sy - 1, sx - 1] = True
    k = 0
    while front.any():
        k += 1
        grow = np.zeros_like(front)
        grow[1:, :] |= front[:-1, :]
        grow[:-1, :] |= front[1:, :]
        grow[:, 1:] |= front[:, :-1]
        grow[:, :-1] |= front[:, 1:]
        front = grow & free & (dist < 0)
        dist[front] = k
    assert r["found"] and len(r["path"]) - 1 == dist[gy - 1, gx - 1] == r["goal_depth"]
    assert (len(r["path"]), r["pops"], r["n_nodes"]) == (101, 1863, 1869)
    assert r["path_length"] == 240.00000000000017
    # every queued node sits at its flood-fill distance
    assert all(dist[(e - 1) // 51, (e - 1) % 51] == d for e, d in zip(r["queue"], r["depth"]))
