"""The yardstick of mp_grid_field on the CPU: the two restatements of tests/gridfield_ref.py agree bit for bit, the
field is what planDKA!'s restatement (tests/gridsearch_ref.py) leaves behind, and the case set of
tests/gridfield_cases.py covers what it claims."""
import functools
import math

import numpy as np
import pytest

import gridfield_cases as C
import gridfield_ref as F
import gridsearch_ref as S

SMALL = C.small_cases()
MOVE_SETS = [F.MOVES_REF, F.MOVES_8, F.MOVES_4]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def src_of(case):
    g = C.grid_of(case)
    return g, F.source_cell(g, C.real(case, case["source"]))


@functools.lru_cache(maxsize=None)
def ref_field(i, moves=F.MOVES_REF, to_source=False):
    case = SMALL[i]
    g, src = src_of(case)
    return F.field_heap(g, case["mask"], src, moves, to_source)


def ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def test_real_points_fall_in_their_cells():
    for case in SMALL:
        g = C.grid_of(case)
        for cell in [case["source"]] + case["queries"]:
            assert g.cell(C.real(case, cell)) == tuple(cell)


@pytest.mark.parametrize("to_source", [False, True])
@pytest.mark.parametrize("moves", MOVE_SETS)
def test_the_two_restatements_are_bit_equal(moves, to_source):
    for i, case in enumerate(SMALL):
        g, src = src_of(case)
        jac, rounds = F.field_jacobi(g, case["mask"], src, moves, to_source)
        assert np.array_equal(bits(ref_field(i, moves, to_source)), bits(jac)), case["name"]
        assert rounds <= case["nx"] * case["ny"]


def test_serpentine_figures():
    case = C.serpentine()
    g, src = src_of(case)
    f, rounds = F.field_jacobi(g, case["mask"], src)
    assert np.array_equal(bits(f), bits(F.field_heap(g, case["mask"], src)))
    assert int(np.isfinite(f).sum()) == 4453 and not np.isinf(f[case["mask"] != 0]).any()
    assert rounds + 1 == 4420  # with the round that changes nothing and so proves the fixed point
    far = float(f[np.isfinite(f)].max())
    assert abs(far - 2074.72) < 0.01
    iy, ix = np.unravel_index(np.argmax(np.where(np.isfinite(f), f, -1.0)), f.shape)
    assert len(F.walk(g, f, src, (int(ix) + 1, int(iy) + 1))) - 1 == rounds  # a round a move


def test_field_is_what_planDKA_leaves():
    """dka_search from the source to each free cell: final_cost == field bit for bit, found <=> finite; an
    exhausted search (goal (0, 0), never popped) has n_nodes == n_reached."""
    checked = 0
    for i, case in enumerate(SMALL):
        g, src = src_of(case)
        if src is None:
            continue
        f = ref_field(i)
        mask = case["mask"]
        for iy in range(1, g.ny + 1):
            for ix in range(1, g.nx + 1):
                if not mask[iy - 1, ix - 1] and (ix, iy) != src:
                    assert math.isinf(f[iy - 1, ix - 1])
                    continue
                r = S.dka_search(g, src, (ix, iy), mask)
                assert r["found"] == bool(np.isfinite(f[iy - 1, ix - 1])), (case["name"], ix, iy)
                if r["found"]:
                    assert bits(r["final_cost"]) == bits(f[iy - 1, ix - 1]), (case["name"], ix, iy)
                    checked += 1
        spent = S.dka_search(g, src, (0, 0), mask)
        assert not spent["found"] and not spent["capped"]
        assert spent["n_nodes"] == int(np.isfinite(f).sum()), case["name"]
    assert checked > 500


def test_moves4_on_unit_cells_counts_bfs_steps():
    n = 0
    for i, case in enumerate(SMALL):
        g, src = src_of(case)
        if src is None or g.xf != 1.0 or g.yf != 1.0:
            continue
        f = ref_field(i, F.MOVES_4)
        for cell in case["queries"]:
            if g.encode(cell) == 0 or not (case["mask"][cell[1] - 1, cell[0] - 1] or cell == src):
                continue
            r = S.bfs_search(g, src, cell, case["mask"])
            assert r["found"] == bool(np.isfinite(f[cell[1] - 1, cell[0] - 1]))
            if r["found"]:
                assert f[cell[1] - 1, cell[0] - 1] == len(r["path"]) - 1
                n += 1
    assert n >= 8


def test_paths_follow_the_rule_and_fold():
    for to_source in (False, True):
        for i, case in enumerate(SMALL):
            g, src = src_of(case)
            f = ref_field(i, F.MOVES_8, to_source)
            q = F.queries(g, f, src, [C.real(case, c) for c in case["queries"]], case["stride"], F.MOVES_8, to_source)
            for k, p in enumerate(q["paths"]):
                if not p:
                    assert math.isinf(q["q_cost"][k])
                    continue
                ends = (p[-1], p[0]) if to_source else (p[0], p[-1])
                assert ends == (g.encode(src), g.encode(case["queries"][k]))
                costs = [f.reshape(-1)[e - 1] for e in p]
                assert all(a > b for a, b in zip(costs, costs[1:])) if to_source else all(a < b for a, b in zip(costs, costs[1:]))
                assert abs(q["path_length"][k] - q["q_cost"][k]) <= 1e-9 * max(1.0, q["q_cost"][k])


# ---- coverage the set claims
def by_name(name):
    i = [c["name"] for c in SMALL].index(name)
    return i, SMALL[i]


def test_covers_a_near_tie_on_non_square_cells():
    """A cell whose second candidate lies within 8 ulp of its minimum, the two not equal: the arithmetic order
    decides the bits."""
    near = 0
    for i, case in enumerate(SMALL):
        g, src = src_of(case)
        if src is None or g.xf == g.yf:
            continue
        f = ref_field(i)
        for iy in range(1, g.ny + 1):
            for ix in range(1, g.nx + 1):
                if (ix, iy) == src or not np.isfinite(f[iy - 1, ix - 1]):
                    continue
                t = sorted(set(c[1] for c in F.candidates(g, f, (ix, iy))))
                assert t[0] == f[iy - 1, ix - 1]
                near += len(t) > 1 and ulps(t[0], t[1]) <= 8
    assert near >= 5


def test_covers_pocket_offgrid_blocked_source_and_corner():
    i, case = by_name("pocket")
    g, src = src_of(case)
    f = ref_field(i, F.MOVES_8)
    assert case["mask"][5, 6] and math.isinf(f[5, 6]) and np.isfinite(f[case["mask"] != 0]).sum() == case["mask"].sum() - 1
    q = F.queries(g, f, src, [C.real(case, c) for c in case["queries"]], 64, F.MOVES_8)
    assert list(q["path_n"][:3]) == [0, 0, 0] and np.isinf(q["q_cost"][:3]).all() and (q["path_n"][3:] > 0).all()
    i, case = by_name("blocked_source_spreads")
    assert case["mask"][3, 4] == 0 and np.isfinite(ref_field(i)).sum() == case["mask"].sum() + 1
    assert by_name("all_free_corner")[1]["source"] == (1, 1)
    i, case = by_name("all_free_corner")
    assert np.isfinite(ref_field(i)).all()
    i, case = by_name("all_blocked_but_source")
    assert np.isfinite(ref_field(i)).sum() == 1 and ref_field(i)[1, 2] == 0.0
    i, case = by_name("source_off_grid")
    assert src_of(case)[1] is None and np.isinf(ref_field(i)).all()


def test_covers_a_cell_only_moves8_reaches():
    i, case = by_name("staircase")
    assert np.isfinite(ref_field(i, F.MOVES_8)).sum() == 5 and np.isfinite(ref_field(i, F.MOVES_REF)).sum() == 1
    i, case = by_name("staircase_down")
    assert np.isfinite(ref_field(i, F.MOVES_REF)).sum() == 5


def test_covers_a_path_rule_tie_and_a_cut_path():
    i, case = by_name("all_free_corner")
    g, src = src_of(case)
    f = ref_field(i)
    tied = [c for c in F.candidates(g, f, (3, 2)) if c[1] == f[1, 2]]
    assert [c[0] for c in tied] == [3, 4]  # (1, 0) from (2, 2) and (1, 1) from (2, 1): the lower bit wins
    assert F.walk(g, f, src, (3, 2)) == [g.encode(c) for c in [(1, 1), (2, 2), (3, 2)]]
    i, case = by_name("stride_cut")
    g, src = src_of(case)
    q = F.queries(g, ref_field(i), src, [C.real(case, c) for c in case["queries"]], case["stride"])
    assert q["path_n"][0] == 12 > case["stride"] and (q["path"][0] > 0).all() and q["path_n"][1] <= case["stride"]
