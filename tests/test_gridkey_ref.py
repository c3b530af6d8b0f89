"""The (f, seq) ordering rule of the large-grid kernels (tests/gridkey_ref.py) against the sorting restatements
astar_ref.search and gridsearch_ref.dka_search, on seeded random masks -- no GPU."""
import functools

import numpy as np
import pytest

import astar_ref as A
import gridkey_ref as K
import gridsearch_ref as R

# (nx, ny, bound): x_factor != y_factor in every one
GRIDS = [(20, 17, [0.0, 10.0, 0.0, 3.0]), (33, 41, [-2.0, 5.0, 1.0, 30.0]), (57, 23, [0.0, 12.0, -3.0, 4.1]),
         (80, 70, [0.0, 100.0, 0.0, 55.0]), (24, 24, [0.0, 23.0, 0.0, 46.0])]
DENSITIES = [0.0, 0.1, 0.25, 0.35]
# (grid, density, A* or Dijkstra); the last grid (y_factor = 2 x_factor: many equal f) only at density 0.1, where
# A* pops a push and an in-open decrease of one iteration that tie in f -- the input that tells the rules apart
CASES = [(gi, di, dka) for gi in range(len(GRIDS)) for di in range(len(DENSITIES)) for dka in (False, True)
         if gi < 4 or di == 1]
SEEDS = {(4, 1): 58}


def case_input(gi, di):
    nx, ny, bound = GRIDS[gi]
    rs = np.random.RandomState(SEEDS.get((gi, di), 1000 + 10 * gi + di))
    mask = (rs.rand(ny, nx) >= DENSITIES[di]).astype(np.uint8)
    spos = (int(rs.randint(1, nx // 4 + 1)), int(rs.randint(1, ny // 4 + 1)))
    gpos = (int(rs.randint(3 * nx // 4, nx + 1)), int(rs.randint(3 * ny // 4, ny + 1)))
    mask[spos[1] - 1, spos[0] - 1] = mask[gpos[1] - 1, gpos[0] - 1] = 1
    if (gi, di) == (2, 3):  # a blocked column: the search exhausts the start's side
        mask[:, nx // 2 - 1] = 0
    return A.Grid(bound, nx, ny), spos, gpos, mask


@functools.lru_cache(maxsize=None)
def run(gi, di, dka, rule="key"):
    grid, spos, gpos, mask = case_input(gi, di)
    ref = (R.dka_search if dka else A.search)(grid, spos, gpos, mask)
    return ref, K.search(grid, spos, gpos, mask, dka=dka, rule=rule)


def same(ref, got):
    return (got["pop_seq"] == ref["pop_seq"] and got["path"] == ref["path"] and got["n_nodes"] == ref["n_nodes"]
            and got["final_cost"] == ref["final_cost"] and got["found"] == ref["found"])


@pytest.mark.parametrize("gi,di,dka", CASES)
def test_key_rule_is_the_stable_sort(gi, di, dka):
    """Pop sequence, parent chain, cost, node count and path length are the sorting reference's."""
    ref, got = run(gi, di, dka)
    assert got["pop_seq"] == ref["pop_seq"] and got["pops"] == ref["pops"]
    assert got["n_nodes"] == ref["n_nodes"] and got["found"] == ref["found"]
    assert got["final_cost"] == ref["final_cost"] and got["path_length"] == ref["path_length"]
    assert got["path"] == ref["path"]  # the goal's parent chain
    assert not got["capped"] and ref["pops"] > 10


def test_inputs_exercise_the_rule():
    outs = [run(*c)[1] for c in CASES]
    assert sum(o["multi_dec"] for o in outs) >= 20
    assert sum(o["equal_f"] for o in outs) >= 20  # A* updates that keep f, and so their number
    assert any(o["found"] for o in outs) and any(not o["found"] for o in outs)


def test_direction_order_rule_differs():
    """Numbering pushes and decreases together in direction order is not the stable sort: at least one input
    tells the two apart, so the comparison above can fail."""
    assert any(not same(*run(gi, di, dka, "direction")) for gi, di, dka in CASES)
