"""The CPU restatement of planRRT! (tests/rrt_ref.py) against the reference's definitions: the rounding of
round(digits = 2), ProjectionStates' quirks, collision's end-point test, and the invariants of a grown tree."""
import functools
import math
import os
from fractions import Fraction

import numpy as np

import rrt_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obstacle_fields_64.npz")
BOUND = [0.0, 120.0, 0.0, 120.0]


def exact_round2(v):
    """rint(v * 100.0) / 100.0 with the rint done in exact rational arithmetic (half to even)."""
    p = v * 100.0
    if p == 0.0:
        return p / 100.0  # keeps the sign of zero
    q = Fraction(p)
    fl = q.numerator // q.denominator
    rem = q - fl
    n = fl + (1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1) else 0)
    out = float(n) / 100.0
    return -0.0 if (n == 0 and p < 0) else out


def test_round2_pins():
    # the rounding acts on the double product v * 100.0, not on the decimal literal
    for v in [0.125, 0.135, 2.675, 0.005, 0.015, 0.025, 1.005, -0.125, -0.135, -2.675, -0.004, 0.0, -0.0, 3.0, 1e-9,
              119.995, 0.285, 1.115]:
        got, want = R.round2(v), exact_round2(v)
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (v, got, want)
    assert R.round2(0.125) == 0.12        # 12.5 exactly: half to even
    assert R.round2(0.135) == 0.14        # 0.135 * 100.0 = 13.500000000000002
    assert R.round2(2.675) == 2.68        # the product rounds to 267.5 exactly, then half to even (decimal rounding: 2.67)
    assert R.round2(-0.125) == -0.12
    assert math.copysign(1.0, R.round2(-0.0)) == -1.0 and math.copysign(1.0, R.round2(-0.004)) == -1.0


def test_projection_states():
    # vertical segment: sign(0.0) = 0 makes dpsi = 0, the length lands on dx (the reference's behaviour)
    assert R.projection_states((1.0, 1.0), (1.0, 3.5)) == (2.5, 0.0)
    assert R.projection_states((1.0, 1.0), (1.0, -1.5))[0] == 2.5
    # rho < 0.001: zero
    assert R.projection_states((2.0, 2.0), (2.0005, 2.0005)) == (0.0, 0.0)
    # the four quadrants: dpsi = atan(dy / |dx|) * sign(dx) is an angle in (-pi/2, pi/2), so the projection is
    # (|dx|, dy * sign(dx)): a segment that points left comes back point-reflected (the reference's behaviour)
    for dx, dy in [(3.0, 4.0), (-3.0, 4.0), (-3.0, -4.0), (3.0, -4.0), (0.5, -0.25), (-1.234, 0.777)]:
        px, py = R.projection_states((10.0, 20.0), (10.0 + dx, 20.0 + dy))
        wx, wy = abs(dx), dy * math.copysign(1.0, dx)
        assert abs(px - wx) <= 0.005 + 1e-9 and abs(py - wy) <= 0.005 + 1e-9, (dx, dy, px, py)
        assert R.round2(px) == px and R.round2(py) == py
    assert R.projection_states((0.0, 0.0), (3.0, 4.0)) == (3.0, 4.0)
    assert R.projection_states((0.0, 0.0), (-3.0, 4.0)) == (3.0, -4.0)
    assert R.projection_states((0.0, 0.0), (-3.0, -4.0)) == (3.0, 4.0)
    assert R.projection_states((0.0, 0.0), (3.0, -4.0)) == (3.0, -4.0)


def test_steer_branches():
    # in range: the node is the sample itself, the cost is 5 * the rounded length
    loc, cost, inr = R.steer((0.0, 0.0), 1.0, (1.0, 2.0), 0.0, 3.0)
    assert inr and loc == (1.0, 2.0) and cost == 1.0 + 5.0 * math.sqrt(5.0)
    # out of range: pulled to grow_max along the rounded direction
    loc, cost, inr = R.steer((0.0, 0.0), 0.0, (30.0, 40.0), 0.0, 3.0)
    assert not inr and loc == (1.8, 2.4) and cost == 5.0 * math.sqrt(1.8 * 1.8 + 2.4 * 2.4)
    # the |dx| <= 0.01 clamp moves the node 0.01 to the right of a vertical pull... which is horizontal here
    loc, _, inr = R.steer((5.0, 5.0), 0.0, (5.0, 50.0), 0.0, 3.0)
    assert not inr and loc == (8.0, 5.0)


def test_collision_tests_end_points_only():
    circle = [(5.0, 0.0, 1.0)]
    # the segment crosses the circle, both end points are outside it: free (the reference's behaviour)
    assert not R.collision(circle, (0.0, 0.0), (10.0, 0.0), BOUND)
    assert R.collision(circle, (0.0, 0.0), (5.5, 0.0), BOUND)
    assert R.collision(circle, (4.5, 0.5), (10.0, 0.0), BOUND)      # the first point counts too
    assert R.collision(circle, (0.0, 0.0), (6.0, 0.0), BOUND)       # <=: on the rim
    assert R.collision([], (0.0, 0.0), (121.0, 0.0), BOUND)         # the bound test is on the second point
    assert not R.collision([], (-5.0, 0.0), (1.0, 0.0), BOUND)      # ... only
    assert not R.collision([], (0.0, 0.0), (120.0, 120.0), BOUND)


@functools.lru_cache(maxsize=None)
def run(rrt_star, buffer_size=7):
    z = np.load(GOLD)
    obs = R.field(z["circles"], z["count"], 53)
    U = np.random.default_rng(11).random((600, 3))
    return obs, R.plan(BOUND, (0.0, 0.0), (40.0, 40.0), obs, U, buffer_size, rrt_star, 0.2)


def check_tree(obs, out, bitwise):
    n, loc, cost, par = out["n_nodes"], out["loc"], out["cost"], out["parent"]
    assert par[0] == -1 and n > 100
    for i in range(1, n):
        k, steps = i + 1, 0
        while k != 1:
            k = par[k - 1]
            steps += 1
            assert 1 <= k <= n and steps <= n
        assert not R.out_of_bound(loc[i], BOUND)
        assert all((loc[i][0] - ox) ** 2 + (loc[i][1] - oy) ** 2 > r * r for ox, oy, r in obs)
        edge = R.neural_cost(R.projection_states(loc[par[i] - 1], loc[i]))
        step = cost[i] - cost[par[i] - 1]
        if bitwise:
            assert cost[i] == cost[par[i] - 1] + edge
        else:
            assert abs(step - edge) <= 1e-9 * abs(edge), (i, step, edge)  # relative to 5 * |proj|
    assert (loc[n:] == 0).all() and (cost[n:] == 0).all() and (par[n:] == 0).all()


def test_tree_invariants_rrt_star():
    obs, out = run(True)
    check_tree(obs, out, bitwise=False)
    rej, rew, capped, inr = out["counters"]
    assert rej >= 1 and rew >= 1 and capped >= 1 and inr >= 1 and out["status"] == 1
    assert out["n_nodes"] + rej == 601
    p = out["path_idx"]
    assert p[0] == out["best_idx"] and p[-1] == 1 and out["best_cost"] == out["cost"][p[0] - 1]


def test_tree_invariants_plain_rrt():
    obs, out = run(False)
    check_tree(obs, out, bitwise=True)
    assert out["counters"][1] == 0 and out["counters"][2] == 0


def test_stale_snapshot():
    # buffer_size = n_iter + 1: the BallTree is never rebuilt, every node hangs off node 1
    _, out = run(True, 601)
    assert (out["parent"][1: out["n_nodes"]] == 1).all() and out["n_nodes"] > 100
