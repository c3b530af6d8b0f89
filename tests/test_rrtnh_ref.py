"""The CPU restatement of the car-like planRRT! (tests/rrtnh_ref.py) against the reference's definitions
(PathPlanning/RRTNonholonomic/src/{rrt_utils,types}.jl): rounding, ProjectionStates on hand-computed poses,
MyMetrics, InitialCheck and FeasibilityClassifier at their boundaries, both steer branches, the order of the tests
in collision, the stale BallTree snapshot, the invariants of a grown RRT* tree, and the ABI side of mp_rrtnh_plan.
No GPU."""
import functools
import math
import os

import numpy as np

import rrt_ref
import rrtnh_ref as N
import test_julia_binding as J
from motionplanning_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "obstacle_fields_64.npz")
BOUND = [0.0, 120.0, 0.0, 120.0]


def bits(x):
    return np.float64(x).tobytes()


# ---- round(v, digits = d)
def test_round_digits_on_ties():
    # v * 10^d is exact for these, so rint sees a true tie and rounds it to even
    assert N.round_digits(0.125, 2) == 0.12 and N.round_digits(0.375, 2) == 0.38
    assert N.round_digits(-0.125, 2) == -0.12 and N.round_digits(2.5e-3 * 0.5, 3) == 0.001  # 1.25 -> 1
    assert N.round_digits(0.0625, 3) == 0.062 and N.round_digits(0.1875, 3) == 0.188
    # 2.675 is below the tie in binary, but the product 2.675 * 100.0 rounds to 267.5: the tie goes to 268
    assert 2.675 * 100.0 == 267.5 and N.round_digits(2.675, 2) == 2.68
    assert N.round_digits(1.0000000002, 2) == 1.0 and N.round_digits(-1.0000000002, 2) == -1.0
    assert math.isnan(N.round_digits(math.nan, 2))
    assert math.copysign(1.0, N.round_digits(-0.001, 2)) == -1.0  # rint keeps the sign of zero


def test_fma_has_one_rounding():
    a = 1.0 + 2.0 ** -30
    assert N.fma(a, a, -1.0) == 2.0 ** -29 + 2.0 ** -60  # a*a rounds the last term away
    assert a * a - 1.0 == 2.0 ** -29
    assert N.fma(3.0, 4.0, 5.0) == 17.0 and math.isnan(N.fma(math.inf, 0.0, 1.0))


# ---- ProjectionStates
def test_projection_states_hand_computed():
    o = [0.0, 0.0, 0.0]
    assert N.projection_states(o, [2.0, 0.0, 0.0]) == [2.0, 0.0, 0.0]            # ahead
    assert N.projection_states(o, [0.0, 2.0, 0.0]) == [0.0, 2.0, 0.0]            # left: acos(0) * (+1)
    assert N.projection_states(o, [0.0, -2.0, 0.0]) == [0.0, -2.0, 0.0]          # right: acos(0) * (-1)
    # behind: the cross product is 0 and Base's sign(0.0) = 0.0, so dpsi = pi * 0 = 0 and the point reads as ahead
    assert N.projection_states(o, [-2.0, 0.0, 0.0]) == [2.0, 0.0, 0.0]
    # behind and a little to the left: acos(round(-0.999.., 2)) = acos(-1) = pi, dy = round(rho * sin(pi)) = 0
    assert N.projection_states(o, [-2.0, 0.01, 0.0]) == [-2.0, 0.0, 0.0]
    # the cosine is rounded to 2 digits first: 3-4-5 gives exactly 0.6 and 0.8
    assert N.projection_states(o, [3.0, 4.0, 0.0]) == [3.0, 4.0, 0.0]
    assert N.projection_states(o, [3.0, -4.0, 0.0]) == [3.0, -4.0, 0.0]
    # rounding the cosine moves the point: (10, 0.3) has cos = 0.99955 -> 1.0, so dy = 0
    assert N.projection_states(o, [10.0, 0.3, 0.0]) == [10.0, 0.0, 0.0]
    # a turned frame: heading pi/2, a point straight ahead of it
    assert N.projection_states([1.0, 1.0, math.pi / 2], [1.0, 3.0, math.pi / 2]) == [2.0, 0.0, 0.0]
    assert N.projection_states([1.0, 1.0, math.pi / 2], [3.0, 1.0, 0.0])[:2] == [0.0, -2.0]


def test_projection_states_coincident_and_yaw_difference():
    assert N.projection_states([5.0, 5.0, 0.3], [5.0, 5.0, 0.3]) == [0.0, 0.0, 0.0]
    assert N.projection_states([5.0, 5.0, 0.3], [5.0005, 5.0, 0.3]) == [0.0, 0.0, 0.0]  # norm < 0.001
    assert N.projection_states([5.0, 5.0, 0.3], [5.001, 5.0, 0.3])[0] == 0.0            # rho = 0.001 rounds to 0.0
    # the heading difference is rounded to 3 digits, second minus first
    assert N.projection_states([0.0, 0.0, 0.1], [1.0, 0.0, 0.35049])[2] == 0.25
    assert N.projection_states([0.0, 0.0, 0.35049], [1.0, 0.0, 0.1])[2] == -0.25
    assert N.projection_states([0.0, 0.0, 0.0], [1.0, 0.0, 0.0625])[2] == 0.062  # a tie at 3 digits, to even


# ---- MyMetrics
def test_metric_is_bitwise_symmetric():
    rng = np.random.default_rng(7)
    for _ in range(300):
        a = [float(v) for v in rng.uniform(-50, 50, 2)] + [float(rng.uniform(-4, 4))]
        b = [float(v) for v in rng.uniform(-50, 50, 2)] + [float(rng.uniform(-4, 4))]
        assert bits(N.metric(a, b)) == bits(N.metric(b, a)), (a, b)
        assert N.metric(a, b) >= 0.0


def test_metric_near_vertical_branch_and_value():
    # |dx| <= 0.01 takes rho = pi/2, whatever the sign of dy
    a, b = [1.0, 0.0, 0.2], [1.0078125, 5.0, -0.1]
    assert abs(a[0] - b[0]) <= 0.01
    r = math.sqrt((b[0] - a[0]) ** 2 + 25.0) + 0.1
    rho = math.pi / 2
    w = r * math.sin(((0.2 + -0.1) / 2 - rho) * 2)
    want = 40 * (2 * (0.2 - rho) ** 2 + 2 * (-0.1 - rho) ** 2) + 10 * (-0.1 - 0.2) ** 2 + w * w
    assert math.isclose(N.metric(a, b), want, rel_tol=1e-14)
    assert bits(N.metric(a, b)) == bits(N.metric(b, a))
    # just past the threshold the atan branch: a steep segment has rho near pi/2 with the sign of dy/dx
    c = [1.0100001, 5.0, -0.1]
    rho2 = math.atan((a[1] - c[1]) / (a[0] - c[0]))
    assert rho2 > 1.56
    w2 = (math.sqrt((c[0] - a[0]) ** 2 + 25.0) + 0.1) * math.sin(((0.2 + -0.1) / 2 - rho2) * 2)
    want2 = 40 * (2 * (0.2 - rho2) ** 2 + 2 * (-0.1 - rho2) ** 2) + 10 * 0.3 ** 2 + w2 * w2
    assert math.isclose(N.metric(a, c), want2, rel_tol=1e-12)
    # aligned poses one behind the other on the x axis: only the 0.1 offset is left, times sin(0) = 0
    assert N.metric([0.0, 0.0, 0.0], [5.0, 0.0, 0.0]) == 0.0


# ---- InitialCheck and FeasibilityClassifier
def test_initial_check_boundaries():
    ok = [2.0, 0.0, 0.0]
    assert N.initial_check(ok)
    for i, (lo, hi) in enumerate([(1.0, 3.0), (-1.0, 1.0), (-0.35, 0.35)]):
        for v, want in [(lo, True), (hi, True), (np.nextafter(lo, -np.inf), False), (np.nextafter(hi, np.inf), False)]:
            P = list(ok)
            P[i] = float(v)
            assert N.initial_check(P) is want, (i, v)


def test_feasibility_classifier_boundaries():
    # theta against |0.1 / dist * dist|: the test is one-sided, so any negative theta passes it
    d = 2.0
    for theta, want in [(0.05, True), (0.0999, True), (0.1001, False), (0.3, False)]:
        P = [d * math.cos(theta), d * math.sin(theta), 0.0]
        lo, hi = N.max_yawangle(math.sqrt(P[0] * P[0] + P[1] * P[1]), math.atan(P[1] / P[0]))
        P[2] = (lo + hi) / 2  # inside the yaw bounds, so only the test on theta decides
        assert lo < hi and N.feasibility_classifier(P) is want, theta
    lo, hi = N.max_yawangle(2.0, -0.3)
    mid = (lo + hi) / 2
    assert N.feasibility_classifier([2.0 * math.cos(-0.3), 2.0 * math.sin(-0.3), mid]) is (lo <= mid <= hi)
    assert lo < hi and N.feasibility_classifier([2.0 * math.cos(-0.3), 2.0 * math.sin(-0.3), mid])
    # the yaw bounds themselves
    P = [2.0, 0.0, 0.0]
    lo, hi = N.max_yawangle(2.0, 0.0)
    assert lo < 0.0 < hi
    for v, want in [(lo, True), (hi, True), (np.nextafter(lo, -np.inf), False), (np.nextafter(hi, np.inf), False)]:
        assert N.feasibility_classifier([P[0], P[1], float(v)]) is want, v


def test_max_yawangle_value_and_mirror():
    # the cubic by hand at (2, 0.05), folded left as the Julia does
    x, y = 2.0, 0.05
    p = N.YAW_LO
    want = (p[0] + p[1] * x + p[2] * y + p[3] * x * x + p[4] * x * y + p[5] * y * y + p[6] * x ** 3
            + p[7] * x * x * y + p[8] * x * y * y + p[9] * y ** 3)
    lo, hi = N.max_yawangle(x, y)
    assert math.isclose(lo, want, rel_tol=1e-13)
    # the upper bound is the lower one mirrored in y: hi(x, y) = -lo(x, -y)
    assert math.isclose(hi, -N.max_yawangle(x, -y)[0], rel_tol=1e-13)
    assert N.max_ang_ratio(2.0) == 0.05


# ---- steer
def test_steer_in_range_without_the_draw():
    start = [0.0, 0.0, 0.0]
    # 2 m ahead and 0.1 m left.  ProjectionStates rounds the cosine 0.99875 to 1.0, so the bearing reads as 0 and
    # the projection is [2.0, 0.0]: bearings come in steps of acos(0.99) = 0.14 > max_ang, so every steer that does
    # not draw ang_ratio goes straight ahead
    assert N.projection_states(start, [2.0, 0.1, 0.0]) == [2.0, 0.0, 0.0]
    new, cost, inr, drew = N.steer(start, 1.5, [2.0, 0.1, 0.0], 0.9, 0.5)
    assert inr and not drew
    assert new[0] == 2.0 and new[1] == 0.0
    lo, hi = N.max_yawangle(2.0, 0.0)
    assert math.isclose(new[2], 0.5 * (hi - lo) + lo, rel_tol=1e-12)
    assert cost == 1.5 + N.neural_cost(N.projection_states(start, new))
    # u_ratio is not read on this branch, u_yaw is
    assert N.steer(start, 1.5, [2.0, 0.1, 0.0], 0.1, 0.5)[0] == new
    assert N.steer(start, 1.5, [2.0, 0.1, 0.0], 0.9, 0.25)[0][2] != new[2]


def test_steer_in_range_with_the_draw():
    start = [0.0, 0.0, 0.0]
    # 2 m ahead and 1 m left: atan(0.5)/2.236 = 0.207 > 0.1/2.236: ang_ratio = (2u - 1) * max_ang_ratio
    new, _, inr, drew = N.steer(start, 0.0, [2.0, 1.0, 0.0], 0.75, 0.5)
    assert inr and drew
    P = N.projection_states(start, [2.0, 1.0, 0.0])
    assert P == [1.99, 1.02, 0.0]  # cos = 0.894 -> 0.89, dpsi = acos(0.89) = 0.4735, rho = 2.236
    dist = math.sqrt(P[0] * P[0] + P[1] * P[1])
    ang = (2 * 0.75 - 1) * (0.1 / dist) * dist
    assert math.isclose(new[0], dist * math.cos(ang), rel_tol=1e-12)
    assert math.isclose(new[1], dist * math.sin(ang), rel_tol=1e-12)
    assert N.steer(start, 0.0, [2.0, 1.0, 0.0], 0.25, 0.5)[0][1] < 0.0 < new[1]


def test_steer_out_of_range_both_ways():
    start = [0.0, 0.0, 0.0]
    # far ahead, nearly straight: the step is grow_max and the bearing is kept (no draw)
    new, _, inr, drew = N.steer(start, 0.0, [30.0, 0.6, 0.2], 0.9, 0.5)
    assert not inr and not drew
    assert math.isclose(math.hypot(new[0], new[1]), 3.0, rel_tol=1e-12)
    # far and to the side: the bearing is drawn within +-max_ang
    new, _, inr, drew = N.steer(start, 0.0, [10.0, 10.0, 0.2], 1.0, 0.5)
    assert not inr and drew
    assert math.isclose(math.atan2(new[1], new[0]), 0.1, rel_tol=1e-9) and math.isclose(math.hypot(*new[:2]), 3.0)
    # too close (dist < grow_min): stretched to grow_max as well
    new, _, inr, drew = N.steer(start, 0.0, [0.5, 0.0, 0.0], 0.5, 0.5)
    assert not inr and not drew and math.isclose(new[0], 3.0) and new[1] == 0.0
    # a target at the start itself: dist = 0 is not stretched, dx is clamped to 0.01 and the step is still grow_max
    new, cost, inr, drew = N.steer([1.0, 1.0, 0.0], 0.0, [1.0, 1.0, 0.3], 0.5, 0.5)
    assert not inr and not drew and math.isclose(new[0], 4.0) and math.isfinite(cost)


def test_neural_cost_of_zero_distance_is_inf_or_nan():
    assert N.neural_cost([0.0, 0.0, 0.2]) == math.inf and math.isnan(N.neural_cost([0.0, 0.0, 0.0]))
    assert N.neural_cost([3.0, 4.0, 0.5]) == 25.0 + 0.25 / 5.0


# ---- collision
def test_collision_order():
    circle = [(2.0, 0.0, 0.5)]
    a = [0.0, 0.0, 0.0]
    assert N.collision_why([], a, [2.0, 0.0, 0.0], BOUND) == 0
    # outside the bound AND kinematically bad AND inside a circle: the bound test answers
    assert N.collision_why([(-1.0, 0.0, 5.0)], a, [-1.0, 0.0, 2.0], BOUND) == 1
    # inside the bound, kinematically bad (sideways) and inside a circle: kinematics answers
    assert N.collision_why([(0.0, 2.0, 0.5)], a, [0.0, 2.0, 0.0], BOUND) == 2
    assert N.collision_why(circle, a, [2.0, 0.0, 0.0], BOUND) == 3
    # the circle test is <= on both end points
    assert N.collision_why([(2.0, 0.5, 0.5)], a, [2.0, 0.0, 0.0], BOUND) == 3
    assert N.collision_why([(2.0, 0.5, np.nextafter(0.5, 0.0))], a, [2.0, 0.0, 0.0], BOUND) == 0
    assert N.collision_why([(0.0, 0.5, 0.5)], a, [2.0, 0.0, 0.0], BOUND) == 3
    # only the second pose is tested against the bound, and the edge has a direction
    assert N.collision_why([], [-2.0, 5.0, 0.0], [0.0, 5.0, 0.0], BOUND) == 0
    assert N.collision_why([], [0.0, 5.0, 0.0], [2.0, 5.01, 0.0], BOUND) == 0
    assert N.collision_why([], [2.0, 5.01, 0.0], [0.0, 5.0, 0.0], BOUND) == 2
    assert N.collision([], [2.0, 5.01, 0.0], [0.0, 5.0, 0.0], BOUND) is True


def test_near_disk():
    assert N.near_disk(BOUND, 2) == 24.0 and N.near_disk(BOUND, 100000) == 24.0
    r = N.near_disk([0.0, 4.0, 0.0, 4.0], 400)
    assert math.isclose(r, 6 * 4 * 4 * 5 * (math.log(400.0) / 400), rel_tol=1e-14) and r < 24.0


# ---- the planner
def uniforms(seed, n_iter):
    return np.random.default_rng(seed).random((n_iter, 6))


def test_stale_snapshot_hangs_every_node_off_node_one():
    r = N.plan(BOUND, [0.0, 0.0, 0.0], [30.0, 10.0], [], uniforms(3, 64), 65, True, 0.2)
    assert r["n_nodes"] > 5 and (r["parent"][1: r["n_nodes"]] == 1).all()
    assert r["counters"][3] == 0  # the only snapshot node is the parent, which rewire skips


@functools.lru_cache(maxsize=None)
def grown():
    z = np.load(GOLD)
    obs = rrt_ref.field(z["circles"], z["count"], 53)
    return obs, N.plan(BOUND, [0.0, 0.0, 0.0], [30.0, 10.0], obs, uniforms(1, 600), 7, True, 0.2)


def test_tree_invariants_rrt_star():
    obs, r = grown()
    n, par, S, C = r["n_nodes"], r["parent"], r["state"], r["cost"]
    assert n > 300 and r["counters"][3] >= 50 and r["counters"][4] >= 100 and r["status"] == 1
    assert sum(r["counters"][:3]) + n - 1 == 600
    assert par[0] == -1 and C[0] == 0.0
    rewired_edges = 0
    for i in range(1, n):
        k, steps = i + 1, 0
        while k != 1:  # no cycles: every node reaches node 1
            k = int(par[k - 1])
            steps += 1
            assert 1 <= k <= n and steps < n
        p = int(par[i]) - 1
        a, b = [float(v) for v in S[p]], [float(v) for v in S[i]]
        assert N.collision(obs, a, b, BOUND) is False, i
        # an edge made by steer (parent older than the node) costs neural_cost(ProjectionStates(parent, node));
        # one made by rewire (parent newer) keeps what rewire charged, neural_cost(ProjectionStates(near, new)),
        # the projection taken from the child's side (:397-398).  Propagation reorders the sums: not bit-exact
        edge = N.projection_states(a, b) if p < i else N.projection_states(b, a)
        want = C[p] + N.neural_cost(edge)
        assert math.isclose(C[i], want, rel_tol=1e-9), (i, C[i], want)
        rewired_edges += p > i
    assert rewired_edges >= 20  # both kinds of edge were checked
    assert (S[n:] == 0).all() and (C[n:] == 0).all() and (par[n:] == 0).all()
    path = list(r["path_idx"])
    assert path[0] == r["best_idx"] and path[-1] == 1
    assert all(par[a - 1] == b for a, b in zip(path, path[1:]))


def test_plain_rrt_has_no_near_sets():
    _, star = grown()
    z = np.load(GOLD)
    obs = rrt_ref.field(z["circles"], z["count"], 53)
    r = N.plan(BOUND, [0.0, 0.0, 0.0], [30.0, 10.0], obs, uniforms(1, 600), 7, False, 0.2)
    assert r["counters"][3] == 0 and r["counters"][4] == 0 and r["counters"][7] == 0 and r["max_disk"] == 0
    # poses do not depend on costs or rewiring: the same uniforms grow the same poses
    assert r["n_nodes"] == star["n_nodes"] and r["state"].tobytes() == star["state"].tobytes()


# ---- the ABI side
def test_abi_signature_and_julia_ccall():
    res, args = abi.SIGNATURES["mp_rrtnh_plan"]
    proto = J.c_prototypes()["mp_rrtnh_plan"]
    # the prototype has 20 parameters, the same classes as mp_rrt_plan's
    assert res == abi.ctypes.c_int and len(args) == len(proto[1]) == 20
    assert args == abi.SIGNATURES["mp_rrt_plan"][1] and args[1] == abi.ctypes.POINTER(abi.RRTParams)
    calls = [c for c in J.jl_ccalls() if c[0] == "mp_rrtnh_plan"]
    assert len(calls) == 1 and len(calls[0][2]) == 20 and calls[0][2][1] == "Ref{RrtParams}"
    assert [J.jl_class(t) for t in calls[0][2]] == proto[1]
    assert "const mp_rrt_params_t* p" in " ".join(open(J.HDR).read().split("mp_rrtnh_plan(")[-1].split())
