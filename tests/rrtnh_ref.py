"""CPU restatement of the car-like sampling planner PathPlanning/RRTNonholonomic/src/{rrt_utils,setup,types}.jl
(planRRT!, RRT and RRT* over poses [x, y, psi]) -- test infrastructure only, the checker of
motionplanning_amd/csrc/rrtnh.hip (mp_rrtnh_plan).

Plain Python floats (IEEE double, no contraction).  acos, atan, sin, cos and log are the CPU build of
include/mp_jlmath.h (oracle.m), sqrt is math.sqrt, fma is exact.  Written from the Julia; line numbers are
rrt_utils.jl's unless types.jl is named.

Defined differently from the reference (include/mpgpu.h):
  * the tree queries (knn 1, inrange, knn 30 on the BallTree) are brute force over the snapshot under MyMetrics
    (types.jl:9-23): the nearest node is the minimum, the lowest index on ties; the near set is every snapshot
    node with metric <= r, and from 30 such nodes on the 30 smallest by (metric, index).  MyMetrics is no metric,
    so the BallTree's pruning has no defined answer to restate;
  * the final inrange on the KDTree is brute force on dx*dx + dy*dy <= goal_tolerance^2;
  * no 100 s wall-clock break (:563-566);
  * the node capacity is n_iter + 1.
Conventions not pinned against a Julia run: round(v, digits = d) is rint(v * 10^d) / 10^d; x^2 and x^3 are x*x
and x*x*x; n-ary + and * fold left; norm of a 2-vector is sqrt(v1*v1 + v2*v2); dot of two 2-vectors is
fma(x1, y1, x0*y0) (oracle/or_blas.h ddot).
The six uniforms of iteration it are u[it] = (u_bias, u_x, u_y, u_psi, u_ratio, u_yaw); u_x and u_y are ignored
when the sample is the goal and u_ratio when steer does not draw ang_ratio (the reference draws them only then).
"""
import math
from fractions import Fraction

import numpy as np

import oracle

NEAR_CAP = 30      # planRRT! :547-549
RADIUS_CAP = 24.0  # nearDisk :372
MAX_ANG = 0.1      # get_max_ang_ratio :116
PI = math.pi       # Float64(pi)

# get_max_yawangle (:120-145): p00 p10 p01 p20 p11 p02 p30 p21 p12 p03 of the lower and the upper bound
YAW_LO = (-0.03911, 0.05831, 0.1148, -0.04344, 0.4135, -0.05552, 0.005515, -0.05701, 0.1892, -0.1725)
YAW_HI = (0.03911, -0.05831, 0.1148, 0.04344, 0.4135, 0.05552, -0.005515, -0.05701, -0.1892, -0.1725)


def fma(a, b, c):
    """fma(a, b, c) with one rounding."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    v = Fraction(a) * Fraction(b) + Fraction(c)
    if v == 0:
        return a * b + c  # the sign of an exact zero sum is that of the rounded expression
    return float(v)


def div(a, b):
    """IEEE a / b (Python raises on a zero divisor)."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def round_digits(v, d):
    """round(v, digits = d): Base's _round_digits with RoundNearest, rint(v * 10^d) / 10^d."""
    s = 10.0 ** d
    return float(np.rint(v * s)) / s


def sign(x):
    """Base.sign: +-1.0, and x itself (+-0.0, NaN) otherwise."""
    if x > 0.0:
        return 1.0
    if x < 0.0:
        return -1.0
    return x


def metric(a, b):
    """MyMetrics (types.jl:9-23) of two poses."""
    ex, ey = b[0] - a[0], b[1] - a[1]
    r = math.sqrt(ex * ex + ey * ey) + 0.1
    fx = a[0] - b[0]
    if abs(fx) <= 0.01:
        rho = PI / 2
    else:
        rho = oracle.m("atan", (a[1] - b[1]) / fx)
    d = b[2] - a[2]
    e1, e2 = a[2] - rho, b[2] - rho
    w = r * oracle.m("sin", ((a[2] + b[2]) / 2 - rho) * 2)
    return (40 * (2 * (e1 * e1) + 2 * (e2 * e2)) + 10 * (d * d)) + w * w


def projection_states(n1, n2):
    """ProjectionStates (:208-238): [dx, dy, dpsi_head] of pose n2 seen from pose n1."""
    c, s = oracle.m("cos", n1[2]), oracle.m("sin", n1[2])  # h1 = euler2Rot(psi1)[1:2, 1]
    dx, dy = n2[0] - n1[0], n2[1] - n1[1]
    nrm = math.sqrt(dx * dx + dy * dy)
    if nrm >= 0.001:
        rho = nrm
        ux, uy = dx / nrm, dy / nrm
        sg = c * uy - s * ux
        den = math.sqrt(ux * ux + uy * uy) * math.sqrt(c * c + s * s)
        dpsi = oracle.m("acos", round_digits(div(fma(uy, s, ux * c), den), 2)) * sign(sg)
    else:
        rho = 0.0
        dpsi = 0.0
    return [round_digits(rho * oracle.m("cos", dpsi), 2), round_digits(rho * oracle.m("sin", dpsi), 2),
            round_digits(n2[2] - n1[2], 3)]


def neural_cost(P):
    """(:106-112); a zero distance gives Inf or NaN."""
    dist = math.sqrt(P[0] * P[0] + P[1] * P[1])
    return 5 * dist + div(P[2] * P[2], dist)


def max_ang_ratio(dist):
    """get_max_ang_ratio (:115-118)."""
    return div(MAX_ANG, dist)


def _cubic(p, x, y):
    p00, p10, p01, p20, p11, p02, p30, p21, p12, p03 = p
    return (((((((((p00 + p10 * x) + p01 * y) + p20 * (x * x)) + p11 * x * y) + p02 * (y * y)) + p30 * (x * x * x))
              + p21 * (x * x) * y) + p12 * x * (y * y)) + p03 * (y * y * y))


def max_yawangle(x, y):
    """get_max_yawangle (:120-145) -> (lower, upper)."""
    return _cubic(YAW_LO, x, y), _cubic(YAW_HI, x, y)


def initial_check(P):
    """InitialCheck (:240-258)."""
    if P[0] < 1.0 or P[0] > 3.0:
        return False
    if P[1] < -1.0 or P[1] > 1.0:
        return False
    if P[2] < -0.35 or P[2] > 0.35:
        return False
    return True


def feasibility_classifier(P):
    """FeasibilityClassifier (:154-175); the test on theta is one-sided, as written there."""
    dist = math.sqrt(P[0] * P[0] + P[1] * P[1])
    theta = oracle.m("atan", div(P[1], P[0]))
    if theta > abs(max_ang_ratio(dist) * dist):
        return False
    lo, hi = max_yawangle(dist, theta)
    if P[2] < lo or P[2] > hi:
        return False
    return True


def from_proj_to_real(n1, P):
    """FromProj2Real (:261-277): h1 = (cos, sin), l1 = cross([0, 0, 1], h1) = (0*0 - 1*sin, 1*cos - 0*0)."""
    c, s = oracle.m("cos", n1[2]), oracle.m("sin", n1[2])
    l1x, l1y = 0.0 - s, c - 0.0
    x = n1[0] + c * P[0]
    y = n1[1] + s * P[0]
    x = x + l1x * P[1]
    y = y + l1y * P[1]
    return [x, y, n1[2] + P[2]]


def decide_proj(dist, ang_ratio, u_yaw):
    """DistToDeltaXY (:147-152) and decide_proj (:282-290)."""
    ang = ang_ratio * dist
    lo, hi = max_yawangle(dist, ang_ratio * dist)
    return [dist * oracle.m("cos", ang), dist * oracle.m("sin", ang), u_yaw * (hi - lo) + lo]


def steer(start, start_cost, target, u_ratio, u_yaw, grow_min=1.0, grow_max=3.0):
    """steer (:292-365) -> (new pose, new cost, took the in-range branch, drew ang_ratio)."""
    new = list(target)
    P = projection_states(start, new)
    dist = math.sqrt(P[0] * P[0] + P[1] * P[1])
    inr = dist <= grow_max and dist >= grow_min
    if inr:
        d = dist
    else:
        d = grow_max  # adjustdist (:331)
        if dist > 0.001:
            k = d / dist
            new = from_proj_to_real(start, [P[0] * k, P[1] * k, P[2]])
        P = projection_states(start, new)
    mar = max_ang_ratio(d)
    if abs(P[0]) <= 0.01:
        P[0] = 0.01
    dpsi = oracle.m("atan", P[1] / P[0])
    drew = div(abs(dpsi), d) > mar
    if drew:
        ang_ratio = (2 * u_ratio - 1) * mar
    else:
        ang_ratio = div(dpsi, d)
    new = from_proj_to_real(start, decide_proj(d, ang_ratio, u_yaw))
    P = projection_states(start, new)
    return new, start_cost + neural_cost(P), inr, drew


def out_of_bound(loc, b):
    """CheckWithinBoundary (:450-456): True when OUTSIDE."""
    return loc[0] < b[0] or loc[0] > b[1] or loc[1] < b[2] or loc[1] > b[3]


def collision_why(obstacles, n1, n2, bound):
    """collision (:458-498) -> 0 free, 1 the bound test on n2, 2 kinematics of the edge n1 -> n2, 3 a circle."""
    if out_of_bound(n2, bound):
        return 1
    P = projection_states(n1, n2)
    if not (initial_check(P) and feasibility_classifier(P)):
        return 2
    for ox, oy, r in obstacles:
        for q in (n1, n2):
            ex, ey = q[0] - ox, q[1] - oy
            if ex * ex + ey * ey <= r * r:
                return 3
    return 0


def collision(obstacles, n1, n2, bound):
    return collision_why(obstacles, n1, n2, bound) != 0


def near_disk(bound, n):
    """nearDisk (:370-373); minimum([a, 24]) propagates a NaN."""
    gamma = 6 * (bound[1] - bound[0]) * (bound[3] - bound[2]) * 5
    a = gamma * (oracle.m("log", float(n)) / n)
    return a if (a < RADIUS_CAP or a != a) else RADIUS_CAP


def plan(bound, start, goal, obstacles, uniforms, buffer_size, rrt_star, bias_rate, grow_min=1.0, grow_max=3.0,
         goal_tolerance=1.0):
    """planRRT! (:528-583) on given uniforms [n_iter][6].  Node indices are 1-based (row 0 of the arrays is node
    1); parent[0] = -1.  counters: samples rejected by the bound test, by kinematics, by a circle; rewired edges;
    near sets that reached the cap; steers on the in-range branch; steers that drew ang_ratio; near sets whose
    radius was below 24.  max_disk is the largest in-disk set of any iteration."""
    bound = [float(v) for v in bound]
    obstacles = [tuple(float(v) for v in o) for o in obstacles]
    goal = (float(goal[0]), float(goal[1]))
    U = np.asarray(uniforms, np.float64).reshape(-1, 6)
    n_iter = len(U)
    cap = n_iter + 1
    S = [[0.0, 0.0, 0.0] for _ in range(cap)]
    C = [0.0] * cap
    par = [0] * cap
    children = {1: set()}
    S[0], par[0] = [float(start[0]), float(start[1]), float(start[2])], -1
    n, n_tree, buf = 1, 1, 0
    cnt = [0] * 8
    max_disk = 0
    for it in range(n_iter):
        ub, ux, uy, up, ur, uw = (float(v) for v in U[it])
        # sampleRRT (:18-44)
        psi = (up - 0.5) * 2 * PI
        if ub < bias_rate:
            s = [goal[0], goal[1], psi]
        else:
            s = [ux * (bound[1] - bound[0]) + bound[0], uy * (bound[3] - bound[2]) + bound[2], psi]
        # knn(balltree, pose, 1) (:536) on the snapshot 1..n_tree
        mi, md = 1, math.inf  # no value compares (NaN): node 1
        for i in range(n_tree):
            d = metric(S[i], s)
            if d < md:
                mi, md = i + 1, d
        p0 = S[mi - 1]
        new, ncost, inr, drew = steer(p0, C[mi - 1], s, ur, uw, grow_min, grow_max)
        cnt[5] += inr
        cnt[6] += drew
        why = collision_why(obstacles, p0, new, bound)
        if why:
            cnt[why - 1] += 1
            continue
        # registerNode (:513-522)
        n += 1
        buf += 1
        S[n - 1], C[n - 1], par[n - 1] = new, ncost, mi
        children[n] = set()
        children[mi].add(n)
        if rrt_star:
            r = near_disk(bound, n)
            cnt[7] += r < RADIUS_CAP
            cand = []
            for i in range(n_tree):
                d = metric(S[i], new)
                if d <= r:
                    cand.append((d, i + 1))
            max_disk = max(max_disk, len(cand))
            if len(cand) >= NEAR_CAP:
                cand = sorted(cand)[:NEAR_CAP]
                cnt[4] += 1
            # rewire (:392-414), root_idx = min_idx
            upd = []
            for _, j in cand:
                if j == mi:
                    continue
                pj = S[j - 1]
                change = (C[n - 1] + neural_cost(projection_states(pj, new))) - C[j - 1]
                if change < 0 and not collision(obstacles, new, pj, bound):
                    children[par[j - 1]].discard(j)
                    children[n].add(j)
                    par[j - 1] = n
                    upd.append((j, change))
            cnt[3] += len(upd)
            # costPropogation (:416-431): the node and its whole subtree
            for j, change in upd:
                stack = [j]
                while stack:
                    v = stack.pop()
                    C[v - 1] = C[v - 1] + change
                    stack.extend(children[v])
        if buf == buffer_size:  # BallTree rebuild (:558-561)
            n_tree, buf = n, 0
    # findBestIdx (:585-593) over all nodes
    best, bcost = 0, 0.0
    tol2 = goal_tolerance * goal_tolerance
    for i in range(n):
        ex, ey = S[i][0] - goal[0], S[i][1] - goal[1]
        if ex * ex + ey * ey <= tol2 and (best == 0 or C[i] < bcost):
            best, bcost = i + 1, C[i]
    path = []
    if best:
        k = best
        path.append(k)
        while k != 1:
            k = par[k - 1]
            path.append(k)
    return dict(n_nodes=n, status=1 if best else 0, best_idx=best, best_cost=bcost if best else 0.0,
                state=np.array(S, np.float64).reshape(cap, 3), cost=np.array(C), parent=np.array(par, np.int32),
                path_idx=np.array(path, np.int32), counters=np.array(cnt, np.int32), max_disk=max_disk)
