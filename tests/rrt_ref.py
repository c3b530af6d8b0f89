"""CPU restatement of the sampling planner PathPlanning/RRT/src/{rrt_utils,setup,types}.jl (planRRT!, RRT and
RRT*) -- test infrastructure only, the checker of motionplanning_amd/csrc/rrt.hip (mp_rrt_plan).

Plain Python floats (IEEE double, no contraction).  sin, cos, atan and log are the CPU build of
include/mp_jlmath.h (oracle.m), sqrt is math.sqrt.  Written from the Julia; line numbers are rrt_utils.jl's.

Defined differently from the reference (include/mpgpu.h):
  * the queries on NearestNeighbors' trees (knn 1, inrange, knn 100, the final inrange) are brute force over
    the same node set, ties to the lowest index;
  * ^(0.5) of nearDisk is sqrt;
  * no 100 s wall-clock break (:391-394);
  * the node capacity is n_iter + 1 (the reference's arrays hold sampling_number nodes).
The three uniforms of iteration it are u[it] = (u_bias, u_x, u_y); u_x and u_y are ignored when the sample is
the goal (the reference draws them only when it is not).
"""
import math

import numpy as np

import oracle

NEAR_CAP = 100  # planRRT! :375-377


def round2(v):
    """round(v, digits = 2): Base's _round_digits with RoundNearest, rint(v * 100.0) / 100.0."""
    return float(np.rint(v * 100.0)) / 100.0


def sign(x):
    """Base.sign: +-1.0, and x itself (+-0.0, NaN) otherwise."""
    if x > 0.0:
        return 1.0
    if x < 0.0:
        return -1.0
    return x


def norm2(a, b):
    """norm of a 2-vector as the left fold sqrt(a^2 + b^2)."""
    return math.sqrt(a * a + b * b)


def projection_states(p1, p2):
    """ProjectionStates (:112-134): [dx, dy] of p2 seen from p1, rounded to 2 digits."""
    dx, dy = p2[0] - p1[0], p2[1] - p1[1]
    nrm = norm2(dx, dy)
    if nrm >= 0.001:
        rho = nrm
        ux, uy = dx / nrm, dy / nrm
        au = abs(ux)
        q = uy / au if au != 0.0 else (math.copysign(math.inf, uy) if uy != 0.0 else math.nan)
        dpsi = oracle.m("atan", q) * sign(ux)  # (:123) sign(0.0) = 0: a vertical segment has dpsi = 0
    else:
        rho = 0.0
        dpsi = 0.0
    return round2(rho * oracle.m("cos", dpsi)), round2(rho * oracle.m("sin", dpsi))


def neural_cost(P):
    """(:101-106)."""
    return 5.0 * math.sqrt(P[0] * P[0] + P[1] * P[1])


def steer(start, start_cost, target, grow_min, grow_max):
    """steer (:159-191) -> (new loc, new cost, took the in-range branch)."""
    P = projection_states(start, target)
    dist = math.sqrt(P[0] * P[0] + P[1] * P[1])
    if dist <= grow_max and dist >= grow_min:
        return (target[0], target[1]), start_cost + neural_cost(P), True
    new = (target[0], target[1])
    if dist > 0.001:
        k = grow_max / dist
        new = (start[0] + P[0] * k, start[1] + P[1] * k)  # FromProj2Real (:138-144)
    P = projection_states(start, new)
    if abs(P[0]) <= 0.01:
        P = (0.01, P[1])
    new = (start[0] + P[0], start[1] + P[1])
    P = projection_states(start, new)
    return new, start_cost + neural_cost(P), False


def out_of_bound(loc, b):
    """CheckWithinBoundary (:274-280): True when OUTSIDE."""
    return loc[0] < b[0] or loc[0] > b[1] or loc[1] < b[2] or loc[1] > b[3]


def collision(obstacles, p1, p2, bound):
    """collision (:282-311): the bound test on p2 only, then both end points against every circle."""
    if out_of_bound(p2, bound):
        return True
    for ox, oy, r in obstacles:
        for x, y in (p1, p2):
            ex, ey = x - ox, y - oy
            if ex * ex + ey * ey <= r * r:
                return True
    return False


def near_disk(bound, n):
    """nearDisk (:194-197); minimum([a, 50]) propagates a NaN."""
    gamma = 0.01 * (bound[1] - bound[0]) * (bound[3] - bound[2])
    a = gamma * math.sqrt(oracle.m("log", float(n)) / n)
    return a if (a < 50.0 or a != a) else 50.0


def plan(bound, start, goal, obstacles, uniforms, buffer_size, rrt_star, bias_rate, grow_min=0.0, grow_max=3.0,
         goal_tolerance=1.0):
    """planRRT! (:341-412) on given uniforms [n_iter][3].  Node indices are 1-based (row 0 of the arrays is
    node 1); parent[0] = -1."""
    bound = [float(v) for v in bound]
    obstacles = [tuple(float(v) for v in o) for o in obstacles]
    goal = (float(goal[0]), float(goal[1]))
    U = np.asarray(uniforms, np.float64).reshape(-1, 3)
    n_iter = len(U)
    cap = n_iter + 1
    X, Y, C = [0.0] * cap, [0.0] * cap, [0.0] * cap
    par = [0] * cap
    children = {1: set()}
    X[0], Y[0], par[0] = float(start[0]), float(start[1]), -1
    n, n_tree, buf = 1, 1, 0
    rejected = rewired = capped = inrange = 0
    for it in range(n_iter):
        ub, ux, uy = (float(v) for v in U[it])
        # sampleRRT (:18-39)
        if ub < bias_rate:
            s = goal
        else:
            s = (ux * (bound[1] - bound[0]) + bound[0], uy * (bound[3] - bound[2]) + bound[2])
        # knn(balltree, loc, 1) on the snapshot 1..n_tree
        mi, md = 1, None
        for i in range(n_tree):
            ex, ey = X[i] - s[0], Y[i] - s[1]
            d = ex * ex + ey * ey
            if md is None or d < md:
                mi, md = i + 1, d
        p0 = (X[mi - 1], Y[mi - 1])
        new, ncost, inr = steer(p0, C[mi - 1], s, grow_min, grow_max)
        inrange += inr
        if collision(obstacles, p0, new, bound):
            rejected += 1
            continue
        # registerNode (:326-335)
        n += 1
        buf += 1
        X[n - 1], Y[n - 1], C[n - 1], par[n - 1] = new[0], new[1], ncost, mi
        children[n] = set()
        children[mi].add(n)
        if rrt_star:
            r = near_disk(bound, n)
            cand = []
            for i in range(n_tree):
                ex, ey = X[i] - new[0], Y[i] - new[1]
                d = math.sqrt(ex * ex + ey * ey)
                if d <= r:
                    cand.append((d, i + 1))
            if len(cand) >= NEAR_CAP:
                cand = sorted(cand)[:NEAR_CAP]
                capped += 1
            # rewire (:216-238), root_idx = min_idx
            upd = []
            for _, j in cand:
                if j == mi:
                    continue
                pj = (X[j - 1], Y[j - 1])
                P = projection_states(pj, new)
                change = (C[n - 1] + neural_cost(P)) - C[j - 1]
                if change < 0 and not collision(obstacles, new, pj, bound):
                    children[par[j - 1]].discard(j)
                    children[n].add(j)
                    par[j - 1] = n
                    upd.append((j, change))
            rewired += len(upd)
            # costPropogation (:240-268): the node and its whole subtree
            for j, change in upd:
                stack = [j]
                while stack:
                    v = stack.pop()
                    C[v - 1] = C[v - 1] + change
                    stack.extend(children[v])
        if buf == buffer_size:
            n_tree, buf = n, 0
    # findBestIdx (:414-422) over all nodes
    best, bcost = 0, 0.0
    tol2 = goal_tolerance * goal_tolerance
    for i in range(n):
        ex, ey = X[i] - goal[0], Y[i] - goal[1]
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
                loc=np.array([X, Y]).T.copy(), cost=np.array(C), parent=np.array(par, np.int32),
                path_idx=np.array(path, np.int32), counters=np.array([rejected, rewired, capped, inrange], np.int32))


def field(circles, count, k):
    """Obstacle field k (1-based) of tests/golden/obstacle_fields_64.npz mapped back to the 120 m field."""
    out = []
    for x, y, r in circles[k - 1][: int(count[k - 1])]:
        out.append(((float(x) - 10.0) * 1.2, 3.0 * float(y) + 60.0, 3.0 * float(r)))
    return out
