"""CPU restatement of the grid A* planner (PathPlanning/Astar/src/{setup,types,astar_utils}.jl) and of
Hybrid A*'s astar_heuristic (PathPlanning/HybridAstar/src/hybrid_astar_utils.jl:375-387, :419) -- test
infrastructure only, the checker of motionplanning_amd/csrc/astar.hip and of mp_ha_plan_astar.

Plain Python floats (IEEE double, no contraction); the two BLAS-dispatched products of the block
obstacles (GetRectanglePts through the oracle's or_ha_rect_pts, the SAT projections as or_blas.h's
blv_t2) round as the reference's OpenBLAS does.  Python 3.10 has no math.fma: the exact product-sum is
formed in rationals and rounded once.
"""
import math
from fractions import Fraction

import numpy as np

import oracle
from motionplanning_amd.abi import ptr

# FindNewNode's directions as written (astar_utils.jl:192): two duplicates, no (-1, +1)
DIRECTIONS = [(-1, 0), (-1, -1), (-1, -1), (1, -1), (1, 0), (1, 1), (0, -1), (1, -1), (0, 1)]
EPS = 1e-1  # checkObsSafety's epsilon (:267)
HA_GRID = 11  # astar_heuristic's mapbound [11, 11] (hybrid_astar_utils.jl:379)


def fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def blv_t2(a0, x0, a1, x1):
    """dgemv 'T' with two rows (oracle/or_blas.h): fma(A[0,j], x_0, A[1,j]*x_1)."""
    return fma(a0, x0, a1 * x1)


def sat_dps(base, other, e):
    """transpose(pts .- bg_pt) * normal_vec for edge e of base (utils.jl:41-49)."""
    bx, by = base[e]
    vx, vy = base[e + 1][0] - bx, base[e + 1][1] - by
    nx, ny = -vy, vx
    db = [blv_t2(p[0] - bx, nx, p[1] - by, ny) for p in base]
    dq = [blv_t2(p[0] - bx, nx, p[1] - by, ny) for p in other]
    return db, dq


def sat(base, other):
    """SeparatingAxisTheorem (utils.jl:37-62): True when an edge normal of base separates."""
    for e in range(len(base) - 1):
        db, dq = sat_dps(base, other, e)
        if max(dq) <= min(db) or max(db) <= min(dq):
            return True
    return False


def convex_free(p1, p2):
    """ConvexCollision (utils.jl:64-74): the && of both SAT directions."""
    return sat(p1, p2) and sat(p2, p1)


def wall_pts(block):
    """GetRectanglePts (utils.jl:14-25) as the oracle computes it: 5 points (x, y)."""
    blk = np.ascontiguousarray(block, np.float64)
    out = np.zeros(10)
    oracle._ha().or_ha_rect_pts(ptr(blk), ptr(out))
    return [(float(out[2 * j]), float(out[2 * j + 1])) for j in range(5)]


def mypts(tx, ty):
    """checkObsSafety's 2x4 test shape (:268): first and last point coincide, there is no y - eps."""
    return [(tx, ty + EPS), (tx - EPS, ty), (tx + EPS, ty), (tx, ty + EPS)]


class Grid:
    """defineAstar (setup.jl:3-24): bound = [xmin, xmax, ymin, ymax], mapbound = [nx, ny]."""

    def __init__(self, bound, nx, ny):
        self.b = [float(v) for v in bound]
        self.nx, self.ny = int(nx), int(ny)
        self.xf = (self.b[1] - self.b[0]) / (float(nx) - 1)
        self.yf = (self.b[3] - self.b[2]) / (float(ny) - 1)

    def cell(self, real):
        """starting_pos / ending_pos (setup.jl:17-18), 1-based."""
        return (int(math.floor((float(real[0]) - self.b[0]) / self.xf + 1)),
                int(math.floor((float(real[1]) - self.b[2]) / self.yf + 1)))

    def encode(self, pos):
        """Encode (astar_utils.jl:176-188): 0 off the grid."""
        x, y = pos
        if x < 1 or x > self.nx or y < 1 or y > self.ny:
            return 0
        return (y - 1) * self.nx + x

    def transfer(self, pos):
        """TransferCoordinate (:237-240)."""
        return ((pos[0] - 1.0) * self.xf + self.b[0], (pos[1] - 1.0) * self.yf + self.b[2])


def free_mask(grid, obstacles, kind):
    """checkObsSafety (:253-279) for every cell: mask[iy-1][ix-1].  An empty obstacle list (where the
    reference indexes obstacle_list[1]) is all free."""
    mask = np.ones((grid.ny, grid.nx), np.uint8)
    obstacles = [list(map(float, o)) for o in obstacles]
    if not obstacles:
        return mask
    walls = [wall_pts(o) for o in obstacles] if kind == 5 else None
    for iy in range(1, grid.ny + 1):
        for ix in range(1, grid.nx + 1):
            tx, ty = grid.transfer((ix, iy))
            ok = True
            if kind == 3:
                for o in obstacles:
                    if (tx - o[0]) * (tx - o[0]) + (ty - o[1]) * (ty - o[1]) < o[2] * o[2]:
                        ok = False
                        break
            else:
                mp = mypts(tx, ty)
                for w in walls:
                    if not convex_free(w, mp):
                        ok = False
                        break
            mask[iy - 1, ix - 1] = ok
    return mask


def search(grid, spos, gpos, mask, max_pops=None):
    """planAstar! + FindNewNode (:83-141, :190-235) from cell spos to cell gpos.  Start == goal (the
    reference's KeyError(nothing) at :110) is cost 0, found."""
    xf2, yf2 = grid.xf * grid.xf, grid.yf * grid.yf
    nodes = {}  # Encode index -> [parent, pos, g, f]
    start = [None, tuple(spos), 0.0, 0.0]
    nodes[grid.encode(spos)] = start
    open_list = [start]
    pops, pop_seq = 0, []
    out = dict(final_cost=0.0, found=False, path=[], path_length=0.0, actualpath=[], capped=False)
    cap = max_pops if max_pops is not None else 2 * (grid.nx * grid.ny + 1)
    while open_list:
        if pops >= cap:
            out["capped"] = True
            break
        pops += 1
        open_list.sort(key=lambda n: n[3])  # stable, as sort! on the open list
        cur = open_list.pop(0)
        cidx = grid.encode(cur[1])
        pop_seq.append(cidx)
        if cur[1] == tuple(gpos):
            out["final_cost"] = cur[2]
            out["found"] = True
            path = [cur[1]]
            while cur[0] is not None:
                cur = nodes[cur[0]]
                path.append(cur[1])
            path.reverse()
            act = [grid.transfer(p) for p in path]
            plen = 0.0
            for i in range(len(act) - 1):
                dx, dy = act[i + 1][0] - act[i][0], act[i + 1][1] - act[i][1]
                n = math.sqrt(dx * dx + dy * dy)
                plen = n if i == 0 else plen + n
            out.update(path=path, actualpath=act, path_length=plen)
            break
        for d in DIRECTIONS:
            npos = (cur[1][0] + d[0], cur[1][1] + d[1])
            nidx = grid.encode(npos)
            if nidx == 0 or not mask[npos[1] - 1, npos[0] - 1]:
                continue
            ddx, ddy = npos[0] - cur[1][0], npos[1] - cur[1][1]
            tg = cur[2] + math.sqrt(float(ddx * ddx) * xf2 + float(ddy * ddy) * yf2)
            gx, gy = npos[0] - gpos[0], npos[1] - gpos[1]
            th = math.sqrt(float(gx * gx) * xf2 + float(gy * gy) * yf2)
            tf = tg + th
            upd = False
            if nidx in nodes:
                nd = nodes[nidx]
                if tg < nd[2]:
                    nd[2], nd[3], nd[0] = tg, tf, cidx
                    upd = True
            else:
                nd = [cidx, npos, tg, tf]
                nodes[nidx] = nd
                upd = True
            if upd and not any(o is nd for o in open_list):
                open_list.append(nd)
    out.update(pops=pops, n_nodes=len(nodes), pop_seq=pop_seq)
    return out


def plan(bound, nx, ny, start_real, goal_real, obstacles, kind):
    """defineAstar + defineAstarobs! + planAstar!."""
    g = Grid(bound, nx, ny)
    return search(g, g.cell(start_real), g.cell(goal_real), free_mask(g, obstacles, kind))


# ------------------------------------------------------------------ Hybrid A*
def ha_grid(p):
    return Grid([p.stbound[0], p.stbound[1], p.stbound[2], p.stbound[3]], HA_GRID, HA_GRID)


def ha_table(p, goal, walls):
    """astar_heuristic (hybrid_astar_utils.jl:375-387) for a state in each of the 11 x 11 cells:
    table[(iy-1)*11 + (ix-1)], plus the mask and the per-cell search records."""
    g = ha_grid(p)
    mask = free_mask(g, [list(w) for w in np.asarray(walls, np.float64).reshape(-1, 5)], 5)
    gpos = g.cell(goal)
    tab = np.zeros(HA_GRID * HA_GRID)
    recs = []
    for iy in range(1, HA_GRID + 1):
        for ix in range(1, HA_GRID + 1):
            r = search(g, (ix, iy), gpos, mask)
            tab[(iy - 1) * HA_GRID + ix - 1] = r["final_cost"]
            recs.append(r)
    return tab, mask, recs


def jl_max(a, b):
    """Julia max for Float64: NaN propagates."""
    if a != a:
        return a
    if b != b:
        return b
    return max(a, b)


def ha_plan(p, start, goal, walls, sc, pc, table=None):
    """planHybridAstar! (:235-296) + FindNewNode (:391-447) around the oracle's ha_expand /
    ha_rs_connect; temp_h = max(rs_heuristic, table[cell]) with a table, max(rs_heuristic, 0) without."""
    g = ha_grid(p)
    gcell = g.encode(g.cell(goal))
    start = np.asarray(start, np.float64)
    s0 = dict(parent=None, st=start.copy(), index=oracle.ha_encode(p, start), g=0.0, h=0.0, f=0.0)
    nodes = {s0["index"]: s0}
    open_list = [s0]
    res = dict(found=False, pops=0, pop_seq=[], states=np.zeros((0, 3)), rs_path=np.zeros((0, 3)), raised=0,
               lookups=0, goal_cell_lookups=0)
    while open_list and res["pops"] < p.max_pops:
        res["pops"] += 1
        open_list.sort(key=lambda n: n["f"])
        cur = open_list.pop(0)
        res["pop_seq"].append(cur["index"])
        ok, path = oracle.ha_rs_connect(p, cur["st"], goal, walls)
        if ok:
            states = [cur["st"]]
            c = cur
            while c["parent"] is not None and c["index"] != s0["index"]:
                c = nodes[c["parent"]]
                states.append(c["st"])
            res.update(found=True, states=np.array(states), rs_path=path)
            break
        nbs, idx, fr, h = oracle.ha_expand(p, cur["st"], goal, walls, sc, pc)
        for k in range(p.n_prim):
            if idx[k] == 0 or not fr[k]:
                continue
            tg = cur["g"] + p.expand_time
            ah = 0.0
            if table is not None:
                cx, cy = g.cell(nbs[k])
                ah = float(table[(cy - 1) * HA_GRID + cx - 1])
                res["lookups"] += 1
                res["goal_cell_lookups"] += g.encode((cx, cy)) == gcell
                res["raised"] += ah > h[k]
            th = jl_max(float(h[k]), ah)
            tf = tg + th
            ix = int(idx[k])
            upd = False
            if ix in nodes:
                nd = nodes[ix]
                if tg < nd["g"]:
                    nd.update(g=tg, h=th, f=tf, parent=cur["index"])
                    upd = True
            else:
                nd = dict(parent=cur["index"], st=nbs[k].copy(), index=ix, g=tg, h=th, f=tf)
                nodes[ix] = nd
                upd = True
            if upd and not any(o is nd for o in open_list):
                open_list.append(nd)
    res["n_nodes"] = len(nodes)
    res["pop_seq"] = np.array(res["pop_seq"], np.int64)
    return res
