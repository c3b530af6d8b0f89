"""CPU restatement of the Dijkstra and breadth-first grid planners (PathPlanning/Dijkstra/src/{setup,types,
dka_utils}.jl, PathPlanning/BreadthFirst/src/{setup,types,bfs_utils}.jl) -- test infrastructure only, the checker
of mp_dka_plan and mp_bfs_plan (motionplanning_amd/csrc/astar.hip).

Both planners share defineAstar's grid (Dijkstra/src/setup.jl:16-19 and BreadthFirst/src/setup.jl:16-19 are
Astar/src/setup.jl:15-18 word for word) and the circle test of checkObsSafety (dka_utils.jl:233-243,
bfs_utils.jl:179-189: strict <, the first hit breaks; an empty list runs 1:0 and leaves every cell free), so Grid
and free_mask(..., 3) come from astar_ref.  Plain Python floats: IEEE double, no contraction.
"""
import math

from astar_ref import Grid, free_mask

# FindNewNode's directions as written: Dijkstra keeps A*'s nine entries (dka_utils.jl:177: two repeats, no
# (-1, +1)), BFS the four axis moves (bfs_utils.jl:140)
DKA_DIRECTIONS = [(-1, 0), (-1, -1), (-1, -1), (1, -1), (1, 0), (1, 1), (0, -1), (1, -1), (0, 1)]
BFS_DIRECTIONS = [(-1, 0), (1, 0), (0, -1), (0, 1)]


def _retrieve(grid, nodes, cur):
    """The goal branch of planDKA! / planBFS! (dka_utils.jl:92-112, bfs_utils.jl:24-43): the parent chain,
    reversed, its TransferCoordinate rows and sum(norm(row[i+1] - row[i])) as a left fold (dka_utils.jl:112;
    BFSResult has no path_length, the same fold is an extension there)."""
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
    return dict(path=path, actualpath=act, path_length=plen)


def dka_search(grid, spos, gpos, mask, max_pops=None):
    """planDKA! (dka_utils.jl:69-126) + FindNewNode (:175-215) from cell spos to cell gpos.  Start == goal (the
    reference indexes nodes_collection[nothing] at :93) is found, cost 0, a one-cell path."""
    xf2, yf2 = grid.xf * grid.xf, grid.yf * grid.yf
    nodes = {}  # Encode index -> [parent, pos, f]
    start = [None, tuple(spos), 0.0]  # DKANode(nothing, starting_pos, 0) (setup.jl:20)
    nodes[grid.encode(spos)] = start  # setup.jl:23
    open_list = [start]  # :71
    pops, pop_seq, max_open = 0, [], 1
    out = dict(final_cost=0.0, found=False, path=[], path_length=0.0, actualpath=[], capped=False)
    cap = max_pops if max_pops is not None else 2 * (grid.nx * grid.ny + 1)
    while open_list:  # :73
        if pops >= cap:
            out["capped"] = True
            break
        pops += 1  # :74
        max_open = max(max_open, len(open_list))
        open_list.sort(key=lambda n: n[2])  # :75, stable, isless on f (types.jl:9)
        cur = open_list.pop(0)  # :76
        cidx = grid.encode(cur[1])
        pop_seq.append(cidx)
        if cur[1] == tuple(gpos):  # :91
            out.update(final_cost=cur[2], found=True, **_retrieve(grid, nodes, cur))
            break
        for d in DKA_DIRECTIONS:  # :179
            npos = (cur[1][0] + d[0], cur[1][1] + d[1])
            nidx = grid.encode(npos)
            if nidx == 0 or not mask[npos[1] - 1, npos[0] - 1]:  # :185-188
                continue
            ddx, ddy = npos[0] - cur[1][0], npos[1] - cur[1][1]
            tf = cur[2] + math.sqrt(float(ddx * ddx) * xf2 + float(ddy * ddy) * yf2)  # :189
            upd = False
            if nidx in nodes:  # :191
                nd = nodes[nidx]
                if tf < nd[2]:  # :193
                    nd[2], nd[0] = tf, cidx
                    upd = True
            else:
                nd = [cidx, npos, tf]  # :201
                nodes[nidx] = nd
                upd = True
            if upd and not any(o is nd for o in open_list):  # :206-209, InOpen :130-137
                open_list.append(nd)
    out.update(pops=pops, n_nodes=len(nodes), pop_seq=pop_seq, max_open=max_open)
    return out


def bfs_search(grid, spos, gpos, mask):
    """planBFS! (bfs_utils.jl:1-59) + FindNewNode (:137-161) from cell spos to cell gpos.  Start == goal (the
    reference indexes nodes_collection[nothing] at :25) is found, a one-cell path.  Beside the planner's outputs:
    queue (every node in the order it entered the open list, as Encode indices), depth (the depth of each of
    them) and queue_left / queue_left_depth (the open list at the goal pop)."""
    nodes = {}  # Encode index -> [parent, pos, depth]
    start = [None, tuple(spos), 0]  # BFSNode(nothing, starting_pos) (setup.jl:20)
    nodes[grid.encode(spos)] = start  # setup.jl:21
    open_list = [start]  # :3
    queue = [start]
    pops, pop_seq = 0, []
    out = dict(found=False, path=[], path_length=0.0, actualpath=[], queue_left=[], queue_left_depth=[])
    while open_list:  # :6
        pops += 1  # :8
        cur = open_list.pop(0)  # :9
        cidx = grid.encode(cur[1])
        pop_seq.append(cidx)
        if cur[1] == tuple(gpos):  # :23
            out.update(found=True, goal_depth=cur[2], queue_left=[grid.encode(n[1]) for n in open_list],
                       queue_left_depth=[n[2] for n in open_list], **_retrieve(grid, nodes, cur))
            break
        for d in BFS_DIRECTIONS:  # :141
            npos = (cur[1][0] + d[0], cur[1][1] + d[1])
            nidx = grid.encode(npos)
            if nidx == 0 or not mask[npos[1] - 1, npos[0] - 1]:  # :147-150
                continue
            if nidx not in nodes:  # :152
                nd = [cidx, npos, cur[2] + 1]
                nodes[nidx] = nd
                open_list.append(nd)  # :155
                queue.append(nd)
    out.update(pops=pops, n_nodes=len(nodes), pop_seq=pop_seq, queue=[grid.encode(n[1]) for n in queue],
               depth=[n[2] for n in queue])
    return out


def plan_dka(bound, nx, ny, start_real, goal_real, circles):
    """defineDKA + defineDKAobs! + planDKA!."""
    g = Grid(bound, nx, ny)
    return dka_search(g, g.cell(start_real), g.cell(goal_real), free_mask(g, circles, 3))


def plan_bfs(bound, nx, ny, start_real, goal_real, circles):
    """defineBFS + defineBFSobs! + planBFS!."""
    g = Grid(bound, nx, ny)
    return bfs_search(g, g.cell(start_real), g.cell(goal_real), free_mask(g, circles, 3))
