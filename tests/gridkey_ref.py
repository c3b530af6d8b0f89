"""CPU model of the (f, seq) ordering rule of the large-grid A* / Dijkstra kernels (motionplanning_amd/csrc/
gridbig.hip) -- test infrastructure only.  astar_ref.search / gridsearch_ref.dka_search stable-sort the open list
by f every iteration and update nodes in place; here the open list is an unordered array and each pop takes the
entry with the smallest (f, seq).  seq comes from a per-search counter, handed out once an iteration's direction
loop has run:

  1. open nodes whose f strictly decreased in this iteration, in the order of their old (f, seq);
  2. then every node appended in this iteration (new, or closed and re-opened), in direction order;
  3. a node updated with an equal f (A*: tg < g can round to the same f) keeps its number.

The array is kept as the kernel keeps it: swap-remove on pop, a per-cell slot index, decrease-key in place.
rule="direction" is the obvious wrong rule (pushes and decreases numbered together in plain direction order); it
exists so that a test can show the inputs tell the two apart.

Beside the planner's outputs a search returns multi_dec (iterations with two or more in-open strict decreases) and
equal_f (updates that left f unchanged).  Plain Python floats: IEEE double, no contraction.
"""
import math

from astar_ref import DIRECTIONS


def search(grid, spos, gpos, mask, dka=False, rule="key", max_pops=None):
    """The reference search from cell spos to cell gpos over mask[iy-1][ix-1] (nonzero: free), as A* or (dka) as
    Dijkstra.  parents: Encode index -> parent Encode index (None for the start)."""
    xf2, yf2 = grid.xf * grid.xf, grid.yf * grid.yf
    spos, gpos = tuple(spos), tuple(gpos)
    s_enc = grid.encode(spos)
    pos = {s_enc: spos}
    g = {s_enc: 0.0}  # Dijkstra: f
    par = {s_enc: None}
    slot = {s_enc: 0}  # cells in the open list -> index into recs
    recs = [[0.0, 0, s_enc]]  # [f, seq, cell], unordered
    counter = 1
    pops, pop_seq, multi_dec, equal_f = 0, [], 0, 0
    out = dict(final_cost=0.0, found=False, path=[], path_length=0.0, actualpath=[], capped=False)
    cap = max_pops if max_pops is not None else 2 * (grid.nx * grid.ny + 1)
    while recs:
        if pops >= cap:
            out["capped"] = True
            break
        pops += 1
        idx = min(range(len(recs)), key=lambda i: (recs[i][0], recs[i][1]))
        cur = recs[idx][2]
        last = recs.pop()
        if idx < len(recs):  # swap-remove
            recs[idx] = last
            slot[last[2]] = idx
        del slot[cur]
        pop_seq.append(cur)
        cpos = pos[cur]
        if cpos == gpos:
            path = []
            c = cur
            while c is not None:
                path.append(pos[c])
                c = par[c]
            path.reverse()
            act = [grid.transfer(p) for p in path]
            plen = 0.0
            for i in range(len(act) - 1):
                dx, dy = act[i + 1][0] - act[i][0], act[i + 1][1] - act[i][1]
                n = math.sqrt(dx * dx + dy * dy)
                plen = n if i == 0 else plen + n
            out.update(final_cost=g[cur], found=True, path=path, actualpath=act, path_length=plen)
            break
        dec, app, events = [], [], []  # (old f, old seq, cell); cells; both in direction order
        for d in DIRECTIONS:
            npos = (cpos[0] + d[0], cpos[1] + d[1])
            n = grid.encode(npos)
            if n == 0 or not mask[npos[1] - 1, npos[0] - 1]:
                continue
            tg = g[cur] + math.sqrt(float(d[0] * d[0]) * xf2 + float(d[1] * d[1]) * yf2)
            tf = tg
            if not dka:
                hx, hy = npos[0] - gpos[0], npos[1] - gpos[1]
                tf = tg + math.sqrt(float(hx * hx) * xf2 + float(hy * hy) * yf2)
            if n in g and not tg < g[n]:  # (Dijkstra: g is f, dka_utils.jl:193)
                continue
            g[n], par[n], pos[n] = tg, cur, npos
            if n in slot:
                r = recs[slot[n]]
                if tf < r[0]:
                    dec.append((r[0], r[1], n))
                    events.append(n)
                    r[0] = tf
                else:
                    equal_f += 1
            else:
                slot[n] = len(recs)
                recs.append([tf, None, n])
                app.append(n)
                events.append(n)
        multi_dec += len(dec) >= 2
        order = events if rule == "direction" else [c for _, _, c in sorted(dec)] + app
        for c in order:
            recs[slot[c]][1] = counter
            counter += 1
    out.update(pops=pops, n_nodes=len(g), pop_seq=pop_seq, parents=par, multi_dec=multi_dec, equal_f=equal_f)
    return out
