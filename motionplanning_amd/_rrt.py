"""What rrt.py and rrt_nonholonomic.py share: the batch's settings check and its packing into the arrays
mp_rrt_plan / mp_rrtnh_plan take (pack_scenes, no library call), the call itself and the result fields (run)."""
import time

import numpy as np

from .abi import RRTParams, f64, ptr


def defineRRTobs_(rrt, obstacle_list):
    """defineRRTobs! (setup.jl): circles [x, y, r]."""
    rrt.s.obstacle_list = [[float(v) for v in o] for o in obstacle_list]


def _settings_key(s):
    return (s.sampling_number, s.buffer_size, s.rrt_star, s.bias_rate, tuple(s.grow_dist), s.goal_tolerance)


def pack_scenes(searchers, start_rows, n_uni, uniforms):
    """(params, bound, start, goal, count, obs, uni) of B searchers sharing their settings; start_rows: a start
    row per searcher; uniforms: [B][n_iter][n_uni], or None to draw them per searcher from
    ``numpy.random.default_rng(searcher.s.seed)``."""
    s0 = searchers[0].s
    if any(_settings_key(a.s) != _settings_key(s0) for a in searchers):
        raise ValueError("plan_batch: every searcher needs the same sampling_number, buffer_size, rrt_star, "
                         "bias_rate, grow_dist and goal_tolerance")
    B, n_iter = len(searchers), int(s0.sampling_number)
    p = RRTParams(n_iter=n_iter, buffer_size=int(s0.buffer_size), rrt_star=int(s0.rrt_star), reserved=0,
                  bias_rate=float(s0.bias_rate), grow_min=float(s0.grow_dist[0]), grow_max=float(s0.grow_dist[1]),
                  goal_tolerance=float(s0.goal_tolerance))
    if uniforms is None:
        uniforms = [np.random.default_rng(a.s.seed).random((max(n_iter, 0), n_uni)) for a in searchers]
    uni = f64(uniforms).reshape(B, max(n_iter, 0), n_uni)
    bound = f64([a.s.BoundPosition for a in searchers])
    goal = f64([a.s.ending_position for a in searchers])
    # obstacle lists padded to the longest; obs_count tells the library how many rows of each count
    count = np.array([len(a.s.obstacle_list) for a in searchers], np.int32)
    obs = np.zeros((B, int(count.max()), 3))
    for b, a in enumerate(searchers):
        if count[b]:
            obs[b, : count[b]] = f64(a.s.obstacle_list).reshape(-1, 3)
    return p, bound, f64(start_rows), goal, count, obs, uni


def run(ctx, plan, packed, searchers, result, state_field, n_counters):
    """One call of plan (mp_rrt_plan / mp_rrtnh_plan) for the packed batch; every searcher gets a new result() with
    its tree (the nodes in state_field), counters and, if solved, path."""
    p, bound, start, goal, count, obs, uni = packed
    B, cap, n_obs = len(searchers), max(p.n_iter + 1, 1), obs.shape[1]
    nn, status, best, pn = (np.zeros(B, np.int32) for _ in range(4))
    bcost = np.zeros(B)
    state, cost = np.zeros((B, cap, start.shape[1])), np.zeros((B, cap))
    parent, path = np.zeros((B, cap), np.int32), np.zeros((B, cap), np.int32)
    counters = np.zeros((B, n_counters), np.int32)
    t0 = time.time()
    ctx.check(plan(ctx.handle, p, B, ptr(bound), ptr(start), ptr(goal), n_obs, ptr(count), ptr(obs) if n_obs else None,
                   ptr(uni), ptr(nn), ptr(status), ptr(best), ptr(bcost), ptr(state), ptr(cost), ptr(parent), ptr(path),
                   ptr(pn), ptr(counters)))
    dt = time.time() - t0
    for b, a in enumerate(searchers):
        r = a.r = result()
        r.n_nodes = int(nn[b])
        nodes = state[b, : nn[b]].copy()
        setattr(r, state_field, nodes)
        r.costs, r.parents = cost[b, : nn[b]].copy(), parent[b, : nn[b]].copy()
        r.counters = counters[b].copy()
        r.tSolve = dt
        if status[b]:
            r.status = "Solved"
            r.resultIdxs = path[b, : pn[b]].astype(np.int64)
            r.Path = nodes[r.resultIdxs - 1, :2].T.copy()  # getBestPath: 2 x k
            r.cost = float(bcost[b])
        else:
            r.status = "NotSolved"
    return searchers
