"""Hybrid A* setting groups away from main_hybrid_astar.jl's driver settings -- test infrastructure shared by
tests/test_hastar_settings_ref.py (the CPU oracle and tests/astar_ref.py on these settings) and
tests/test_gpu_hastar_settings.py (the device against the oracle).

Each group is a list of HybridAstarSearchers sharing one HybridAstarSettings shape (n_prim, n_col, resolutions,
stbound, vehicle, minR, number of walls) plus its max_pops; group(name) builds it, refs(name) plans it with the
CPU oracle once per process (16 threads: the ctypes calls release the GIL) and keeps the results unchanged.

    defaults   defineHybridAstar() untouched: 14 primitives, 100 columns, res (0.2, 0.2, π/10), 151 x 101 x 21
    np10       5 steers x 2 gears: n_prim mod 16 = 10, the tail without word units or prescan block
    np64       32 x 2, the limit (one neighbour per lane of the bookkeeping wave)
    np1        one primitive, straight ahead: the open list runs empty
    np17       17 x 1: a last 16-neighbour group with one lane, five 4-neighbour groups (the last with one)
    np16       8 x 2: four full 4-neighbour groups, one full 16-neighbour group
    ncol103    expand_time 1.03, (n_col - 1) % 5 = 2, res (0.5, 0.25, π/9): 31 x 41 x 19
    ncol6      n_col 6: two swept poses;  ncol5: n_col 5, one (the driver scenes scaled by 0.03)
    finepsi    res[2] = π/2100: no heading tables (4,202 >= 4,096 headings), 12 x 9 x 4201; six scenes of about
               89 MB of search state each, some 530 MB of device workspace for the one batch
    walls0     no walls: every scene connects at its first pop
    walls16    MAXW walls: the scene's 3 and 13 small blocks
    rawstart   driver settings, unregulated start headings beside regulated ones (mp_ha_plan directly)
"""
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle
from motionplanning_amd import hybrid_astar as ha
from motionplanning_amd.configs import julia_linrange

PI = math.pi


def _driver_like(scene, start=None, use_astar=False, **over):
    """ha.driver_searcher with some of driver_settings() replaced."""
    st = dict(ha.driver_settings(), **over)
    h = ha.defineHybridAstar(st["vehicle_size"], st["gear_set"], st["steer_set"], st["minR"], st["expand_time"],
                             st["resolutions"], st["stbound"], scene["starting_real"] if start is None else start,
                             scene["ending_real"], use_astar)
    ha.defineHybridAstarobs_(h, scene["walls"])
    return h


def _starts(n, seed):
    """ha.scenario_batch's starts: x in {5, 5.5, ..., 9}, heading π/2 + k·π/12, k in {-2..2}; the first half of the
    n for the perpendicular scene, the second for the parallel one."""
    r = np.random.default_rng(seed)
    xs = np.arange(5.0, 9.0 + 1e-9, 0.5)
    out = []
    for i in range(n):
        scene = ha.PERPENDICULAR if i < n // 2 else ha.PARALLEL
        x = float(xs[r.integers(len(xs))])
        k = int(r.integers(-2, 3))
        out.append((scene, [x, 0.0, PI / 2 + k * PI / 12]))
    return out


def _driver_group(n_extra, seed, use_astar, **over):
    """Both driver scenes, then n_extra seeded scenario_batch-style starts, all with the overrides."""
    hs = [_driver_like(ha.PERPENDICULAR, None, use_astar, **over), _driver_like(ha.PARALLEL, None, use_astar, **over)]
    hs += [_driver_like(sc, st, use_astar, **over) for sc, st in _starts(n_extra, seed)]
    return hs


def _steers(n):
    minR = ha.driver_settings()["minR"]
    return julia_linrange(-1 / minR, 1 / minR, n)


# of default_rng(1)'s first 40 default-settings scenes: two stopped at 400 pops, two found before pop 20, six found
# at pops 42, 124, 312, 57, 265 and 23 (the oracle's figures, asserted by tests/test_hastar_settings_ref.py)
DEFAULT_SCENES = (0, 1, 2, 3, 8, 11, 13, 15, 21, 23)


def _defaults(use_astar, keep=DEFAULT_SCENES):
    r = np.random.default_rng(1)
    hs = []
    for _ in range(max(keep) + 1):
        w1 = [2.5, -5 + r.uniform(-1, 1), 0.0, 0.5, r.uniform(1, 2.5)]
        w2 = [r.uniform(-10, 10), r.uniform(-12, 2), r.uniform(-PI, PI), r.uniform(0.5, 2), r.uniform(0.3, 1)]
        goal = [-5 + r.uniform(-2, 2), -5 + r.uniform(-2, 2), r.uniform(-PI, PI)]
        h = ha.defineHybridAstar(ending_real=goal, use_astar=use_astar)
        ha.defineHybridAstarobs_(h, [w1, w2])
        hs.append(h)
    return [hs[i] for i in keep]


def _listed(rows, use_astar, **over):
    """Both driver scenes, then the listed (scene, [x, y, quarter-turn-relative heading]) starts."""
    hs = [_driver_like(ha.PERPENDICULAR, None, use_astar, **over), _driver_like(ha.PARALLEL, None, use_astar, **over)]
    return hs + [_driver_like(sc, [x, y, PI / 2 + dpsi], use_astar, **over) for sc, x, y, dpsi in rows]


def _scaled(scene, k):
    """The scene with every length multiplied by k (headings kept)."""
    sc3 = lambda s: [s[0] * k, s[1] * k, s[2]]
    return dict(starting_real=sc3(scene["starting_real"]), ending_real=sc3(scene["ending_real"]),
                walls=[[w[0] * k, w[1] * k, w[2], w[3] * k, w[4] * k] for w in scene["walls"]])


def _small(expand_time, use_astar, n_extra=12, seed=2):
    """The driver problem scaled by K = 0.03 (a 9 cm vehicle on a 1.5 cm lattice), so that an expansion of 5 or 6
    Euler steps at speed 1 still crosses cells: expand_time 0.065 / 0.055 stand for 2.17 / 1.83 s of the driver's."""
    K = 0.03
    st = ha.driver_settings()
    over = dict(vehicle_size=[3 * K, 2 * K], minR=st["minR"] * K, steer_set=st["steer_set"] / K,
                expand_time=expand_time, resolutions=[0.5 * K, 0.5 * K, PI / 12],
                stbound=[[-5 * K, 10 * K], [0, 10 * K], [-PI, PI]])
    scenes = [(ha.PERPENDICULAR, None), (ha.PARALLEL, None)] + _starts(n_extra, seed)
    hs = []
    for scene, start in scenes:
        sc = _scaled(scene if start is None else dict(scene, starting_real=start), K)
        hs.append(_driver_like(sc, None, use_astar, **over))
    return hs


def _walls16(use_astar):
    r = np.random.default_rng(5)
    extra = [[r.uniform(-5, 10), r.uniform(6, 10), r.uniform(-PI, PI), 0.3, 0.3] for _ in range(13)]
    scenes = [(ha.PERPENDICULAR, None), (ha.PARALLEL, None)] + _starts(4, 4)
    return [_driver_like(dict(sc, walls=sc["walls"] + extra), st, use_astar) for sc, st in scenes]


def _walls0(use_astar):
    scenes = [(ha.PERPENDICULAR, None), (ha.PARALLEL, None)] + _starts(2, 4)
    return [_driver_like(dict(sc, walls=[]), st, use_astar) for sc, st in scenes]


# name -> (builder(use_astar), max_pops)
GROUPS = {
    "defaults": (_defaults, 400),
    "np10": (lambda ua: _driver_group(10, 4, ua, steer_set=_steers(5)), 300),
    "np64": (lambda ua: _driver_group(4, 4, ua, steer_set=_steers(32)), 300),
    "np1": (lambda ua: _driver_group(0, 4, ua, steer_set=[0.0], gear_set=[1]), 300),
    "np17": (lambda ua: _driver_group(4, 4, ua, steer_set=_steers(17), gear_set=[1]), 300),
    "np16": (lambda ua: _driver_group(6, 4, ua, steer_set=_steers(8)), 300),
    "ncol103": (lambda ua: _listed([(ha.PARALLEL, 4.5, 3.0, 0.0), (ha.PARALLEL, 4.5, 3.0, 2 * PI / 9),
                                    (ha.PARALLEL, 5.5, 5.0, 2 * PI / 9), (ha.PARALLEL, 6.5, 5.0, 2 * PI / 9),
                                    (ha.PERPENDICULAR, 5.5, 1.0, 2 * PI / 9), (ha.PERPENDICULAR, 6.5, 3.0, 0.0)], ua,
                                   expand_time=1.03, resolutions=[0.5, 0.25, PI / 9]), 300),
    "ncol6": (lambda ua: _small(0.065, ua), 300),
    "ncol5": (lambda ua: _small(0.055, ua), 300),
    "finepsi": (lambda ua: _listed([(ha.PERPENDICULAR, 2.0, 5.0, -PI / 2), (ha.PERPENDICULAR, 2.0, 5.0, PI / 4),
                                    (ha.PARALLEL, 2.0, 3.0, -PI / 6), (ha.PERPENDICULAR, 6.0, 5.0, PI / 2)], ua,
                                   resolutions=[1.0, 1.0, PI / 2100], stbound=[[-2, 9], [0, 8], [-PI, PI]]), 200),
    "walls0": (_walls0, 300),
    "walls16": (_walls16, 300),
}
# the groups whose scenes must not all end the same way: every group but np1 and walls0, the raw starts included
MIXED = [g for g in GROUPS if g not in ("np1", "walls0")] + ["rawstart"]


def _walls_of(h):
    return np.array(h.s.obstacle_list, np.float64).reshape(-1, 5)


def group(name, use_astar=False):
    """(searchers, max_pops) of a group; fresh objects every call."""
    build, max_pops = GROUPS[name]
    return build(use_astar), max_pops


def sized(name, n, seed=11, use_astar=False):
    """n scenes of np10's or np64's settings (both driver scenes first), for the batch-shape thresholds."""
    return _driver_group(n - 2, seed, use_astar, steer_set=_steers({"np10": 5, "np64": 32}[name]))


def plan_refs_of(hs, max_pops):
    """The oracle's plans of a list of searchers sharing their settings."""
    sc, pc = primitives(hs[0])
    return plan_refs(ha.params_of(hs[0], max_pops), [h.s.starting_states for h in hs], [h.s.ending_states for h in hs],
                     [_walls_of(h) for h in hs], sc, pc)


def raw_starts():
    """(start [B][3], goal [B][3], walls [B][3][5], params, max_pops) for mp_ha_plan called directly: the driver
    scenes from starts whose heading is no lattice heading (starting_real as given, and off by an ulp, a few
    degrees, more than π) beside regulated ones."""
    hs = [ha.driver_searcher(ha.PERPENDICULAR), ha.driver_searcher(ha.PARALLEL)]
    rows = []
    for h in hs:
        reg = h.s.starting_states
        rows.append((h, reg.copy()))
        rows.append((h, h.s.starting_real.copy()))  # starting_real as the driver gives it
        rows.append((h, np.array([reg[0], reg[1], np.nextafter(reg[2], 4.0)])))
        rows.append((h, np.array([reg[0] - 0.5, reg[1], 1.5])))
        rows.append((h, np.array([reg[0] - 1.0, reg[1] + 0.13, 1.7 + 2 * PI])))  # off the x/y lattice, beyond π
        rows.append((h, np.array([6.0, 0.0, 7 * (PI / 12)])))
    start = np.array([r[1] for r in rows])
    goal = np.array([r[0].s.ending_states for r in rows])
    walls = np.array([r[0].s.obstacle_list for r in rows], np.float64)
    return start, goal, walls, hs[0], 300


def primitives(h):
    return oracle.ha_neighbor_origin(h.s.expand_time, h.s.steer_set, h.s.gear_set)


def plan_refs(p, starts, goals, walls, sc, pc):
    """oracle.ha_plan for every scene, 16 at a time."""
    def one(i):
        return oracle.ha_plan(p, starts[i], goals[i], walls[i], sc, pc)

    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(one, range(len(starts))))


@functools.lru_cache(maxsize=None)
def refs(name):
    """The oracle's plans of group `name` (shared by the tests of this process; not to be modified)."""
    if name == "rawstart":
        start, goal, walls, h0, max_pops = raw_starts()
        sc, pc = primitives(h0)
        return plan_refs(ha.params_of(h0, max_pops), start, goal, walls, sc, pc)
    return plan_refs_of(*group(name))


@functools.lru_cache(maxsize=None)
def restated(name, table):
    """tests/astar_ref.py's ha_plan of every scene of group `name`: without a table (the oracle's search restated),
    or with astar_heuristic's table (use_astar = true, which the oracle does not have)."""
    import astar_ref as R

    hs, max_pops = group(name)
    p = ha.params_of(hs[0], max_pops)
    sc, pc = primitives(hs[0])
    out = []
    for h in hs:
        walls = _walls_of(h)
        tab = R.ha_table(p, h.s.ending_states, walls)[0] if table else None
        out.append(R.ha_plan(p, h.s.starting_states, h.s.ending_states, walls, sc, pc, tab))
    return out


def counts(rs, max_pops):
    """(found after >= 20 pops, stopped at max_pops, open list emptied, found at pop 1) of a list of plans."""
    late = sum(1 for r in rs if r["found"] and r["pops"] >= 20)
    stopped = sum(1 for r in rs if not r["found"] and r["pops"] == max_pops)
    emptied = sum(1 for r in rs if not r["found"] and r["pops"] < max_pops)
    first = sum(1 for r in rs if r["found"] and r["pops"] == 1)
    return late, stopped, emptied, first


def conditions_hold(name, rs, max_pops):
    """So that a comparison cannot pass by doing nothing: a MIXED group has at least 2 scenes found after >= 20 pops,
    at least 1 not found and at most half found at pop 1; np1 ends every scene with an empty open list, walls0 connects
    every scene at its first pop."""
    late, stopped, emptied, first = counts(rs, max_pops)
    if name == "np1":
        return emptied == len(rs)
    if name == "walls0":
        return first == len(rs)
    assert name in MIXED, name
    return late >= 2 and stopped + emptied >= 1 and 2 * first <= len(rs)
