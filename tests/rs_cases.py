"""Pose pairs and command tables for the Reeds-Shepp tests (tests/test_rs_cases.py on the CPU,
tests/test_gpu_rs.py on the device), with their expected values from the oracle (or_change_basis, or_ha_allpath,
or_ha_act_path, or_ha_rs_heuristic), computed once per process.

The random pairs are drawn as ReedsSheppsCurves/main.jl:3-14 draws them: x, y in +-10, ψ in +-π, minR in +-10
(negative turning radii included).  The special pairs are appended; SPECIAL names their offsets from the end.
"""
import ctypes
import functools

import numpy as np

import oracle
from motionplanning_amd.abi import HAParams, ptr

SEED, N_RANDOM = 11, 600
PI = np.pi
# offsets from the end of the pair set
SPECIAL = {"same": -6, "straight": -5, "pi": -4, "minus_pi": -3, "wide_pos": -2, "wide_neg": -1}


def pairs(seed=SEED, n=N_RANDOM):
    """(init[n + 6][3], term[n + 6][3], minR[n + 6])."""
    r = np.random.default_rng(seed)
    u = 2 * r.random((n, 7)) - 1
    init = np.c_[10 * u[:, 0], 10 * u[:, 1], PI * u[:, 2]]
    term = np.c_[10 * u[:, 3], 10 * u[:, 4], PI * u[:, 5]]
    minR = 10 * u[:, 6]
    sp_init = [[1.5, -2.0, 0.7],     # start == goal: the normalised state is 0
               [1.0, 2.0, 0.0],      # goal straight ahead at 2 minR: normalised [2, 0, 0]
               [0.0, 0.0, 0.0],      # normalised [3, 2, π]
               [0.0, 0.0, 0.0],      # normalised [-3, -2, -π]
               [2.0, -1.0, 50.0],    # start headings outside the fast sincos range
               [-4.0, 3.0, -50.0]]
    sp_term = [[1.5, -2.0, 0.7], [4.0, 2.0, 0.0], [3.0, 2.0, PI], [-3.0, -2.0, -PI], [-3.0, 5.0, 1.0], [6.0, 1.0, -2.0]]
    sp_minR = [2.0, 1.5, 1.0, 1.0, 2.5, -1.25]
    return (np.ascontiguousarray(np.r_[init, sp_init]), np.ascontiguousarray(np.r_[term, sp_term]),
            np.ascontiguousarray(np.r_[minR, sp_minR]))


# ------------------------------------------------------------------ the oracle, per pair
def _lib():
    L = oracle._ha()
    if not getattr(L, "_rs_cases_ready", False):  # or_ha_act_path has no argtypes in oracle/__init__.py
        L.or_ha_act_path.restype = ctypes.c_int
        L.or_ha_act_path.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        L._rs_cases_ready = True
    return L


def change_basis(init, term, minR):
    out = np.zeros(3)
    _lib().or_change_basis(ptr(np.ascontiguousarray(init, np.float64)), ptr(np.ascontiguousarray(term, np.float64)),
                           float(minR), ptr(out))
    return out


def act_path(init, minR, table):
    """or_ha_act_path: the n x 3 path of one command table [5][3]."""
    buf = np.zeros((501, 3))
    n = _lib().or_ha_act_path(ptr(np.ascontiguousarray(init, np.float64)), float(minR),
                              ptr(np.ascontiguousarray(table, np.float64)), ptr(buf))
    return buf[:n].copy()


def rs_heuristic(a, b, minR):
    p = HAParams()
    p.minR = float(minR)
    return _lib().or_ha_rs_heuristic(ctypes.byref(p), ptr(np.ascontiguousarray(a, np.float64)),
                                     ptr(np.ascontiguousarray(b, np.float64)))


def n_segments(tables):
    """createPath's cmd_idx of tables[..., 5, 3]: rows before the first with gear == 0."""
    zero = np.asarray(tables)[..., 1] == 0
    return np.where(zero.any(-1), zero.argmax(-1), 5)


@functools.lru_cache(maxsize=None)
def reference():
    """The oracle's values for pairs(): norm[n][3], cost[n][48], cmds[n][48][5][3], best[n], act_cost[n].  Shared by
    the tests; leave it unchanged."""
    init, term, minR = pairs()
    n = len(init)
    norm, cost, cmds = np.zeros((n, 3)), np.zeros((n, 48)), np.zeros((n, 48, 5, 3))
    best = np.zeros(n, np.int32)
    for i in range(n):
        norm[i] = change_basis(init[i], term[i], minR[i])
        best[i], cost[i], cmds[i] = oracle.ha_allpath(norm[i])
    return dict(init=init, term=term, minR=minR, norm=norm, cost=cost, cmds=cmds, best=best,
                act_cost=cost[np.arange(n), best] * minR)


HAND_TABLES = {
    "one_segment": [[1.3, 1, 1]],
    "two_segments": [[0.7, -1, -1], [2.1, 1, 0]],
    "gear0_in_the_middle": [[1.0, 1, 1], [0.5, 0, 1], [2.0, 1, -1], [1.0, -1, 1]],  # one segment counts
    "all_zero": [],
    "straight": [[3.0, 1, 0]],                                   # steer 0: ψ constant, equal increments
    "zero_length_arcs": [[0.0, 1, 1], [2.0, 1, 0], [0.0, 1, 1]],
    "five_segments": [[0.4, 1, 1], [PI / 2, -1, -1], [1.7, -1, 0], [PI / 2, -1, 1], [0.9, 1, -1]],
    "negative_length": [[-0.8, 1, -1], [1.1, -1, 1]],            # createActPath takes abs(length)
}


@functools.lru_cache(maxsize=None)
def tables():
    """Command tables for mp_rs_create_path with a start and a turning radius each: every pair's winner, 200 feasible
    non-winners, the hand-made ones last.  dict(cmds[m][5][3], init[m][3], minR[m], n_hand)."""
    ref = reference()
    n = len(ref["best"])
    r = np.random.default_rng(SEED + 1)
    pb, pc = np.nonzero((ref["cost"] < np.inf) & (np.arange(48)[None, :] != ref["best"][:, None]))
    pick = r.choice(len(pb), 200, replace=False)
    rows_b = np.r_[np.arange(n), pb[pick]]
    rows_c = np.r_[ref["best"].astype(np.int64), pc[pick]]
    hand = np.zeros((len(HAND_TABLES), 5, 3))
    for i, t in enumerate(HAND_TABLES.values()):
        if t:
            hand[i, : len(t)] = t
    h = len(hand)
    h_init = np.c_[10 * (2 * r.random((h, 2)) - 1), PI * (2 * r.random(h) - 1)]
    h_minR = np.where(np.arange(h) % 3 == 2, -1.0, 1.0) * (0.5 + 4 * r.random(h))
    return dict(cmds=np.ascontiguousarray(np.r_[ref["cmds"][rows_b, rows_c], hand]),
                init=np.ascontiguousarray(np.r_[ref["init"][rows_b], h_init]),
                minR=np.ascontiguousarray(np.r_[ref["minR"][rows_b], h_minR]), n_hand=h)


@functools.lru_cache(maxsize=None)
def table_paths(act=True):
    """The oracle's path of every table of tables(): createActPath (act) or createPath, which is the oracle with
    init = 0 and minR = 1.0."""
    t = tables()
    if act:
        return [act_path(i, m, c) for i, m, c in zip(t["init"], t["minR"], t["cmds"])]
    return [act_path(np.zeros(3), 1.0, c) for c in t["cmds"]]
