"""Grid Dijkstra — host-side mirror of PathPlanning/Dijkstra/src/{types,setup,dka_utils}.jl over the libmpgpu
C-ABI (mp_dka_plan).

``defineDKA`` / ``defineDKAobs_`` / ``planDKA_`` keep the reference's names and argument meaning.  The search runs
in the library (planAstar!'s kernels without the heuristic): one wavefront per search up to 51 x 51 cells, one
workgroup on node tables in device memory above that (mp_grid_plan), and for a searcher that carries an occupancy
mask (``defineDKAmask_``); ``plan_batch`` runs B searches that share the grid size in one call, whatever their
obstacle counts.
"""
from dataclasses import dataclass, field

import numpy as np

from . import _gridsearch


@dataclass
class DKASettings:
    """types.jl:11-23."""

    actualbound: np.ndarray = None
    mapbound: np.ndarray = None
    starting_pos: np.ndarray = None
    ending_pos: np.ndarray = None
    starting_real: np.ndarray = None
    ending_real: np.ndarray = None
    obstacle_list: list = field(default_factory=list)
    x_factor: float = 0.0
    y_factor: float = 0.0
    free_mask: np.ndarray = None  # defineDKAmask_ (not in the reference): replaces obstacle_list


@dataclass
class DKAResult:
    """types.jl:34-39, plus the found flag, the popped goal node's f, the planner's loop_count / node count and
    the pop sequence."""

    dkapath: np.ndarray = None
    actualpath: np.ndarray = None
    planning_time: float = 0.0
    path_length: float = 0.0
    final_cost: float = 0.0
    found: bool = False
    loop_count: int = 0
    n_nodes: int = 0
    pop_sequence: np.ndarray = None


@dataclass
class DKASearcher:
    s: DKASettings = field(default_factory=DKASettings)
    r: DKAResult = field(default_factory=DKAResult)


def defineDKA(realsize=(-50, 0, 50, 100), mapbound=(51, 51), starting_real=(-3, 20), ending_real=(50, 20)):
    """setup.jl:3-25 (realsize = [xmin, xmax, ymin, ymax])."""
    return _gridsearch.define(DKASearcher(), realsize, mapbound, starting_real, ending_real)


def defineDKAobs_(dka, obstacle_list):
    """defineDKAobs! (setup.jl:28-31): circles [x, y, r]."""
    dka.s.obstacle_list = [list(map(float, o)) for o in obstacle_list]
    dka.s.free_mask = None


def defineDKAmask_(dka, mask):
    """An occupancy grid in place of the obstacle list: uint8 [ny, nx], nonzero = free (_gridsearch.define_mask)."""
    _gridsearch.define_mask(dka, mask)


def TransferCoordinate(dka, pos):
    """dka_utils.jl:217-220."""
    return _gridsearch.transfer(dka, pos)


def plan_batch(searchers, ctx=None):
    """planDKA! for B searchers sharing mapbound; shorter obstacle lists are padded with [0, 0, 0] circles."""
    return _gridsearch.plan_batch(searchers, "dka", "dkapath", ctx=ctx)


def planDKA_(dka, ctx=None):
    """planDKA! (dka_utils.jl:69-126) for one searcher."""
    plan_batch([dka], ctx=ctx)
    return None
