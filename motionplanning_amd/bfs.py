"""Grid breadth-first search — host-side mirror of PathPlanning/BreadthFirst/src/{types,setup,bfs_utils}.jl over
the libmpgpu C-ABI (mp_bfs_plan).

``defineBFS`` / ``defineBFSobs_`` / ``planBFS_`` keep the reference's names and argument meaning.  The search runs
in the library, a whole level of the queue at a time in the sequential loop's order: one wavefront per search up to
51 x 51 cells, one workgroup on tables in device memory above that (mp_grid_plan), and for a searcher that carries
an occupancy mask (``defineBFSmask_``); ``plan_batch`` runs B searches that share the grid size in one call,
whatever their obstacle counts.
"""
from dataclasses import dataclass, field

import numpy as np

from . import _gridsearch


@dataclass
class BFSSetting:
    """types.jl:9-21."""

    actualbound: np.ndarray = None
    mapbound: np.ndarray = None
    starting_pos: np.ndarray = None
    ending_pos: np.ndarray = None
    starting_real: np.ndarray = None
    ending_real: np.ndarray = None
    obstacle_list: list = field(default_factory=list)
    x_factor: float = 0.0
    y_factor: float = 0.0
    free_mask: np.ndarray = None  # defineBFSmask_ (not in the reference): replaces obstacle_list


@dataclass
class BFSResult:
    """types.jl:32-36, plus the found flag, the planner's loop_count / node count, the pop sequence and
    path_length (not in the reference's BFSResult: planDKA!'s fold over actualpath)."""

    bfspath: np.ndarray = None
    actualpath: np.ndarray = None
    planning_time: float = 0.0
    path_length: float = 0.0
    found: bool = False
    loop_count: int = 0
    n_nodes: int = 0
    pop_sequence: np.ndarray = None


@dataclass
class BFSSearcher:
    s: BFSSetting = field(default_factory=BFSSetting)
    r: BFSResult = field(default_factory=BFSResult)


def defineBFS(realsize=(-50, 0, 50, 100), mapbound=(51, 51), starting_real=(-3, 20), ending_real=(50, 20)):
    """setup.jl:3-25 (realsize = [xmin, xmax, ymin, ymax])."""
    return _gridsearch.define(BFSSearcher(), realsize, mapbound, starting_real, ending_real)


def defineBFSobs_(bfs, obstacle_list):
    """defineBFSobs! (setup.jl:28-31): circles [x, y, r]."""
    bfs.s.obstacle_list = [list(map(float, o)) for o in obstacle_list]
    bfs.s.free_mask = None


def defineBFSmask_(bfs, mask):
    """An occupancy grid in place of the obstacle list: uint8 [ny, nx], nonzero = free (_gridsearch.define_mask)."""
    _gridsearch.define_mask(bfs, mask)


def TransferCoordinate(bfs, pos):
    """bfs_utils.jl:163-166."""
    return _gridsearch.transfer(bfs, pos)


def plan_batch(searchers, ctx=None):
    """planBFS! for B searchers sharing mapbound; shorter obstacle lists are padded with [0, 0, 0] circles."""
    return _gridsearch.plan_batch(searchers, "bfs", "bfspath", ctx=ctx)


def planBFS_(bfs, ctx=None):
    """planBFS! (bfs_utils.jl:1-59) for one searcher."""
    plan_batch([bfs], ctx=ctx)
    return None
