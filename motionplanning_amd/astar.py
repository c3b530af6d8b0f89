"""Grid A* — host-side mirror of PathPlanning/Astar/src/{types,setup,astar_utils}.jl over the libmpgpu
C-ABI (mp_astar_plan, mp_grid_plan).

``defineAstar`` / ``defineAstarobs_`` / ``planAstar_`` keep the reference's names and argument meaning.
The search runs in the library: up to 51 x 51 cells one wavefront per search, node table and open list in LDS;
above that, and for a searcher that carries an occupancy mask (``defineAstarmask_``), one workgroup per search on
node tables in device memory (mp_grid_plan).  ``plan_batch`` runs B searches that share the grid size, the obstacle
kind and the obstacle count in one call.
"""
import math
from dataclasses import dataclass, field

import numpy as np

from . import _gridsearch
from .abi import f64
from .context import default_context


@dataclass
class AstarSettings:
    """types.jl:13-25."""

    actualbound: np.ndarray = None
    mapbound: np.ndarray = None
    starting_pos: np.ndarray = None
    ending_pos: np.ndarray = None
    starting_real: np.ndarray = None
    ending_real: np.ndarray = None
    obstacle_list: list = field(default_factory=list)
    x_factor: float = 0.0
    y_factor: float = 0.0
    free_mask: np.ndarray = None  # defineAstarmask_ (not in the reference): replaces obstacle_list


@dataclass
class AstarResult:
    """types.jl:36-42, plus the planner's loop_count / node count and the pop sequence."""

    astarpath: np.ndarray = None
    actualpath: np.ndarray = None
    planning_time: float = 0.0
    final_cost: float = 0.0
    path_length: float = 0.0
    found: bool = False
    loop_count: int = 0
    n_nodes: int = 0
    pop_sequence: np.ndarray = None


@dataclass
class AstarSearcher:
    s: AstarSettings = field(default_factory=AstarSettings)
    r: AstarResult = field(default_factory=AstarResult)


def defineAstar(realsize=(-50, 0, 50, 100), mapbound=(51, 51), starting_real=(-3, 20), ending_real=(50, 20)):
    """setup.jl:3-24 (realsize = [xmin, xmax, ymin, ymax]); the drawing flags have no counterpart."""
    a = AstarSearcher()
    s = a.s
    s.actualbound = np.asarray(realsize, np.float64)
    s.mapbound = np.asarray(mapbound, np.float64)
    s.starting_real = np.asarray(starting_real, np.float64)
    s.ending_real = np.asarray(ending_real, np.float64)
    s.x_factor = (s.actualbound[1] - s.actualbound[0]) / (s.mapbound[0] - 1)
    s.y_factor = (s.actualbound[3] - s.actualbound[2]) / (s.mapbound[1] - 1)
    s.starting_pos = np.array([math.floor((s.starting_real[0] - s.actualbound[0]) / s.x_factor + 1),
                               math.floor((s.starting_real[1] - s.actualbound[2]) / s.y_factor + 1)], np.int64)
    s.ending_pos = np.array([math.floor((s.ending_real[0] - s.actualbound[0]) / s.x_factor + 1),
                             math.floor((s.ending_real[1] - s.actualbound[2]) / s.y_factor + 1)], np.int64)
    return a


def defineAstarobs_(a, obstacle_list):
    """defineAstarobs! (setup.jl:27-30): circles [x, y, r] or blocks [x, y, ψ, l/2, w/2]."""
    a.s.obstacle_list = [list(map(float, o)) for o in obstacle_list]
    a.s.free_mask = None


def defineAstarmask_(a, mask):
    """An occupancy grid in place of the obstacle list: uint8 [ny, nx], nonzero = free (_gridsearch.define_mask)."""
    _gridsearch.define_mask(a, mask)


def TransferCoordinate(a, pos):
    """astar_utils.jl:237-240."""
    s = a.s
    return np.array([(pos[0] - 1.0) * s.x_factor + s.actualbound[0], (pos[1] - 1.0) * s.y_factor + s.actualbound[2]])


def plan_batch(searchers, ctx=None):
    """planAstar! for B searchers sharing mapbound and either the obstacle kind and count, or all carrying masks."""
    ctx = ctx or default_context()
    masks = _gridsearch.batch_masks(searchers)
    a0 = searchers[0]
    nx, ny = int(a0.s.mapbound[0]), int(a0.s.mapbound[1])
    n_obs = len(a0.s.obstacle_list)
    kind = len(a0.s.obstacle_list[0]) if n_obs else 3
    for a in searchers:
        if (int(a.s.mapbound[0]), int(a.s.mapbound[1])) != (nx, ny) or len(a.s.obstacle_list) != n_obs or any(
                len(o) != kind for o in a.s.obstacle_list):
            raise ValueError("plan_batch: every search needs the same mapbound, obstacle kind and obstacle count")
    obs = f64([a.s.obstacle_list for a in searchers]).reshape(len(searchers), n_obs, kind) if n_obs else None
    return _gridsearch.run(ctx, "astar", searchers, nx, ny, kind, n_obs, obs, masks, "astarpath")


def planAstar_(a, ctx=None):
    """planAstar! (astar_utils.jl:83-141) for one searcher."""
    plan_batch([a], ctx=ctx)
    return None
