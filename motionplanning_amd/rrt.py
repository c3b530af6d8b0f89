"""RRT / RRT* — host-side mirror of PathPlanning/RRT/src/{types,setup,rrt_utils}.jl over the libmpgpu C-ABI
(mp_rrt_plan).

``defineRRT`` / ``defineRRTobs_`` / ``planRRT_`` keep the reference's names and argument order.  The whole
sampling loop runs in the library, one workgroup per tree; ``plan_batch`` grows B trees that share the
settings in one call (bounds, start, goal and obstacle lists may differ per tree).  The library draws no
random numbers: the three uniforms of every iteration are an input, drawn here with
``numpy.random.default_rng(seed)`` unless given.
"""
from dataclasses import dataclass, field

import numpy as np

from . import _rrt
from ._rrt import defineRRTobs_  # noqa: F401  (defineRRTobs!, setup.jl:43-46: circles [x, y, r])
from .context import default_context


@dataclass
class RRTSettings:
    """types.jl:19-39 (the terrain and drawing fields have no counterpart)."""

    starting_position: np.ndarray = None
    ending_position: np.ndarray = None
    BoundPosition: np.ndarray = None
    obstacle_list: list = field(default_factory=list)
    goal_tolerance: float = 1.0
    grow_dist: tuple = (0.0, 3.0)
    sampling_number: int = 0
    buffer_size: int = 0
    rrt_star: bool = False
    bias_rate: float = 0.2
    seed: int = 0


@dataclass
class RRTResult:
    """types.jl:57-63, plus the tree (node i, 1-based, in row i - 1) and the planner's counters."""

    status: str = "NaN"
    Path: np.ndarray = None
    resultIdxs: np.ndarray = None
    tSolve: float = 1e6
    cost: float = 0.0
    n_nodes: int = 0
    loc: np.ndarray = None
    costs: np.ndarray = None
    parents: np.ndarray = None
    counters: np.ndarray = None  # rejected samples, rewired edges, capped near sets, in-range steers

    def tree_segments(self):
        """retrieveTree (rrt_utils.jl:461-476): 2 x 2(n-1), columns [node, parent] for every node but the first."""
        idx = np.arange(1, self.n_nodes)
        if idx.size == 0:
            return np.zeros((2, 0))
        seg = np.empty((2, 2 * idx.size))
        seg[:, 0::2] = self.loc[idx].T
        seg[:, 1::2] = self.loc[self.parents[idx] - 1].T
        return seg


@dataclass
class RRTSearcher:
    s: RRTSettings = field(default_factory=RRTSettings)
    r: RRTResult = field(default_factory=RRTResult)


def defineRRT(sampling_size=10000, starting_pose=(35.0, 50.0), ending_pose=(100.0, 50.0), buffer_size=100,
              BoundPosition=(0, 100, 0, 100), rrt_star=False, bias_rate=0.2, draw_fig=False, make_gif=False, seed=0):
    """setup.jl:2-40 (draw_fig and make_gif are accepted and ignored); ``seed`` seeds the uniforms."""
    rrt = RRTSearcher()
    s = rrt.s
    s.sampling_number, s.buffer_size = int(sampling_size), int(buffer_size)
    s.starting_position = np.asarray(starting_pose, np.float64).reshape(2)
    s.ending_position = np.asarray(ending_pose, np.float64).reshape(2)
    s.BoundPosition = np.asarray(BoundPosition, np.float64).reshape(4)
    s.rrt_star, s.bias_rate, s.seed = bool(rrt_star), float(bias_rate), seed
    return rrt


def _pack(searchers, uniforms=None):
    return _rrt.pack_scenes(searchers, [a.s.starting_position for a in searchers], 3, uniforms)


def plan_batch(searchers, uniforms=None, ctx=None):
    """planRRT! for B searchers sharing sampling_number, buffer_size, rrt_star, bias_rate, grow_dist and
    goal_tolerance.  uniforms: [B][n_iter][3] (u_bias, u_x, u_y), or None to draw them per searcher from
    ``numpy.random.default_rng(searcher.s.seed)``."""
    ctx = ctx or default_context()
    return _rrt.run(ctx, ctx.lib.mp_rrt_plan, _pack(searchers, uniforms), searchers, RRTResult, "loc", 4)


def planRRT_(rrt, ctx=None):
    """planRRT! (rrt_utils.jl:341-412) for one searcher."""
    plan_batch([rrt], ctx=ctx)
    return None
