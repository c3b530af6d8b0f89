"""Car-like RRT / RRT* — host-side mirror of PathPlanning/RRTNonholonomic/src/{types,setup,rrt_utils}.jl over the
libmpgpu C-ABI (mp_rrtnh_plan).

``defineRRT`` / ``defineRRTobs_`` / ``planRRT_`` keep the reference's names and argument order.  Nodes are poses
[x, y, psi]; the whole sampling loop runs in the library, one workgroup per tree; ``plan_batch`` grows B trees that
share the settings in one call (bounds, start pose, goal and obstacle lists may differ per tree).  The library
draws no random numbers: the six uniforms of every iteration (u_bias, u_x, u_y, u_psi, u_ratio, u_yaw) are an
input, drawn here with ``numpy.random.default_rng(seed)`` unless given.  The terrain, candidacy and TPP parts of
the reference are never reached from planRRT! and have no counterpart.
"""
from dataclasses import dataclass, field

import numpy as np

from . import _rrt
from ._rrt import defineRRTobs_  # noqa: F401  (defineRRTobs!, setup.jl:41-44: circles [x, y, r])
from .context import default_context


@dataclass
class RRTSettings:
    """types.jl:97-116 (the terrain, candidacy and drawing fields have no counterpart)."""

    starting_position: np.ndarray = None
    starting_ang: float = 0.0
    ending_position: np.ndarray = None
    ending_ang: object = 0.0  # stored only: planRRT! never reads it
    BoundPosition: np.ndarray = None
    obstacle_list: list = field(default_factory=list)
    goal_tolerance: float = 1.0
    grow_dist: tuple = (1.0, 3.0)
    sampling_number: int = 0
    buffer_size: int = 0
    rrt_star: bool = False
    bias_rate: float = 0.2
    seed: int = 0


@dataclass
class RRTResult:
    """types.jl:133-139, plus the tree (node i, 1-based, in row i - 1) and the planner's counters."""

    status: str = "NaN"
    Path: np.ndarray = None
    resultIdxs: np.ndarray = None
    tSolve: float = 1e6
    cost: float = 0.0
    n_nodes: int = 0
    states: np.ndarray = None  # n x 3 poses
    costs: np.ndarray = None
    parents: np.ndarray = None
    # samples rejected by the bound test, by kinematics, by a circle; rewired edges; capped near sets; in-range
    # steers; steers that drew ang_ratio; near sets with a radius below 24
    counters: np.ndarray = None

    def tree_segments(self):
        """getTree (rrt_utils.jl:614-629): 3 x 2(n-1), columns [node, parent] for every node but the first."""
        idx = np.arange(1, self.n_nodes)
        if idx.size == 0:
            return np.zeros((3, 0))
        seg = np.empty((3, 2 * idx.size))
        seg[:, 0::2] = self.states[idx].T
        seg[:, 1::2] = self.states[self.parents[idx] - 1].T
        return seg


@dataclass
class RRTSearcher:
    s: RRTSettings = field(default_factory=RRTSettings)
    r: RRTResult = field(default_factory=RRTResult)


def defineRRT(sampleNum=10000, starting_pose=(35.0, 50.0), starting_ang=0.0, ending_pose=(100.0, 50.0),
              ending_ang=(0.0, 0.0), buffer_size=100, BoundPosition=(0, 100, 0, 100), rrt_star=False, bias_rate=0.2,
              seed=0):
    """setup.jl:2-38; ``ending_ang`` is accepted and stored only, ``seed`` seeds the uniforms."""
    rrt = RRTSearcher()
    s = rrt.s
    s.sampling_number, s.buffer_size = int(sampleNum), int(buffer_size)
    s.starting_position = np.asarray(starting_pose, np.float64).reshape(2)
    s.starting_ang = float(starting_ang)
    s.ending_position = np.asarray(ending_pose, np.float64).reshape(2)
    s.ending_ang = ending_ang
    s.BoundPosition = np.asarray(BoundPosition, np.float64).reshape(4)
    s.rrt_star, s.bias_rate, s.seed = bool(rrt_star), float(bias_rate), seed
    return rrt


def _pack(searchers, uniforms=None):
    return _rrt.pack_scenes(searchers, [[*a.s.starting_position, a.s.starting_ang] for a in searchers], 6, uniforms)


def plan_batch(searchers, ctx=None, uniforms=None):
    """planRRT! for B searchers sharing sampling_number, buffer_size, rrt_star, bias_rate, grow_dist and
    goal_tolerance.  uniforms: [B][n_iter][6] (u_bias, u_x, u_y, u_psi, u_ratio, u_yaw), or None to draw them per
    searcher from ``numpy.random.default_rng(searcher.s.seed)``."""
    ctx = ctx or default_context()
    return _rrt.run(ctx, ctx.lib.mp_rrtnh_plan, _pack(searchers, uniforms), searchers, RRTResult, "states", 8)


def planRRT_(rrt, ctx=None, uniforms=None):
    """planRRT! (rrt_utils.jl:528-583) for one searcher; uniforms: [n_iter][6] or None."""
    plan_batch([rrt], ctx=ctx, uniforms=None if uniforms is None else [uniforms])
    return None
