"""The case set of the goal-distance field tests: tests/test_gridfield_ref.py checks the restatement on it (and
that it covers what it claims), tests/test_gpu_gridfield.py checks mp_grid_field against the restatement.

A case is a dict: name, nx, ny, bound [xmin, xmax, ymin, ymax], mask uint8 [ny, nx], source (a cell, 1-based, which
may lie off the grid), queries (cells) and stride.  ``real(case, cell)`` is a point inside a cell.
"""
import numpy as np

from astar_ref import Grid


def grid_of(case):
    return Grid(case["bound"], case["nx"], case["ny"])


def real(case, cell):
    """A point in the middle of a cell (also of a cell off the grid)."""
    g = grid_of(case)
    return ((cell[0] - 0.5) * g.xf + g.b[0], (cell[1] - 0.5) * g.yf + g.b[2])


def _case(name, mask, source, bound=None, queries=(), stride=64):
    mask = np.ascontiguousarray(mask, np.uint8)
    ny, nx = mask.shape
    bound = [0.0, nx - 1.0, 0.0, ny - 1.0] if bound is None else bound  # unit cells
    return dict(name=name, nx=nx, ny=ny, bound=[float(v) for v in bound], mask=mask, source=tuple(source),
                queries=[tuple(q) for q in queries], stride=stride)


def _seeded(seed, nx, ny, density, bound):
    r = np.random.default_rng(seed)
    mask = (r.random((ny, nx)) >= density).astype(np.uint8)
    free = np.argwhere(mask != 0)
    sy, sx = free[r.integers(len(free))] if len(free) else (0, 0)
    qs = [(int(x) + 1, int(y) + 1) for y, x in free[r.permutation(len(free))[:6]]]
    return _case(f"seeded{seed}_{nx}x{ny}", mask, (int(sx) + 1, int(sy) + 1), bound, qs)


def pocket_map():
    """9 x 8, unit cells: a free cell (7, 6) walled in on all eight sides, the rest free."""
    m = np.ones((8, 9), np.uint8)
    m[4:7, 5:8] = 0
    m[5, 6] = 1
    return m


def staircase_map():
    """6 x 6: free cells (5,1), (4,2), (3,3), (2,4), (1,5) only, joined by (-1, +1) moves alone: MOVES_8 walks up
    the stair from (5,1), MOVES_REF, which lacks that move, cannot; walking down it uses (1, -1), which both have."""
    m = np.zeros((6, 6), np.uint8)
    for i in range(5):
        m[i, 4 - i] = 1
    return m


def small_cases():
    """Maps of at most 12 x 11 cells: the CPU tests run planDKA!'s restatement to every free cell of each."""
    cases = []
    # seeded maps, square and non-square cells, densities 0 .. 0.35
    shapes = [(7, 11), (12, 7), (9, 9), (11, 8), (8, 10), (12, 11), (10, 7)]
    for i, (nx, ny) in enumerate(shapes):
        bound = [-1.5, -1.5 + 0.47 * (nx - 1), 2.0, 2.0 + 0.31 * (ny - 1)] if i % 2 == 0 else \
            [0.0, 1.3 * (nx - 1), -4.0, -4.0 + 0.9 * (ny - 1)]
        cases.append(_seeded(100 + i, nx, ny, 0.05 * i, bound))
    cases.append(_case("all_free_corner", np.ones((7, 9), np.uint8), (1, 1), queries=[(9, 7), (3, 2), (1, 1), (9, 1)]))
    cases.append(_case("all_free_far_corner", np.ones((6, 5), np.uint8), (5, 6), [0.0, 2.0, 1.0, 4.5],
                       queries=[(1, 1), (3, 5)]))
    only = np.zeros((5, 6), np.uint8)
    cases.append(_case("all_blocked_but_source", only, (3, 2), queries=[(3, 2), (4, 2)]))
    # the pocket (7, 6) is unreached; (0, 3) and (10, 9) are off the grid
    cases.append(_case("pocket", pocket_map(), (2, 2), queries=[(7, 6), (0, 3), (10, 9), (9, 8), (5, 8)]))
    blocked_src = np.ones((7, 8), np.uint8)
    blocked_src[3, 4] = 0
    cases.append(_case("blocked_source_spreads", blocked_src, (5, 4), [0.0, 3.5, 0.0, 1.8], queries=[(1, 1), (8, 7)]))
    cases.append(_case("staircase", staircase_map(), (5, 1), queries=[(1, 5), (3, 3)]))
    cases.append(_case("staircase_down", staircase_map(), (1, 5), queries=[(5, 1)]))
    cases.append(_case("source_off_grid", np.ones((4, 5), np.uint8), (0, 2), queries=[(2, 2)]))
    # a path of 12 cells into a stride of 5
    cases.append(_case("stride_cut", np.ones((3, 12), np.uint8), (1, 2), queries=[(12, 2), (4, 1)], stride=5))
    return cases


def serpentine(nx=130, ny=67, cell=(0.47, 0.31)):
    """Odd rows (iy = 2, 4, ...) blocked except one gap at alternating ends; cells 0.47 x 0.31; source (1, 1)."""
    m = np.ones((ny, nx), np.uint8)
    for k, row in enumerate(range(1, ny, 2)):
        m[row] = 0
        m[row, nx - 1 if k % 2 == 0 else 0] = 1
    bound = [0.0, cell[0] * (nx - 1), 0.0, cell[1] * (ny - 1)]
    return _case(f"serpentine_{nx}x{ny}", m, (1, 1), bound, queries=[(nx, ny), (1, ny), (nx // 2, ny // 2 | 1)],
                 stride=nx * ny)


# the tile side of gridfield.hip is 64: the sizes straddle it in both directions
GPU_NX, GPU_NY = (2, 63, 64, 65, 130), (2, 3, 67, 130)


def sized(nx, ny):
    """A seeded map of nx x ny at density 0.25 with non-square cells, the source in a tile corner or on a tile edge
    (whichever of (64, 64), (65, 65), (64, 1), (1, 64) the map has, else its far corner), four queries."""
    r = np.random.default_rng(1000 * nx + ny)
    mask = (r.random((ny, nx)) >= 0.25).astype(np.uint8)
    spots = [(sx, sy) for sx, sy in [(64, 64), (65, 65), (64, 1), (1, 64), (65, 3)] if sx <= nx and sy <= ny]
    src = spots[(nx + ny) % len(spots)] if spots else (nx, ny)
    qs = [(nx, ny), (1, 1), (nx, 1), (max(1, nx // 2), max(1, ny // 2))]
    return _case(f"sized_{nx}x{ny}", mask, src, [0.0, 0.47 * (nx - 1), 0.0, 0.31 * (ny - 1)], qs, stride=nx + ny)


def rim_source():
    """70 x 69: the source (64, 64) is the only member of its tile, so every way out starts in another tile (all
    three of them: the source is the tile's corner cell)."""
    m = np.ones((69, 70), np.uint8)
    m[:64, :64] = 0
    return _case("rim_source", m, (64, 64), [0.0, 0.47 * 69, 0.0, 0.31 * 68], [(70, 69), (65, 1), (1, 65), (1, 1)], stride=140)


def batch_of_six():
    """Six unlike 70 x 66 maps: densities, cell shapes and sources differ; one is all free, one has no way out of
    the source."""
    nx, ny = 70, 66
    out = []
    for i in range(6):
        r = np.random.default_rng(50 + i)
        mask = (r.random((ny, nx)) >= [0.0, 0.1, 0.2, 0.3, 0.35, 1.0][i]).astype(np.uint8)
        src = [(1, 1), (64, 64), (70, 66), (65, 2), (33, 65), (40, 40)][i]
        bound = [0.1 * i, 0.1 * i + (0.2 + 0.1 * i) * (nx - 1), -1.0, -1.0 + 0.5 * (ny - 1)]
        out.append(_case(f"six_{i}", mask, src, bound, [(nx, ny), (1, 1), (35, 33)], stride=nx + ny))
    return out


def band(n=2048):
    """n x n, blocked except a three-cell band along the bottom row and the right column; source in the far corner
    (1, 1) of the band's start, queries at the band's other end (n, n): offsets beyond 2^21 cells."""
    m = np.zeros((n, n), np.uint8)
    m[:3, :] = 1
    m[:, n - 3:] = 1
    return _case(f"band_{n}", m, (1, 1), [0.0, 0.5 * (n - 1), 0.0, 0.25 * (n - 1)], queries=[(n, n), (n - 2, n // 2)],
                 stride=2 * n)
