"""The case set of the occupancy-map tests (tests/test_gridmap_ref.py on the CPU, tests/test_gpu_gridmap.py on the
device): named maps at the smallest shapes at which the kernels of motionplanning_amd/csrc/gridmap.hip can go wrong.

The row pass takes 64 cells a step, so nx runs over {2, 63, 64, 65, 130}: one partial step, one full step, a full step
and one cell, two steps and two cells.  The column pass tiles four rows a block and searches up and down a column, so
ny runs over {2, 3, 5, 67, 130}: less than a tile, a tile and a row, and columns longer than 64 rows.
"""
import numpy as np

SHAPES = [(2, 2), (63, 3), (64, 5), (65, 67), (130, 130), (2, 130), (130, 2)]  # (nx, ny)
INFLATE_R2 = [0, 1, 2, 4, 5, 10 ** 6]


def _free(nx, ny):
    return np.ones((ny, nx), np.uint8)


def _points(nx, ny, pts, free_byte=1):
    m = np.full((ny, nx), free_byte, np.uint8)
    for x, y in pts:
        m[y, x] = 0
    return m


def _build():
    cases = []
    rng = np.random.default_rng(2048)
    for nx, ny in SHAPES:
        add = lambda name, m: cases.append((f"{name}_{nx}x{ny}", m))
        add("all_free", _free(nx, ny))
        add("all_blocked", np.zeros((ny, nx), np.uint8))
        for i, (x, y) in enumerate([(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)]):
            add(f"corner{i}", _points(nx, ny, [(x, y)]))
        add("point", _points(nx, ny, [(nx // 2, ny // 2)], free_byte=255))  # any nonzero byte is free
        add("dense", (rng.random((ny, nx)) >= 0.3).astype(np.uint8))
        sparse = _free(nx, ny)
        sparse.reshape(-1)[rng.choice(nx * ny, size=max(1, nx * ny // 1500), replace=False)] = 0
        add("sparse", sparse)
        # a row whose only blocked cell lies in the row's last 64-cell step (partial unless nx = 64)
        add("last_step", _points(nx, ny, [(nx - 1, ny // 2)]))
        if nx > 64:
            add("last_step_first", _points(nx, ny, [(64 * ((nx - 1) // 64), ny // 3)]))
        if ny > 64:  # the column search must pass 64 rows: the only blocked cells are in row 0
            far = _free(nx, ny)
            far[0, :] = 0
            add("column_far", far)
    # a free cell whose two nearest blocked cells tie: (15, 10) between (10, 10) and (20, 10); (40, 35) between rows
    cases.append(("tie_65x67", _points(65, 67, [(10, 10), (20, 10), (40, 30), (40, 40)])))
    # the nearest blocked cell lies in the same row (a blocked column) / in the same column (a blocked row)
    same_row = _free(65, 67)
    same_row[:, 30] = 0
    cases.append(("same_row_65x67", same_row))
    same_col = _free(65, 67)
    same_col[20, :] = 0
    cases.append(("same_column_65x67", same_col))
    # ... and diagonally: every cell off the point's row and column
    cases.append(("diagonal_65x67", _points(65, 67, [(31, 33)])))
    return cases


CASES = _build()
NAMES = [n for n, _ in CASES]


def by_shape():
    """{(nx, ny): (names, masks [B, ny, nx])}: one batch of unlike maps per shape."""
    out = {}
    for nx, ny in SHAPES:
        sel = [(n, m) for n, m in CASES if m.shape == (ny, nx)]
        out[(nx, ny)] = ([n for n, _ in sel], np.stack([m for _, m in sel]))
    return out


def get(name):
    return CASES[NAMES.index(name)][1]
