"""CPU restatements of the occupancy-map tools (include/mpgpu.h, "occupancy maps") -- test infrastructure only, the
checker of motionplanning_amd/csrc/gridmap.hip.

A map is uint8 mask[ny][nx], cell (ix, iy) (1-based) at mask[iy-1][ix-1], nonzero = free.  d2[ny][nx] is the squared
Euclidean distance, in cells, from each cell to the nearest blocked cell: 0 on a blocked cell, D2_NONE everywhere on a
map without one.  With the border a one-cell frame around the map (ix = 0, nx+1, iy = 0, ny+1) is blocked too.
Inflation by r2: a cell is free iff it is free in the input and d2 > r2.

Two independent restatements of d2, both in exact integers: d2_brute measures every cell against every blocked and
frame cell; d2_separable takes the distance along each row first and then the minimum over the rows of a column.
"""
import numpy as np

D2_NONE = 2 ** 31 - 1  # MP_MAP_D2_NONE
BORDER, OUT_OCCUPIED = 1, 2  # MP_MAP_BORDER, MP_MAP_OUT_OCCUPIED
_FAR = 1 << 30  # (its square still fits int64)


def d2_brute(mask, border=False):
    """min over every blocked cell (and frame cell) of dx^2 + dy^2; for small maps: cells x blocked cells."""
    mask = np.asarray(mask)
    ny, nx = mask.shape
    ys, xs = np.nonzero(mask == 0)
    px, py = [xs.astype(np.int64)], [ys.astype(np.int64)]
    if border:
        fx, fy = np.arange(-1, nx + 1), np.arange(-1, ny + 1)
        px += [fx, fx, np.full(ny + 2, -1), np.full(ny + 2, nx)]
        py += [np.full(nx + 2, -1), np.full(nx + 2, ny), fy, fy]
    px, py = np.concatenate(px), np.concatenate(py)
    if px.size == 0:
        return np.full((ny, nx), D2_NONE, np.int32)
    out = np.empty((ny, nx), np.int64)
    x = np.arange(nx, dtype=np.int64)
    for y in range(ny):
        out[y] = ((x[:, None] - px[None, :]) ** 2 + (y - py[None, :]) ** 2).min(axis=1)
    return out.astype(np.int32)


def row_distance(mask, border=False):
    """g[y][x]: the distance along row y to its nearest blocked cell (int64; _FAR or more: none)."""
    mask = np.asarray(mask)
    ny, nx = mask.shape
    x = np.broadcast_to(np.arange(nx, dtype=np.int64), (ny, nx))
    blocked = mask == 0
    left = np.maximum.accumulate(np.where(blocked, x, -_FAR), axis=1)
    right = np.minimum.accumulate(np.where(blocked, x, _FAR)[:, ::-1], axis=1)[:, ::-1]
    g = np.minimum(np.where(left < 0, _FAR, x - left), np.where(right >= _FAR, _FAR, right - x))
    if border:
        g = np.minimum(g, np.minimum(x + 1, nx - x))
    return g


def d2_separable(mask, border=False):
    """min over y' of g(x, y')^2 + (y - y')^2, and with the border the frame's rows above and below."""
    mask = np.asarray(mask)
    ny, nx = mask.shape
    g = row_distance(mask, border)
    g2 = np.where(g >= _FAR, np.int64(1) << 62, g * g)
    y = np.arange(ny, dtype=np.int64)
    best = np.full((ny, nx), np.int64(1) << 62)
    if border:
        best = np.minimum(best, (np.minimum(y + 1, ny - y) ** 2)[:, None])
    for yp in range(ny):
        best = np.minimum(best, g2[yp][None, :] + ((y - yp) ** 2)[:, None])
    return np.where(best >= (np.int64(1) << 62), D2_NONE, best).astype(np.int32)


def inflate(mask, r2, border=False, occupied=False, d2=None):
    """1 = free iff free in the input and d2 > r2 (occupied: the opposite polarity)."""
    d2 = d2_separable(mask, border) if d2 is None else d2
    free = (np.asarray(mask) != 0) & (d2.astype(np.int64) > int(r2))
    return (~free if occupied else free).astype(np.uint8)


def clearance(d2, path, n):
    """(min_d2, at) over the first n entries of path (Encode values 1..N, 0 skipped); the first index wins."""
    flat = np.asarray(d2).reshape(-1)
    best, at = D2_NONE, -1
    for i in range(int(n)):
        e = int(path[i])
        if e == 0:
            continue
        assert 1 <= e <= flat.size
        if at < 0 or flat[e - 1] < best:
            best, at = int(flat[e - 1]), i
    return best, at


def point_field(nx, ny, x0, y0, border=False):
    """d2 of an nx x ny map whose only blocked cell is (x0, y0) (0-based), analytically: (x-x0)^2 + (y-y0)^2, and
    with the border the frame at min(x+1, nx-x, y+1, ny-y) cells."""
    x, y = np.arange(nx, dtype=np.int64)[None, :], np.arange(ny, dtype=np.int64)[:, None]
    d = (x - x0) ** 2 + (y - y0) ** 2
    if border:
        d = np.minimum(d, np.minimum(np.minimum(x + 1, nx - x), np.minimum(y + 1, ny - y)) ** 2)
    return d.astype(np.int32)


def next_attainable(r2):
    """The least sum of two squares above r2: the least d2 a cell can have beyond r2 (r2 + 1 where that is one)."""
    v = int(r2) + 1
    while True:
        a = 0
        while a * a <= v:
            b = int(np.sqrt(v - a * a) + 0.5)
            if a * a + b * b == v:
                return v
            a += 1
        v += 1
