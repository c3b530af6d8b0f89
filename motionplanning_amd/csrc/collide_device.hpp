// collide_device.hpp — the rectangle and SAT device code that collide.hip (the batched collision calls) and
// roadmap.hip (the roadmap's fused edge check) share: GetRectanglePts, a rectangle's per-edge SAT table and
// SeparatingAxisTheorem on it (PathPlanning/CollisionDetection/src/utils.jl), rounded as collide.hip describes;
// the wall rows of an LDS tile, a checked pose's vehicle rectangle and the walk of the pose over a tile.
// Include it after mp_jlmath.h (with MPJ_LANE_SAFE as the including file needs it).  Everything has internal linkage.
#pragma once
#include "../../include/mp_jlmath.h"
#include "../../include/mpgpu.h"

namespace {

__device__ __forceinline__ double sat_dp(double mx, double my, double nx, double ny) {
  return __builtin_fma(mx, nx, my * ny);
}

// min / max of two projections in the rectangle tests' inner loop: v_min_f64 / v_max_f64 as they are.  The
// operands come out of an FMA, so they are never signalling NaNs and the instruction alone is IEEE minNum /
// maxNum; __builtin_fmin quiets each operand first (a v_max_f64 x, x apiece: 4 of an edge's 30 fp64 instructions).
__device__ __forceinline__ double dmin(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double dmax(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// GetRectanglePts with cos and sin given: the four distinct corners (the fifth column repeats the first bit
// for bit, so it changes no minimum or maximum and adds a fifth edge equal to none).
__device__ __forceinline__ void rect_pts4(double ox, double oy, double c, double s, double l, double w, double* pts) {
  const double px[4] = {-l, -l, l, l}, py[4] = {w, -w, -w, w};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    pts[2 * j] = __builtin_fma(-s, py[j], c * px[j]) + ox;
    pts[2 * j + 1] = __builtin_fma(c, py[j], s * px[j]) + oy;
  }
}

// Edge e of a rectangle's SAT table: [bx, by, nx, ny, min, max] of its own four projections (utils.jl:41-52).
// A NaN projection makes min and max NaN, as Julia's minimum / maximum do.
__device__ __forceinline__ void rect_edge(const double* q, int e, double* o) {
  const int e1 = (e + 1) & 3;
  const double bx = q[2 * e], by = q[2 * e + 1];
  const double vx = q[2 * e1] - bx, vy = q[2 * e1 + 1] - by;
  const double nx = -vy, ny = vx;
  double d[4];
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = sat_dp(q[2 * j] - bx, q[2 * j + 1] - by, nx, ny);
  double mn = __builtin_fmin(__builtin_fmin(d[0], d[1]), __builtin_fmin(d[2], d[3]));
  double mx = __builtin_fmax(__builtin_fmax(d[0], d[1]), __builtin_fmax(d[2], d[3]));
  if (__builtin_isunordered(d[0], d[1]) | __builtin_isunordered(d[2], d[3])) mn = mx = __builtin_nan("");
  o[0] = bx; o[1] = by; o[2] = nx; o[3] = ny; o[4] = mn; o[5] = mx;
}

// One edge of SeparatingAxisTheorem with the base's part given: does the edge normal separate the four points q?
__device__ __forceinline__ bool edge_separates(double bx, double by, double nx, double ny, double mnb, double mxb,
                                               const double* q) {
  double d[4];
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = sat_dp(q[2 * j] - bx, q[2 * j + 1] - by, nx, ny);
  const double mno = dmin(dmin(d[0], d[1]), dmin(d[2], d[3]));
  const double mxo = dmax(dmax(d[0], d[1]), dmax(d[2], d[3]));
  const bool nan = __builtin_isunordered(d[0], d[1]) | __builtin_isunordered(d[2], d[3]);
  return !nan && ((mxo <= mnb) || (mxb <= mno));
}

// SeparatingAxisTheorem(base, other) with base's table (24 doubles, LDS or registers): the first separating
// edge ends the walk (utils.jl:57-59).
__device__ __forceinline__ bool sat_table(const double* tab, const double* q) {
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const double* o = tab + 6 * e;
    if (edge_separates(o[0], o[1], o[2], o[3], o[4], o[5], q)) return true;
  }
  return false;
}

// ------------------------------------------------------------ walls in LDS tiles, the vehicle in registers
// A wall's row: its 4 corners (8 doubles), then its SAT table, 4 edges x [bx, by, nx, ny, min, max] (24).
constexpr int WALL_ROW = 32;   // doubles per wall row
constexpr int WALL_TILE = 32;  // walls per LDS tile

// Block2Pts of the wall [x, y, yaw, half length, half width] and its SAT table.
__device__ __forceinline__ void wall_row(const double* wall5, double* row) {
  double sw, cw;
  mpj_sincos_bl(wall5[2], &sw, &cw);
  rect_pts4(wall5[0], wall5[1], cw, sw, wall5[3], wall5[4], row);
#pragma unroll
  for (int e = 0; e < 4; e++) rect_edge(row, e, row + 8 + 6 * e);
}

// The rectangle of the vehicle at pose (x, y, ψ) (hybrid_astar_utils.jl:193), its centre `shift` ahead of the
// pose: corners vq[8] and its own SAT table vt[24].
__device__ __forceinline__ void vehicle_rect(double x, double y, double psi, double shift, double half_len,
                                             double half_wid, double* vq, double* vt) {
  double sp, cp, sy, cy;
  mpj_sincos_bl(psi, &sp, &cp);
  const double yaw = mpj_modpi_bl(psi);
  mpj_sincos_bl(yaw, &sy, &cy);
  rect_pts4(x + shift * cp, y + shift * sp, cy, sy, half_len, half_wid, vq);
#pragma unroll
  for (int e = 0; e < 4; e++) rect_edge(vq, e, vt + 6 * e);
}

// The first of a tile's tw wall rows that the vehicle (vq, vt) hits under `mode`, -1 if none:
// ConvexCollision(wall, vehicle), utils.jl:64-74.
__device__ __forceinline__ int tile_first_hit(int mode, const double* wt, int tw, const double* vq,
                                              const double* vt) {
  for (int w = 0; w < tw; w++) {
    const double* row = wt + w * WALL_ROW;  // the same address in every lane: an LDS broadcast
    bool fr = sat_table(row + 8, vq);
    if (mode == MP_SAT_BOTH) {
      if (fr) fr = sat_table(vt, row);
    } else if (mode == MP_SAT_EITHER) {
      if (!fr) fr = sat_table(vt, row);
    }
    if (!fr) return w;
  }
  return -1;
}

}  // namespace
