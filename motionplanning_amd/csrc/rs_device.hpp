// rs_device.hpp — the Reeds–Shepp device code that hastar.hip (Hybrid A*'s RS_connected and rs_heuristic) and
// reeds_shepp.hip (the batched Reeds–Shepp module) share: the twelve words as one straight-line program (rs_word),
// the polar forms they start from (rs_pre), the four variants, Julia's findmin order and changeBasis
// (PathPlanning/ReedsSheppsCurves/src/ReedsSheppsUtils.jl).  Include it after mp_jlmath.h (with MPJ_LANE_SAFE as the
// including file needs it).  Everything has internal linkage, the __constant__ word tables included.
#pragma once
#include "../../include/mp_jlmath.h"

namespace {

constexpr double PI2 = MPJ_PI / 2;

// ------------------------------------------------------------ Reeds–Shepp
__device__ __forceinline__ void polar(double a, double b, double* r, double* th) {
  *r = mpj_sqrt(a * a + b * b);
  *th = mpj_atan2_bl(b, a);
}

struct Cmd {
  int n;
  double tr[5], ge[5], st[5];
};

// The two polar forms every RS word starts from (ReedsSheppsUtils.jl path1..12):
// A = polar(x - sin p, y - 1 + cos p), B = polar(x + sin p, y - 1 - cos p).  Computed once
// per candidate variant instead of once per word (same operands, same bits).
struct RsPre {
  double p, rA, tA, rB, tB;
};
__device__ __forceinline__ RsPre rs_pre(const double* q) {
  double sp, cp;
  mpj_sincos_bl(q[2], &sp, &cp);
  RsPre R;
  R.p = q[2];
  polar(q[0] - sp, q[1] - 1 + cp, &R.rA, &R.tA);
  polar(q[0] + sp, q[1] - 1 - cp, &R.rB, &R.tB);
  return R;
}

__device__ __forceinline__ double fin(double t, double u, double v, double cost) {
  if ((t < 0) || (v < 0) || (u < 0)) return __builtin_inf();
  return cost;
}

// Reeds–Shepp words path1..path12 (ReedsSheppsUtils.jl:48-380): rs_word below.

// One Reeds–Shepp word w (wave-uniform) as ONE straight-line program: each transcendental
// (sqrt, acos, sin, asin, atan2) and the three modπ appear once, guarded by uniform branches
// on w, with word-selected operands — the same operations on the same operands as the
// reference words and oracle/or_hastar.c rs_path (bit-identical), but one copy of the code
// instead of twelve inlined word bodies (which overflowed the instruction cache).
__constant__ signed char kRsGe[12][5] = {{1, 1, 1}, {1, 1, 1}, {1, -1, 1}, {1, -1, -1}, {1, 1, -1},
                                         {1, 1, -1, -1}, {1, -1, -1, 1}, {1, -1, -1, -1}, {1, 1, 1, -1},
                                         {1, -1, -1, -1}, {1, 1, 1, -1}, {1, -1, -1, -1, 1}};
__constant__ signed char kRsSt[12][5] = {{1, 0, 1}, {1, 0, -1}, {1, -1, 1}, {1, -1, 1}, {1, -1, 1},
                                         {1, -1, 1, -1}, {1, -1, 1, -1}, {1, -1, 0, 1}, {1, 0, -1, 1},
                                         {1, -1, 0, -1}, {1, 0, 1, -1}, {1, -1, 0, 1, -1}};
// command lengths as: 0 t, 1 u, 2 v, 3 π/2
__constant__ signed char kRsTr[12][5] = {{0, 1, 2}, {0, 1, 2}, {0, 1, 2}, {0, 1, 2}, {0, 1, 2},
                                         {0, 1, 1, 2}, {0, 1, 1, 2}, {0, 3, 1, 2}, {0, 1, 3, 2},
                                         {0, 3, 1, 2}, {0, 1, 3, 2}, {0, 3, 1, 3, 2}};
__constant__ signed char kRsN[12] = {3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 5};

__device__ __forceinline__ double rs_word(int w_, const RsPre& R, Cmd* c, double* tuv = nullptr) {
  const int w = __builtin_amdgcn_readfirstlane(w_);  // wave-uniform word: scalar branches and table loads
  const double p = R.p;
  const bool useA = (w == 1) | (w == 3) | (w == 4) | (w == 5) | (w == 8) | (w == 9);
  const double rho = useA ? R.rA : R.rB, th = useA ? R.tA : R.tB;
  const double r2 = rho * rho;
  double sq = 0.0, ang = 0.0, ac = 0.0;
  if (w == 2 || w == 8 || w == 9 || w == 12) sq = mpj_sqrt(r2 - 4);
  double u;  // words 1, 2, 8-12: direct; 3-7: below
  if (w == 1) u = rho;
  else if (w == 2) u = sq;
  else if (w == 8 || w == 9) u = sq - 2;
  else if (w == 10 || w == 11) u = rho - 2;
  else if (w == 12) u = sq - 4;
  else u = 0.0;
  const double u1 = (20 - r2) / 16;
  if (w >= 3 && w <= 7) {
    double arg;
    if (w <= 4) arg = rho / 4;
    else if (w == 5) arg = 1 - r2 / 8;
    else if (w == 6) arg = rho <= 2 ? (rho + 2) / 4 : (rho - 2) / 4;
    else arg = u1;
    ac = mpj_acos(arg);
  }
  if (w == 5 || w == 7) {
    u = ac;
    ang = mpj_asin(2 * mpj_sin(u) / rho);
  } else if (w == 2 || w == 8 || w == 9 || w == 12) {
    double y, x;
    if (w == 2) { y = 2; x = u; }
    else if (w == 8) { y = 2; x = u + 2; }
    else if (w == 9) { y = u + 2; x = 2; }
    else { y = 2; x = u + 4; }
    ang = mpj_atan2_bl(y, x);
  } else if (w >= 3 && w <= 6) {
    ang = ac;
  }
  // t = modπ(targ)   (word 1: t = θ, and modπ(θ) == θ for θ = atan2(...) ∈ [-π, π])
  double targ;
  if (w == 1 || w == 11) targ = th;
  else if (w == 2) targ = th + ang;
  else if (w == 10) targ = th + PI2;
  else if (w == 5 || w == 9 || (w == 6 && !(rho <= 2))) targ = th + PI2 - ang;
  else targ = th + PI2 + ang;
  const double t = mpj_modpi_bl(targ);
  if (w == 3 || w == 4 || w == 6) {  // u = modπ(π - 2a) / modπ(a) / modπ(π - a)
    const double uarg = (w == 6) ? (rho <= 2 ? ang : MPJ_PI - ang) : MPJ_PI - 2 * ang;
    u = mpj_modpi_bl(uarg);
  }
  double varg;
  if (w == 1 || w == 10 || w == 11) varg = (w == 1) ? p - t : p - t - PI2;
  else if (w == 2 || w == 7 || w == 12) varg = t - p;
  else if (w == 3) varg = p - t - u;
  else if (w == 4) varg = t + u - p;
  else if (w == 5) varg = t - p - u;
  else if (w == 6) varg = p - t + 2 * u;
  else if (w == 8) varg = t - p + PI2;
  else varg = t - p - PI2;  // w == 9
  const double v = mpj_modpi_bl(varg);
  const double at = __builtin_fabs(t), au = __builtin_fabs(u), av = __builtin_fabs(v);
  double cost;
  if (w <= 5) cost = at + au + av;
  else if (w <= 7) cost = at + 2 * au + av;
  else if (w == 8) cost = at + PI2 + au + av;
  else if (w <= 11) cost = at + au + PI2 + av;
  else cost = at + PI2 + au + PI2 + av;
  bool valid;
  if (w == 1) valid = true;
  else if (w == 2 || (w >= 8 && w <= 11)) valid = rho >= 2;
  else if (w <= 6) valid = rho <= 4;
  else if (w == 7) valid = (rho <= 6) && (0 <= u1) && (u1 <= 1);
  else valid = rho >= 4;
  if (tuv) {  // the word's segment lengths: with (w, variant) they determine its commands (cmd_from_tuv)
    tuv[0] = t;
    tuv[1] = u;
    tuv[2] = v;
  }
  if (c) {
    const int wi = w - 1;
    c->n = kRsN[wi];
#pragma unroll
    for (int r = 0; r < 5; r++) {
      const int code = kRsTr[wi][r];
      c->tr[r] = code == 0 ? t : code == 1 ? u : code == 2 ? v : PI2;
      c->ge[r] = kRsGe[wi][r];
      c->st[r] = kRsSt[wi][r];
    }
  }
  return valid ? fin(t, u, v, cost) : __builtin_inf();
}

// Julia findmin order on (cost, candidate id): NaN first (lowest id among NaNs), else the
// smallest cost, ties to the lowest id.  A total order, so per-lane then cross-lane
// reduction gives the same winner as allpath's sequential findmin.
__device__ __forceinline__ bool rs_before(double a, int ia, double b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an && bn) return ia < ib;
  if (an) return true;
  if (bn) return false;
  return (a < b) || (a == b && ia < ib);
}

// allpath + findmin (ReedsSheppsUtils.jl:383-436, hybrid_astar_utils.jl rs_heuristic /
// RS_connected).  The word loop is wave-uniform (no divergent 12-way switch): lane&3 is
// the variant (plain, timeflip, reflect, reverse) of candidate id = 4(w-1)+variant.
// Returns the winning cost in every lane; *best_id = winning id; if cm != nullptr the
// winner's commands [5][3] (distance, gear, steer) are written to cm (LDS) by one lane.
__device__ __forceinline__ void rs_variant(const double* s, int var, double* q) {
  q[0] = s[0]; q[1] = s[1]; q[2] = s[2];
  if (var == 1) { q[0] = -q[0]; q[2] = -q[2]; }       // timeflip
  else if (var == 2) { q[1] = -q[1]; q[2] = -q[2]; }  // reflect
  else if (var == 3) { q[0] = -q[0]; q[1] = -q[1]; }  // reverse
}

// changeBasis with sin/cos of init's heading given (the lattice-heading tables)
__device__ __forceinline__ void change_basis_sc(const double* init, const double* term, double minR, double s0,
                                                double c0, double* out) {
  const double p0 = init[2], pg = term[2];
  const double dx = (term[0] - init[0]) / minR, dy = (term[1] - init[1]) / minR;
  out[0] = dx * c0 + dy * s0;
  out[1] = -dx * s0 + dy * c0;
  out[2] = pg - p0;
}
__device__ __forceinline__ void change_basis(const double* init, const double* term, double minR, double* out) {
  const double p0 = init[2], pg = term[2];
  const double dx = (term[0] - init[0]) / minR, dy = (term[1] - init[1]) / minR;
  double s0, c0;
  mpj_sincos_bl(p0, &s0, &c0);
  out[0] = dx * c0 + dy * s0;
  out[1] = -dx * s0 + dy * c0;
  out[2] = pg - p0;
}

}  // namespace
