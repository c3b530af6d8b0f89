// rs_device.hpp — the Reeds–Shepp device code that hastar.hip (Hybrid A*'s RS_connected and rs_heuristic),
// reeds_shepp.hip (the batched Reeds–Shepp module) and roadmap.hip (the roadmap's edges) share: the twelve words as
// one straight-line program (rs_word), the polar forms they start from (rs_pre), the four variants, Julia's findmin
// order and changeBasis (PathPlanning/ReedsSheppsCurves/src/ReedsSheppsUtils.jl); on top of them a candidate's
// command table (rs_cmd_write, rs_cmd_write_tuv), allpath + findmin of a pair in four lanes (rs_pair_best) and
// createPath's three chains (rs_heading_chain, rs_running_sum, rs_step_inc).  Include it after mp_jlmath.h (with
// MPJ_LANE_SAFE as the including file needs it).  Everything has internal linkage, the __constant__ word tables
// included.
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
  if (tuv) {  // the word's segment lengths: with (w, variant) they determine its commands (rs_cmd_write_tuv)
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

// The variant (plain, timeflip, reflect, reverse) of normalised state s that allpath hands to the words.
__device__ __forceinline__ void rs_variant(const double* s, int var, double* q) {
  q[0] = s[0]; q[1] = s[1]; q[2] = s[2];
  if (var == 1) { q[0] = -q[0]; q[2] = -q[2]; }       // timeflip
  else if (var == 2) { q[1] = -q[1]; q[2] = -q[2]; }  // reflect
  else if (var == 3) { q[0] = -q[0]; q[1] = -q[1]; }  // reverse
}

// ------------------------------------------------------------ command tables
// A candidate's command table o[5][3] (distance, gear, steer) with allpath's variant signs (timeflip: gear,
// reflect: steer, reverse: both) from the rows of the plain word that rs_word left in c; rows >= c.n are 0, and all
// rows where !ok (the candidate's cost is Inf).  Every lane forms the rows, the lanes with `store` write them.
__device__ __forceinline__ void rs_cmd_write(const Cmd& c, bool ok, int var, bool store, double* o) {
  const int n = ok ? c.n : 0;
#pragma unroll
  for (int r = 0; r < 5; r++) {
    double tr = 0.0, ge = 0.0, st = 0.0;
    if (r < n) {
      tr = c.tr[r];
      ge = c.ge[r];
      st = c.st[r];
      if (var == 1 || var == 3) ge = -1 * ge;
      if (var == 2 || var == 3) st = -1 * st;
    }
    if (store) {
      o[3 * r] = tr;
      o[3 * r + 1] = ge;
      o[3 * r + 2] = st;
    }
  }
}
// The same table from candidate id = 4(w-1) + variant and the word's (t, u, v), without evaluating the word again:
// the rows it needs come from the word tables (none where !ok), the signs and stores are rs_cmd_write's.
__device__ __forceinline__ void rs_cmd_write_tuv(int id, bool ok, const double* tuv, double* o) {
  const int wi = id >> 2;
  Cmd c;
  c.n = ok ? kRsN[wi] : 0;
#pragma unroll
  for (int r = 0; r < 5; r++)
    if (r < c.n) {
      const int code = kRsTr[wi][r];
      c.tr[r] = code == 0 ? tuv[0] : code == 1 ? tuv[1] : code == 2 ? tuv[2] : PI2;
      c.ge[r] = kRsGe[wi][r];
      c.st[r] = kRsSt[wi][r];
    }
  rs_cmd_write(c, ok, id & 3, true, o);
}

// ------------------------------------------------------------ allpath + findmin
// allpath + findmin (ReedsSheppsUtils.jl:383-436, hybrid_astar_utils.jl rs_heuristic / RS_connected) of one pose
// pair, normalised state s, in the four lanes 4j..4j+3 of a wave: lane & 3 = var is the variant of candidate
// id = 4(w-1) + var, and the word loop is wave-uniform (no divergent 12-way switch).  The winner's cost and id come
// back in all four lanes (rs_before is a total order, so per lane then across lanes finds allpath's winner) and,
// when TUV, so do its word's (t, u, v).  Where `live`, every candidate's cost goes to cost[48] (may be null) and,
// when WC, its command table to cmds[48][5][3].
template <bool WC, bool TUV>
__device__ __forceinline__ void rs_pair_best(const double* s, int var, bool live, double* __restrict__ cost,
                                             double* __restrict__ cmds, double* bc_out, int* bi_out,
                                             double* tuv_out) {
  double q[3];
  rs_variant(s, var, q);
  const RsPre R = rs_pre(q);
  double bc = __builtin_inf();
  int bi = 1 << 20;
  double bt[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
  for (int w = 1; w <= 12; w++) {
    Cmd c;
    double tv[3];
    const double cst = rs_word(w, R, WC ? &c : nullptr, TUV ? tv : nullptr);
    const int id = 4 * (w - 1) + var;
    if (rs_before(cst, id, bc, bi)) {
      bc = cst;
      bi = id;
      if (TUV) { bt[0] = tv[0]; bt[1] = tv[1]; bt[2] = tv[2]; }
    }
    if (live && cost) cost[id] = cst;
    if (WC && live) rs_cmd_write(c, cst < __builtin_inf(), var, true, cmds + id * 15);
  }
#pragma unroll
  for (int o = 2; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(bc, o);
    const int oi = __shfl_xor(bi, o);
    double ot[3] = {0.0, 0.0, 0.0};
    if (TUV) {
      ot[0] = __shfl_xor(bt[0], o);
      ot[1] = __shfl_xor(bt[1], o);
      ot[2] = __shfl_xor(bt[2], o);
    }
    if (rs_before(ov, oi, bc, bi)) {
      bc = ov;
      bi = oi;
      if (TUV) { bt[0] = ot[0]; bt[1] = ot[1]; bt[2] = ot[2]; }
    }
  }
  *bc_out = bc;
  *bi_out = bi;
  if (TUV) { tuv_out[0] = bt[0]; tuv_out[1] = bt[1]; tuv_out[2] = bt[2]; }
}

// ------------------------------------------------------------ createPath
// createPath / createActPath (ReedsSheppsUtils.jl:411-466; operand order of the oracle's or_ha_act_path), a block
// of RS_PT command tables segment by segment over LDS rows of RS_PST doubles.  Three serial chains, each kept in
// order for the bits of the reference; cm = the segment's command row (distance, gear, steer).  The closed form of
// repeated addition (mpj_rep_add_ok) is not used here: see DESIGN.md.
constexpr int RS_PT = 16;    // paths per block
constexpr int RS_PST = 101;  // LDS row stride in doubles (100 steps + 1: ψ_0..ψ_100; odd against bank conflicts)

// The heading recurrence ψ_{k+1} = ψ_k + (steer*gear)*Δt from ψ_0 = q into psi[0..100]; returns ψ_100.
__device__ __forceinline__ double rs_heading_chain(const double* cm, double q, double* psi) {
  const double dt = __builtin_fabs(cm[0]) / 100;
  const double c = (cm[2] * cm[1]) * dt;
  psi[0] = q;
  for (int k = 0; k < 100; k++) {
    q = q + c;
    psi[k + 1] = q;
  }
  return q;
}

// The running sum of a segment's 100 increments from acc, in place over them; returns the last.  Batches of 20
// increments into registers first, so the LDS reads pipeline ahead of the chain.
__device__ __forceinline__ double rs_running_sum(double* inc, double acc) {
  for (int u0 = 0; u0 < 100; u0 += 20) {
    double v[20];
#pragma unroll
    for (int u = 0; u < 20; u++) v[u] = inc[u0 + u];
#pragma unroll
    for (int u = 0; u < 20; u++) {
      acc = acc + v[u];
      inc[u0 + u] = acc;
    }
  }
  return acc;
}

// One step's increments ((gear*cos ψ)*minR)*Δt, ((gear*sin ψ)*minR)*Δt.
__device__ __forceinline__ void rs_step_inc(const double* cm, double psi, double minR, double* dx, double* dy) {
  const double dt = __builtin_fabs(cm[0]) / 100, v = cm[1];
  double sn, cs;
  mpj_sincos_bl(psi, &sn, &cs);
  double d0 = v * cs, d1 = v * sn;
  d0 = d0 * minR;
  d1 = d1 * minR;
  *dx = d0 * dt;
  *dy = d1 * dt;
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
