// reeds_shepp.hip — the batched Reeds–Shepp module for gfx950 (PathPlanning/ReedsSheppsCurves/main.jl and
// src/ReedsSheppsUtils.jl; rs_heuristic of HybridAstar/src/hybrid_astar_utils.jl:361-373) + C-ABI.
//
// rs_allpath_kernel  changeBasis + allpath + findmin for B pose pairs: 16 pairs per wave, lanes 4j..4j+3 = the four
//                    variants of pair j, the word loop wave-uniform (rs_pair_best of rs_device.hpp); the norm and
//                    command stores are optional.
// rs_matrix_kernel   the Reeds–Shepp distance of every (a_i, b_j): the same lane layout, a wave's 16 pairs along b,
//                    no command stores (8 B + 1 optional byte per pair), sin/cos of a_i's heading once per block.
// rs_path_kernel     createPath / createActPath for n command tables: a block takes RS_PT paths segment by segment --
//                    the heading recurrence and the x / y running sums one lane per chain, the 100 sincos and
//                    increments of a segment one thread per (path, step), turned through LDS in between (the three
//                    chains are rs_device.hpp's).
#include <cstdint>

// the libm routines run under divergent control flow here (tails, ragged tiles): lane-safe variants
#define MPJ_LANE_SAFE 1
#include "../../include/mp_jlmath.h"
#include "rs_device.hpp"
#include "runtime.hpp"

namespace {

constexpr int RS_NCAND = 48;
constexpr int RS_MAXPATH = 501;  // 100 * 5 segments + 1
constexpr int RS_MT = 256;       // rs_matrix_kernel: threads per block = 64 pairs along b
constexpr int RS_PTH = 256;      // rs_path_kernel: threads per block (RS_PT paths, rs_device.hpp)

// main.jl:15-17 for B pose pairs.  norm may be null; cmds is written when WC.
template <bool WC>
__global__ __launch_bounds__(64) void rs_allpath_kernel(int B, const double* __restrict__ init,
                                                        const double* __restrict__ term,
                                                        const double* __restrict__ minR, double* __restrict__ norm,
                                                        double* __restrict__ cost, double* __restrict__ cmds,
                                                        int* __restrict__ best, double* __restrict__ act_cost) {
  const int lane = threadIdx.x, var = lane & 3;
  const int b = blockIdx.x * 16 + (lane >> 2);
  const bool live = b < B;
  double s[3] = {0.0, 0.0, 0.0};
  double mr = 1.0;
  if (live) {
    mr = minR[b];
    change_basis(init + 3 * (size_t)b, term + 3 * (size_t)b, mr, s);
    if (norm && var == 0) {
      norm[3 * (size_t)b] = s[0];
      norm[3 * (size_t)b + 1] = s[1];
      norm[3 * (size_t)b + 2] = s[2];
    }
  }
  double bc;
  int bi;
  rs_pair_best<WC, false>(s, var, live, cost + (size_t)(live ? b : 0) * RS_NCAND,
                          WC ? cmds + (size_t)(live ? b : 0) * RS_NCAND * 15 : nullptr, &bc, &bi, nullptr);
  if (live && var == 0) {
    best[b] = bi;
    act_cost[b] = bc * mr;
  }
}

// dist[na][nb] = opt_cost * minR of (a_i -> b_j), best[na][nb] (may be null) the winning candidate.  Block
// (row i, chunk c) takes the 64-pair tiles c, c + nchunk, ... of row i: a wave's 16 pairs are consecutive j, so the
// var == 0 lanes store 16 consecutive doubles.
__global__ __launch_bounds__(RS_MT) void rs_matrix_kernel(int na, int nb, int nchunk, const double* __restrict__ a,
                                                          const double* __restrict__ b, double minR,
                                                          double* __restrict__ dist, uint8_t* __restrict__ best) {
  const int i = blockIdx.x / nchunk, chunk = blockIdx.x - i * nchunk;
  const int var = threadIdx.x & 3;
  const double ai[3] = {a[3 * (size_t)i], a[3 * (size_t)i + 1], a[3 * (size_t)i + 2]};
  double s0, c0;
  mpj_sincos_bl(ai[2], &s0, &c0);  // row a's heading: once per block, for every tile of the row it takes
  const int ntile = (nb + 63) / 64;
  for (int t = chunk; t < ntile; t += nchunk) {
    const int j = t * 64 + (threadIdx.x >> 2);
    const bool live = j < nb;
    double s[3] = {0.0, 0.0, 0.0};
    if (live) {
      const double bj[3] = {b[3 * (size_t)j], b[3 * (size_t)j + 1], b[3 * (size_t)j + 2]};
      change_basis_sc(ai, bj, minR, s0, c0, s);
    }
    double bc;
    int bi;
    rs_pair_best<false, false>(s, var, false, nullptr, nullptr, &bc, &bi, nullptr);
    if (live && var == 0) {
      const size_t o = (size_t)i * nb + j;
      dist[o] = bc * minR;
      if (best) best[o] = (uint8_t)bi;
    }
  }
}

// createPath / createActPath (ReedsSheppsUtils.jl:411-466; operand order of the oracle's or_ha_act_path) for the
// command tables cmds[n][5][3].  Block = RS_PT paths, segment by segment; per segment s
//   phase A  lane p of wave 0: the heading recurrence ψ_{k+1} = ψ_k + (steer*gear)*Δt of segment s into psi_s[p];
//            lane 2p+c of wave 1: the running sum x (c = 0) / y (c = 1) of segment s-1, in place over its increments;
//   phase B  thread per (path, step k): stores x, y of column 100(s-1)+k+1, then sincos(ψ_k) and the increments
//            ((gear*cos ψ)*minR)*Δt, ((gear*sin ψ)*minR)*Δt of segment s into the same slot, and stores ψ_{k+1}.
// The three chains (rs_heading_chain, rs_running_sum, rs_step_inc) stay serial and in order; a path with fewer
// segments sits out the later rounds.  Consecutive threads hold consecutive steps of a path, so a wave's stores cover
// one contiguous piece of the path's row.
__global__ __launch_bounds__(RS_PTH) void rs_path_kernel(long long n, const double* __restrict__ init,
                                                         const double* __restrict__ minR,
                                                         const double* __restrict__ cmds, double* __restrict__ path,
                                                         int* __restrict__ path_len) {
  __shared__ double psi_s[RS_PT][RS_PST], xs_s[RS_PT][RS_PST], ys_s[RS_PT][RS_PST];
  __shared__ double cur_s[RS_PT][3], mr_s[RS_PT];
  __shared__ int nseg_s[RS_PT];
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * RS_PT;
  const int np = (int)((n - p0) < RS_PT ? (n - p0) : RS_PT);
  if (tid < RS_PT) {
    int ns = 0;
    double st[3] = {0.0, 0.0, 0.0}, mr = 1.0;
    if (tid < np) {
      const size_t g = (size_t)(p0 + tid);
      const double* cm = cmds + g * 15;
      for (int r = 0; r < 5; r++) {
        if (cm[3 * r + 1] == 0) break;
        ns++;
      }
      if (init) {
        st[0] = init[3 * g];
        st[1] = init[3 * g + 1];
        st[2] = init[3 * g + 2];
        mr = minR[g];
      }
      double* o = path + g * (RS_MAXPATH * 3);
      o[0] = st[0];
      o[1] = st[1];
      o[2] = st[2];
      path_len[g] = 100 * ns + 1;
    }
    nseg_s[tid] = ns;
    cur_s[tid][0] = st[0];
    cur_s[tid][1] = st[1];
    cur_s[tid][2] = st[2];
    mr_s[tid] = mr;
  }
  __syncthreads();
  int mx = 0;
  for (int p = 0; p < RS_PT; p++) mx = nseg_s[p] > mx ? nseg_s[p] : mx;
  for (int s = 0; s <= mx; s++) {
    // ---- phase A: the serial chains, one lane each
    if (tid < RS_PT) {
      const int p = tid;
      if (s < nseg_s[p])
        cur_s[p][2] = rs_heading_chain(cmds + (size_t)(p0 + p) * 15 + 3 * s, cur_s[p][2], psi_s[p]);
    } else if (tid >= 64 && tid < 64 + 2 * RS_PT) {
      const int p = (tid - 64) >> 1, c = (tid - 64) & 1;
      if (s >= 1 && s - 1 < nseg_s[p]) cur_s[p][c] = rs_running_sum(c == 0 ? xs_s[p] : ys_s[p], cur_s[p][c]);
    }
    __syncthreads();
    // ---- phase B: one thread per (path, step)
    for (int i = tid; i < RS_PT * 100; i += RS_PTH) {
      const int p = i / 100, k = i - 100 * p;
      const int ns = nseg_s[p];
      double* row = path + (size_t)(p0 + p) * (RS_MAXPATH * 3);
      if (s >= 1 && s - 1 < ns) {
        double* o = row + 3 * (100 * (s - 1) + k + 1);
        o[0] = xs_s[p][k];
        o[1] = ys_s[p][k];
      }
      if (s < ns) {
        rs_step_inc(cmds + (size_t)(p0 + p) * 15 + 3 * s, psi_s[p][k], mr_s[p], &xs_s[p][k], &ys_s[p][k]);
        row[3 * (100 * s + k + 1) + 2] = psi_s[p][k + 1];
      }
    }
    __syncthreads();
  }
  // columns from path_len on are 0.0
  for (int p = 0; p < np; p++) {
    double* row = path + (size_t)(p0 + p) * (RS_MAXPATH * 3);
    for (int e = 3 * (100 * nseg_s[p] + 1) + tid; e < RS_MAXPATH * 3; e += RS_PTH) row[e] = 0.0;
  }
}

}  // namespace

extern "C" {

int mp_rs_allpath(mp_ctx* ctx, int32_t B, const double* init, const double* term, const double* minR, double* norm,
                  double* cost, double* cmds, int32_t* best, double* act_cost) {
  if (!ctx) return mp_fail(nullptr, MP_ERR_INVALID, "mp_rs_allpath: NULL context");
  MP_CHECK(ctx, B >= 1, "mp_rs_allpath: B (%d) must be >= 1", B);
  MP_CHECK(ctx, init && term && minR && cost && best && act_cost, "mp_rs_allpath: NULL argument");
  MP_HIP(ctx, hipSetDevice(ctx->device));
  int st = MP_OK;
  const size_t nB = (size_t)B;
  const double* dinit = mp_upload(ctx, WS_IO0, init, 3 * nB, &st);
  const double* dterm = mp_upload(ctx, WS_IO1, term, 3 * nB, &st);
  const double* dminR = mp_upload(ctx, WS_IO2, minR, nB, &st);
  double* dnorm = mp_alloc_out(ctx, WS_IO3, norm, 3 * nB, &st);
  double* dcost = mp_alloc_out(ctx, WS_IO4, cost, RS_NCAND * nB, &st);
  double* dcmds = mp_alloc_out(ctx, WS_IO5, cmds, RS_NCAND * 15 * nB, &st);
  int32_t* dbest = mp_alloc_out(ctx, WS_IO6, best, nB, &st);
  double* dact = mp_alloc_out(ctx, WS_IO7, act_cost, nB, &st);
  if (st) return st;
  mp_time_begin(ctx);
  const dim3 grid((unsigned)((B + 15) / 16));
  if (dcmds)
    hipLaunchKernelGGL(rs_allpath_kernel<true>, grid, dim3(64), 0, ctx->stream, B, dinit, dterm, dminR, dnorm, dcost,
                       dcmds, (int*)dbest, dact);
  else
    hipLaunchKernelGGL(rs_allpath_kernel<false>, grid, dim3(64), 0, ctx->stream, B, dinit, dterm, dminR, dnorm, dcost,
                       dcmds, (int*)dbest, dact);
  MP_HIP(ctx, hipGetLastError());
  mp_time_end(ctx);
  if ((st = mp_download(ctx, norm, (const double*)dnorm, 3 * nB))) return st;
  if ((st = mp_download(ctx, cost, (const double*)dcost, RS_NCAND * nB))) return st;
  if ((st = mp_download(ctx, cmds, (const double*)dcmds, RS_NCAND * 15 * nB))) return st;
  if ((st = mp_download(ctx, best, (const int32_t*)dbest, nB))) return st;
  if ((st = mp_download(ctx, act_cost, (const double*)dact, nB))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

int mp_rs_create_path(mp_ctx* ctx, int64_t n, const double* init, const double* minR, const double* cmds,
                      double* path, int32_t* path_len) {
  if (!ctx) return mp_fail(nullptr, MP_ERR_INVALID, "mp_rs_create_path: NULL context");
  MP_CHECK(ctx, n >= 1, "mp_rs_create_path: n (%lld) must be >= 1", (long long)n);
  MP_CHECK(ctx, n <= ((int64_t)1 << 31) - 1, "mp_rs_create_path: n (%lld) above 2^31 - 1", (long long)n);
  MP_CHECK(ctx, cmds && path && path_len, "mp_rs_create_path: NULL argument");
  MP_CHECK(ctx, (init != nullptr) == (minR != nullptr),
           "mp_rs_create_path: init and minR go together (both: createActPath, neither: createPath)");
  MP_HIP(ctx, hipSetDevice(ctx->device));
  int st = MP_OK;
  const size_t N = (size_t)n;
  const double* dinit = mp_upload(ctx, WS_IO0, init, 3 * N, &st);
  const double* dminR = mp_upload(ctx, WS_IO1, minR, N, &st);
  const double* dcmds = mp_upload(ctx, WS_IO2, cmds, 15 * N, &st);
  double* dpath = mp_alloc_out(ctx, WS_IO3, path, (size_t)RS_MAXPATH * 3 * N, &st);
  int32_t* dlen = mp_alloc_out(ctx, WS_IO4, path_len, N, &st);
  if (st) return st;
  mp_time_begin(ctx);
  hipLaunchKernelGGL(rs_path_kernel, dim3((unsigned)((n + RS_PT - 1) / RS_PT)), dim3(RS_PTH), 0, ctx->stream,
                     (long long)n, dinit, dminR, dcmds, dpath, (int*)dlen);
  MP_HIP(ctx, hipGetLastError());
  mp_time_end(ctx);
  if ((st = mp_download(ctx, path, (const double*)dpath, (size_t)RS_MAXPATH * 3 * N))) return st;
  if ((st = mp_download(ctx, path_len, (const int32_t*)dlen, N))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

int mp_rs_cost_matrix(mp_ctx* ctx, int32_t na, const double* a, int32_t nb, const double* b, double minR,
                      double* dist, uint8_t* best) {
  if (!ctx) return mp_fail(nullptr, MP_ERR_INVALID, "mp_rs_cost_matrix: NULL context");
  MP_CHECK(ctx, na >= 1 && nb >= 1, "mp_rs_cost_matrix: na (%d) and nb (%d) must be >= 1", na, nb);
  MP_CHECK(ctx, a && b && dist, "mp_rs_cost_matrix: NULL argument");
  // a block takes 2, 4 or 8 of a row's 64-pair tiles while the grid still holds 2048 blocks (8 per CU)
  const long long ntile = ((long long)nb + 63) / 64;
  long long nchunk = ntile;
  for (int per = 2; per <= 8 && (long long)na * ((ntile + per - 1) / per) >= 2048; per *= 2)
    nchunk = (ntile + per - 1) / per;
  MP_CHECK(ctx, (long long)na * nchunk <= 0x7fffffffll, "mp_rs_cost_matrix: %d x %d pairs are too many for one call",
           na, nb);
  MP_HIP(ctx, hipSetDevice(ctx->device));
  int st = MP_OK;
  const size_t np = (size_t)na * (size_t)nb;
  const double* da = mp_upload(ctx, WS_IO0, a, 3 * (size_t)na, &st);
  const double* db = mp_upload(ctx, WS_IO1, b, 3 * (size_t)nb, &st);
  double* ddist = mp_alloc_out(ctx, WS_IO2, dist, np, &st);
  uint8_t* dbest = mp_alloc_out(ctx, WS_IO3, best, np, &st);
  if (st) return st;
  mp_time_begin(ctx);
  hipLaunchKernelGGL(rs_matrix_kernel, dim3((unsigned)(na * nchunk)), dim3(RS_MT), 0, ctx->stream, (int)na, (int)nb,
                     (int)nchunk, da, db, minR, ddist, dbest);
  MP_HIP(ctx, hipGetLastError());
  mp_time_end(ctx);
  if ((st = mp_download(ctx, dist, (const double*)ddist, np))) return st;
  if ((st = mp_download(ctx, best, (const uint8_t*)dbest, np))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

}  // extern "C"
