// roadmap.hip — a multi-query roadmap planner under the Reeds–Shepp metric (PRM for a car) for gfx950 + C-ABI.
// A build extension: every edge is RS_connected (HybridAstar/src/hybrid_astar_utils.jl:224-233) of a pose pair, the
// distance is rs_heuristic's opt_cost*minR (:361-373); the graph layer on top has no counterpart in the reference.
//
// rm_wall_kernel      Block2Pts of the scene's walls and each wall's SAT table, once per call: wtab[n_walls][32]
//                     (wall_row of collide_device.hpp).
// rm_rank_kernel      block per row: the row's n distances (lanes 4j..4j+3 = the four variants of column j,
//                     rs_pair_best) stay in LDS, then k block-wide argmins on (d, j) pick the candidates in rank
//                     order.  mode 0 ranks d(row -> j), mode 1 d(j -> row) (the goal's columns: changeBasis is not
//                     symmetric bit for bit).  It also writes the candidates as a pair list for rm_connect_kernel.
// rm_connect_kernel   RS_connected for a pair list, RS_PT pairs per block: wave 0 finds each pair's winner and rebuilds
//                     its command table from (word, variant, t, u, v); then createPath's chains with the path in LDS
//                     only -- the serial ψ / x / y chains one lane each, the 100 sincos and increments of a segment
//                     one thread per (path, step) -- and after each segment's running sums land, its 20 columns
//                     = 0 (mod 5) are tested against the walls (LDS tiles of WALL_TILE rows of wtab).  A hit pair sits out
//                     the later segments.  One double per pair leaves the kernel: d where free, +Inf where blocked.
// rm_dijkstra_kernel  block per query over vertices 0 = start, 1..n = nodes, n + 1 = goal: dist, parent and the settled
//                     flags in LDS, per round a block-wide argmin on (dist, vertex), then one thread per out-edge.
#include <climits>
#include <cmath>
#include <vector>

// divergent control flow around the libm calls (ragged tiles, hit pairs, inactive poses): lane-safe variants
#define MPJ_LANE_SAFE 1
#include "../../include/mp_jlmath.h"
#include "collide_device.hpp"
#include "rs_device.hpp"
#include "runtime.hpp"

namespace {

constexpr int RM_MAXN = MP_ROADMAP_MAX_NODES;
constexpr int RM_RT = 256;    // rm_rank_kernel: threads per block = 64 columns per tile
// rm_connect_kernel: RS_PT pairs per block in LDS rows of RS_PST (rs_device.hpp), walls in tiles of WALL_TILE rows of
// WALL_ROW doubles (collide_device.hpp)
constexpr int RM_CT = 320;    // ... threads per block: RS_PT * RM_NCHK checked poses, 5 passes over RS_PT * 100 steps
constexpr int RM_NCHK = 20;   // ... checked columns per segment: steps 4, 9, ..., 99 are path columns = 0 (mod 5)
constexpr int RM_DT = 256;    // rm_dijkstra_kernel: threads per block

__device__ __forceinline__ bool rm_finite(double d) { return __builtin_fabs(d) < __builtin_inf(); }

// The lowest (d, i) of a block of T threads, in every thread.  The caller synchronises before the next call.
template <int T>
__device__ __forceinline__ void block_argmin(double& d, int& i, double* red_d, int* red_i) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double od = __shfl_xor(d, o);
    const int oi = __shfl_xor(i, o);
    if (od < d || (od == d && oi < i)) { d = od; i = oi; }
  }
  if ((threadIdx.x & 63) == 0) {
    red_d[threadIdx.x >> 6] = d;
    red_i[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  d = red_d[0];
  i = red_i[0];
#pragma unroll
  for (int w = 1; w < T / 64; w++) {
    const double od = red_d[w];
    const int oi = red_i[w];
    if (od < d || (od == d && oi < i)) { d = od; i = oi; }
  }
}

// -------------------------------------------------------------------- walls
__global__ __launch_bounds__(64) void rm_wall_kernel(int nw, const double* __restrict__ walls,
                                                     double* __restrict__ wtab) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= nw) return;
  double row[WALL_ROW];
  wall_row(walls + 5 * (size_t)i, row);
  double* o = wtab + (size_t)i * WALL_ROW;
#pragma unroll
  for (int j = 0; j < WALL_ROW; j++) o[j] = row[j];
}

// -------------------------------------------------------------------- candidates
// P is the pose table (columns 0..n-1 are the nodes); row r is pose row_base + r.  Row r's k candidates in rank order
// go to nbr[r][k] (-1 past the last) and, as pose-table indices (from, to), to pa / pb[r][k] (-1, -1 for padding).
// excl_self: column r is no candidate of row r (a build's rows are the nodes themselves).
__global__ __launch_bounds__(RM_RT) void rm_rank_kernel(int n, int k, int mode, int row_base, int excl_self,
                                                        const double* __restrict__ P, double minR,
                                                        int* __restrict__ nbr, int* __restrict__ pa,
                                                        int* __restrict__ pb) {
  __shared__ double d_s[RM_MAXN];
  __shared__ double red_d[RM_RT / 64];
  __shared__ int red_i[RM_RT / 64];
  const int r = blockIdx.x, tid = threadIdx.x, var = tid & 3;
  const int ri = row_base + r;
  const double a[3] = {P[3 * (size_t)ri], P[3 * (size_t)ri + 1], P[3 * (size_t)ri + 2]};
  double s0, c0;
  mpj_sincos_bl(a[2], &s0, &c0);
  const int ntile = (n + 63) / 64;
  for (int t = 0; t < ntile; t++) {
    const int j = t * 64 + (tid >> 2);
    const bool live = j < n;
    double s[3] = {0.0, 0.0, 0.0};
    if (live) {
      const double b[3] = {P[3 * (size_t)j], P[3 * (size_t)j + 1], P[3 * (size_t)j + 2]};
      if (mode == 0) change_basis_sc(a, b, minR, s0, c0, s);
      else change_basis(b, a, minR, s);
    }
    double bc;
    int bi;
    rs_pair_best<false, false>(s, var, false, nullptr, nullptr, &bc, &bi, nullptr);
    if (live && var == 0) {
      const double d = bc * minR;
      d_s[j] = (rm_finite(d) && !(excl_self && j == r)) ? d : __builtin_inf();
    }
  }
  __syncthreads();
  for (int q = 0; q < k; q++) {
    double bd = __builtin_inf();
    int bj = INT_MAX;
    for (int j = tid; j < n; j += RM_RT) {  // ascending j: the strict < keeps the lowest index
      const double d = d_s[j];
      if (d < bd) { bd = d; bj = j; }
    }
    block_argmin<RM_RT>(bd, bj, red_d, red_i);
    if (tid == 0) {
      const bool have = bd < __builtin_inf();
      const size_t o = (size_t)r * k + q;
      nbr[o] = have ? bj : -1;
      pa[o] = have ? (mode == 0 ? ri : bj) : -1;
      pb[o] = have ? (mode == 0 ? bj : ri) : -1;
      if (have) d_s[bj] = __builtin_inf();
    }
    __syncthreads();
  }
}

// -------------------------------------------------------------------- edges
// w_out[e] = d(P[pa[e]] -> P[pb[e]]) where RS_connected holds, +Inf where the path hits a wall, where d is not finite
// or where the pair is padding (an index < 0).  Per segment s (createPath's chains of rs_device.hpp, the check between):
//   A  lane p of wave 0: the heading chain of segment s; lane 2p+c of wave 1: the x / y running sum of segment s-1;
//   C  thread (p, c): column 100(s-1) + 5c + 5 of path p (x, y from the sums, ψ saved by B of the round before)
//      against every wall, ConvexCollision(wall, vehicle) with both SATs; s = 0: thread p, the start pose;
//   B  thread per (path, step): sincos(ψ_k) and the increments of segment s; ψ of the columns C will check.
__global__ __launch_bounds__(RM_CT) void rm_connect_kernel(int E, const int* __restrict__ pa,
                                                           const int* __restrict__ pb, const double* __restrict__ P,
                                                           double minR, double half_len, double half_wid, int nw,
                                                           const double* __restrict__ wtab,
                                                           double* __restrict__ w_out) {
  __shared__ double psi_s[RS_PT][RS_PST], xs_s[RS_PT][RS_PST], ys_s[RS_PT][RS_PST];
  __shared__ double psic_s[RS_PT][RM_NCHK];
  __shared__ double wt[WALL_TILE * WALL_ROW];
  __shared__ double cmd_s[RS_PT][15], cur_s[RS_PT][3], init_s[RS_PT][3], d_s[RS_PT];
  __shared__ int nseg_s[RS_PT], hit_s[RS_PT];
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * RS_PT;
  if (tid < 64) {
    const int p = tid >> 2, var = tid & 3, e = e0 + p;
    int ia = -1, ib = -1;
    if (e < E) {
      ia = pa[e];
      ib = pb[e];
    }
    const bool live = ia >= 0 && ib >= 0;
    double s[3] = {0.0, 0.0, 0.0}, a[3] = {0.0, 0.0, 0.0};
    if (live) {
      a[0] = P[3 * (size_t)ia];
      a[1] = P[3 * (size_t)ia + 1];
      a[2] = P[3 * (size_t)ia + 2];
      const double b[3] = {P[3 * (size_t)ib], P[3 * (size_t)ib + 1], P[3 * (size_t)ib + 2]};
      change_basis(a, b, minR, s);
    }
    double bc, tuv[3];
    int bi;
    rs_pair_best<false, true>(s, var, false, nullptr, nullptr, &bc, &bi, tuv);
    if (var == 0) {
      const double d = bc * minR;
      const bool ok = live && rm_finite(d);
      const int id = ok ? bi : 0;
      const int n = ok ? kRsN[id >> 2] : 0;
      rs_cmd_write_tuv(id, ok, tuv, cmd_s[p]);
      nseg_s[p] = n;
      hit_s[p] = 0;
      d_s[p] = ok ? d : __builtin_inf();
#pragma unroll
      for (int c = 0; c < 3; c++) init_s[p][c] = cur_s[p][c] = a[c];
    }
  } else if (nw <= WALL_TILE) {  // one tile holds the scene: loaded once
    for (int i = tid - 64; i < nw * WALL_ROW; i += RM_CT - 64) wt[i] = wtab[i];
  }
  __syncthreads();
  int mx = 0;
  for (int p = 0; p < RS_PT; p++) mx = nseg_s[p] > mx ? nseg_s[p] : mx;
  for (int s = 0; s <= mx; s++) {
    // ---- phase A: the serial chains, one lane each
    if (tid < RS_PT) {
      const int p = tid;
      if (s < nseg_s[p] && !hit_s[p]) cur_s[p][2] = rs_heading_chain(cmd_s[p] + 3 * s, cur_s[p][2], psi_s[p]);
    } else if (tid >= 64 && tid < 64 + 2 * RS_PT) {
      const int p = (tid - 64) >> 1, c = (tid - 64) & 1;
      if (s >= 1 && s - 1 < nseg_s[p] && !hit_s[p])
        cur_s[p][c] = rs_running_sum(c == 0 ? xs_s[p] : ys_s[p], cur_s[p][c]);
    }
    __syncthreads();
    // ---- phase C: block_collision_check of the columns that just landed
    if (nw > 0) {
      const int nitem = s == 0 ? 1 : RM_NCHK;
      const int p = tid < RS_PT * nitem ? tid / nitem : 0, c = tid - p * nitem;
      const bool active = tid < RS_PT * nitem && !hit_s[p] && (s == 0 ? nseg_s[p] > 0 : s - 1 < nseg_s[p]);
      double vq[8], vt[24];
      if (active) {  // the pose's rectangle (hybrid_astar_utils.jl:193) and its own SAT table, in registers
        const int k = 5 * c + 4;
        const double x = s == 0 ? init_s[p][0] : xs_s[p][k], y = s == 0 ? init_s[p][1] : ys_s[p][k];
        const double psi = s == 0 ? init_s[p][2] : psic_s[p][c];
        vehicle_rect(x, y, psi, half_len, half_len, half_wid, vq, vt);
      }
      bool hit = false;
      for (int w0 = 0; w0 < nw; w0 += WALL_TILE) {
        const int tw = min(WALL_TILE, nw - w0);
        if (nw > WALL_TILE) {  // block-uniform: the scene takes several tiles, each staged in turn
          __syncthreads();
          for (int i = tid; i < tw * WALL_ROW; i += RM_CT) wt[i] = wtab[(size_t)w0 * WALL_ROW + i];
          __syncthreads();
        }
        if (active && !hit) hit = tile_first_hit(MP_SAT_BOTH, wt, tw, vq, vt) >= 0;
      }
      __syncthreads();  // every read of hit_s above comes before the writes below
      if (hit) hit_s[p] = 1;
      __syncthreads();
    }
    // ---- phase B: one thread per (path, step)
    for (int i = tid; i < RS_PT * 100; i += RM_CT) {
      const int p = i / 100, k = i - 100 * p;
      if (s < nseg_s[p] && !hit_s[p]) {
        rs_step_inc(cmd_s[p] + 3 * s, psi_s[p][k], minR, &xs_s[p][k], &ys_s[p][k]);
        if (k % 5 == 4) psic_s[p][k / 5] = psi_s[p][k + 1];
      }
    }
    __syncthreads();
  }
  if (tid < RS_PT && e0 + tid < E) w_out[e0 + tid] = hit_s[tid] ? __builtin_inf() : d_s[tid];
}

// -------------------------------------------------------------------- queries
// Query q of B.  Out-edges of the start: qnbr[q][k] with qw[q][k], and the direct edge qw[2Bk + q] to the goal; of
// node i: nbr[i][k] with w[i][k], and qw[(B + q)k + r] to the goal where qnbr[B + q][r] == i.  seq[q][n + 2] holds
// the vertices from start to goal, -1 beyond seq_len.
__global__ __launch_bounds__(RM_DT) void rm_dijkstra_kernel(int n, int k, int B, const int* __restrict__ nbr,
                                                            const double* __restrict__ w,
                                                            const int* __restrict__ qnbr,
                                                            const double* __restrict__ qw,
                                                            unsigned char* __restrict__ found,
                                                            double* __restrict__ cost, int* __restrict__ seq,
                                                            int* __restrict__ seq_len, int* __restrict__ settled,
                                                            unsigned char* __restrict__ direct_free) {
  __shared__ double dist[RM_MAXN + 2];
  __shared__ int parent[RM_MAXN + 2];
  __shared__ unsigned char done[RM_MAXN + 2];
  __shared__ int gn_s[MP_ROADMAP_MAX_K];
  __shared__ double gw_s[MP_ROADMAP_MAX_K];
  __shared__ double red_d[RM_DT / 64];
  __shared__ int red_i[RM_DT / 64];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int V = n + 2, goal = n + 1;
  int* sq = seq + (size_t)q * V;
  for (int v = tid; v < V; v += RM_DT) {
    dist[v] = v == 0 ? 0.0 : __builtin_inf();
    parent[v] = -1;
    done[v] = 0;
    sq[v] = -1;
  }
  if (tid < k) {
    gn_s[tid] = qnbr[((size_t)B + q) * k + tid];
    gw_s[tid] = qw[((size_t)B + q) * k + tid];
  }
  const double direct = qw[2 * (size_t)B * k + q];
  __syncthreads();
  int ns = 0;
  bool reached = false;
  for (;;) {
    double bd = __builtin_inf();
    int bv = INT_MAX;
    for (int v = tid; v < V; v += RM_DT) {  // ascending v: the strict < keeps the lowest vertex
      const double d = dist[v];
      if (!done[v] && d < bd) { bd = d; bv = v; }
    }
    block_argmin<RM_DT>(bd, bv, red_d, red_i);
    if (!(bd < __builtin_inf())) break;  // block-uniform
    ns++;
    if (bv == goal) {
      reached = true;
      break;
    }
    // one thread per out-edge of bv; a vertex is the head of at most one of them
    int v = -1;
    double wt = __builtin_inf();
    if (tid < k) {
      const size_t o = (bv == 0 ? (size_t)q : (size_t)(bv - 1)) * k + tid;
      const int j = bv == 0 ? qnbr[o] : nbr[o];
      wt = bv == 0 ? qw[o] : w[o];
      v = j >= 0 ? j + 1 : -1;
    } else if (tid < 2 * k) {
      if (bv != 0 && gn_s[tid - k] == bv - 1) {
        v = goal;
        wt = gw_s[tid - k];
      }
    } else if (tid == 2 * k && bv == 0) {
      v = goal;
      wt = direct;
    }
    if (v >= 0 && !done[v]) {
      const double nd = bd + wt;
      if (nd < dist[v]) {
        dist[v] = nd;
        parent[v] = bv;
      }
    }
    if (tid == RM_DT - 1) done[bv] = 1;
    __syncthreads();
  }
  if (tid == 0) {
    found[q] = reached ? 1 : 0;
    cost[q] = reached ? dist[goal] : __builtin_inf();
    settled[q] = ns;
    direct_free[q] = rm_finite(direct) ? 1 : 0;
    int len = 0;
    if (reached) {
      for (int v = goal; v >= 0 && len < V; v = parent[v]) len++;
      int at = len;
      for (int v = goal; v >= 0 && at > 0; v = parent[v]) sq[--at] = v;
    }
    seq_len[q] = len;
  }
}

// what both calls check of a scene
int rm_check_scene(mp_ctx* ctx, const char* fn, int n, const double* nodes, int n_walls, const double* walls,
                   double minR, double len, double wid, int k) {
  MP_CHECK(ctx, n >= 1 && n <= MP_ROADMAP_MAX_NODES, "%s: n (%d) outside [1, %d]", fn, n, MP_ROADMAP_MAX_NODES);
  MP_CHECK(ctx, k >= 1 && k <= MP_ROADMAP_MAX_K, "%s: k (%d) outside [1, %d]", fn, k, MP_ROADMAP_MAX_K);
  MP_CHECK(ctx, n_walls >= 0, "%s: n_walls (%d) must be >= 0", fn, n_walls);
  MP_CHECK(ctx, nodes && (walls || n_walls == 0), "%s: NULL argument", fn);
  MP_CHECK(ctx, std::isfinite(minR) && minR > 0, "%s: minR must be finite and positive", fn);
  MP_CHECK(ctx, std::isfinite(len) && std::isfinite(wid), "%s: non-finite vehicle size", fn);
  MP_CHECK(ctx, mp_all_finite(nodes, 3 * (size_t)n), "%s: non-finite node", fn);
  MP_CHECK(ctx, n_walls == 0 || mp_all_finite(walls, 5 * (size_t)n_walls), "%s: non-finite wall", fn);
  return MP_OK;
}

// the scene's wall table, enqueued on the context stream (nullptr and MP_OK without walls)
int rm_walls(mp_ctx* ctx, int slot_in, int slot_tab, int n_walls, const double* walls, const double** wtab) {
  *wtab = nullptr;
  if (n_walls == 0) return MP_OK;
  int st = MP_OK;
  const double* dwalls = mp_upload(ctx, slot_in, walls, 5 * (size_t)n_walls, &st);
  double* dtab = (double*)mp_ws(ctx, slot_tab, (size_t)n_walls * WALL_ROW * sizeof(double));
  if (!dtab) return MP_ERR_NOMEM;
  if (st) return st;
  hipLaunchKernelGGL(rm_wall_kernel, dim3((unsigned)((n_walls + 63) / 64)), dim3(64), 0, ctx->stream, n_walls, dwalls,
                     dtab);
  MP_HIP(ctx, hipGetLastError());
  *wtab = dtab;
  return MP_OK;
}

}  // namespace

extern "C" {

int mp_roadmap_build(mp_ctx* ctx, int32_t n, const double* nodes, int32_t n_walls, const double* walls, double minR,
                     double vehicle_len, double vehicle_wid, int32_t k, int32_t* nbr, double* w) {
  if (!ctx) return mp_fail(nullptr, MP_ERR_INVALID, "mp_roadmap_build: NULL context");
  int st;
  if ((st = rm_check_scene(ctx, "mp_roadmap_build", n, nodes, n_walls, walls, minR, vehicle_len, vehicle_wid, k)))
    return st;
  MP_CHECK(ctx, nbr && w, "mp_roadmap_build: NULL output");
  MP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t E = (size_t)n * k;
  const double* dP = mp_upload(ctx, WS_IO0, nodes, 3 * (size_t)n, &st);
  int32_t* dnbr = mp_alloc_out(ctx, WS_IO3, nbr, E, &st);
  double* dw = mp_alloc_out(ctx, WS_IO4, w, E, &st);
  int* dpa = (int*)mp_ws(ctx, WS_IO5, E * sizeof(int));
  int* dpb = (int*)mp_ws(ctx, WS_IO6, E * sizeof(int));
  if (!dpa || !dpb) return MP_ERR_NOMEM;
  if (st) return st;
  const double* dtab;
  if ((st = rm_walls(ctx, WS_IO1, WS_IO2, n_walls, walls, &dtab))) return st;
  hipLaunchKernelGGL(rm_rank_kernel, dim3((unsigned)n), dim3(RM_RT), 0, ctx->stream, (int)n, (int)k, 0, 0, 1, dP, minR,
                     (int*)dnbr, dpa, dpb);
  MP_HIP(ctx, hipGetLastError());
  mp_time_begin(ctx);
  hipLaunchKernelGGL(rm_connect_kernel, dim3((unsigned)((E + RS_PT - 1) / RS_PT)), dim3(RM_CT), 0, ctx->stream, (int)E,
                     dpa, dpb, dP, minR, vehicle_len / 2, vehicle_wid / 2, (int)n_walls, dtab, dw);
  MP_HIP(ctx, hipGetLastError());
  mp_time_end(ctx);
  if ((st = mp_download(ctx, nbr, (const int32_t*)dnbr, E))) return st;
  if ((st = mp_download(ctx, w, (const double*)dw, E))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

int mp_roadmap_query(mp_ctx* ctx, int32_t n, const double* nodes, int32_t n_walls, const double* walls, double minR,
                     double vehicle_len, double vehicle_wid, int32_t k, const int32_t* nbr, const double* w, int32_t B,
                     const double* start, const double* goal, uint8_t* found, double* cost, int32_t* seq,
                     int32_t* seq_len, int32_t* settled, uint8_t* direct_free) {
  if (!ctx) return mp_fail(nullptr, MP_ERR_INVALID, "mp_roadmap_query: NULL context");
  int st;
  if ((st = rm_check_scene(ctx, "mp_roadmap_query", n, nodes, n_walls, walls, minR, vehicle_len, vehicle_wid, k)))
    return st;
  MP_CHECK(ctx, B >= 1 && B <= MP_ROADMAP_MAX_QUERIES, "mp_roadmap_query: B (%d) outside [1, %d]", B,
           MP_ROADMAP_MAX_QUERIES);
  MP_CHECK(ctx, nbr && w && start && goal, "mp_roadmap_query: NULL input");
  MP_CHECK(ctx, found && cost && seq && seq_len && settled && direct_free, "mp_roadmap_query: NULL output");
  MP_CHECK(ctx, mp_all_finite(start, 3 * (size_t)B), "mp_roadmap_query: non-finite start");
  MP_CHECK(ctx, mp_all_finite(goal, 3 * (size_t)B), "mp_roadmap_query: non-finite goal");
  const size_t E = (size_t)n * k, nB = (size_t)B, Bk = nB * k, EQ = 2 * Bk + nB, V = (size_t)n + 2;
  for (size_t e = 0; e < E; e++)
    MP_CHECK(ctx, nbr[e] >= -1 && nbr[e] < n, "mp_roadmap_query: nbr[%zu] = %d outside [-1, %d]", e, nbr[e], n - 1);
  MP_HIP(ctx, hipSetDevice(ctx->device));
  // the pose table: nodes, then the starts, then the goals; the direct pairs close the pair list
  std::vector<double> table(3 * ((size_t)n + 2 * nB));
  std::copy(nodes, nodes + 3 * (size_t)n, table.begin());
  std::copy(start, start + 3 * nB, table.begin() + 3 * (size_t)n);
  std::copy(goal, goal + 3 * nB, table.begin() + 3 * ((size_t)n + nB));
  std::vector<int> direct(2 * nB);
  for (int q = 0; q < B; q++) {
    direct[q] = n + q;
    direct[nB + q] = n + B + q;
  }
  // every buffer first, the copies from this call's own host arrays after the last exit that leaves them in flight
  double* dP = (double*)mp_ws(ctx, WS_IO0, table.size() * sizeof(double));
  int* dpa = (int*)mp_ws(ctx, WS_IO5, EQ * sizeof(int));
  int* dpb = (int*)mp_ws(ctx, WS_IO6, EQ * sizeof(int));
  int* dqn = (int*)mp_ws(ctx, WS_IO7, 2 * Bk * sizeof(int));
  double* dqw = (double*)mp_ws(ctx, WS_IO8, EQ * sizeof(double));
  if (!dP || !dpa || !dpb || !dqn || !dqw) return MP_ERR_NOMEM;
  const int32_t* dnbr = mp_upload(ctx, WS_IO3, nbr, E, &st);
  const double* dw = mp_upload(ctx, WS_IO4, w, E, &st);
  uint8_t* dfound = mp_alloc_out(ctx, WS_IO9, found, nB, &st);
  double* dcost = mp_alloc_out(ctx, WS_IO10, cost, nB, &st);
  int32_t* dseq = mp_alloc_out(ctx, WS_IO11, seq, nB * V, &st);
  int32_t* dlen = mp_alloc_out(ctx, WS_IO12, seq_len, nB, &st);
  int32_t* dset = mp_alloc_out(ctx, WS_IO13, settled, nB, &st);
  uint8_t* ddir = mp_alloc_out(ctx, WS_IO14, direct_free, nB, &st);
  if (st) return st;
  const double* dtab;
  if ((st = rm_walls(ctx, WS_IO1, WS_IO2, n_walls, walls, &dtab))) return st;
  hipError_t he = hipMemcpyAsync(dP, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (he == hipSuccess)
    he = hipMemcpyAsync(dpa + 2 * Bk, direct.data(), nB * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
  if (he == hipSuccess)
    he = hipMemcpyAsync(dpb + 2 * Bk, direct.data() + nB, nB * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
  if (he != hipSuccess) {
    hipStreamSynchronize(ctx->stream);
    return mp_fail(ctx, MP_ERR_HIP, "mp_roadmap_query: H2D copy failed: %s", hipGetErrorString(he));
  }
  hipLaunchKernelGGL(rm_rank_kernel, dim3((unsigned)B), dim3(RM_RT), 0, ctx->stream, (int)n, (int)k, 0, (int)n, 0, dP,
                     minR, dqn, dpa, dpb);
  hipLaunchKernelGGL(rm_rank_kernel, dim3((unsigned)B), dim3(RM_RT), 0, ctx->stream, (int)n, (int)k, 1, (int)(n + B), 0,
                     dP, minR, dqn + Bk, dpa + Bk, dpb + Bk);
  MP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(rm_connect_kernel, dim3((unsigned)((EQ + RS_PT - 1) / RS_PT)), dim3(RM_CT), 0, ctx->stream,
                     (int)EQ, dpa, dpb, dP, minR, vehicle_len / 2, vehicle_wid / 2, (int)n_walls, dtab, dqw);
  MP_HIP(ctx, hipGetLastError());
  mp_time_begin(ctx);
  hipLaunchKernelGGL(rm_dijkstra_kernel, dim3((unsigned)B), dim3(RM_DT), 0, ctx->stream, (int)n, (int)k, (int)B,
                     (const int*)dnbr, dw, dqn, dqw, dfound, dcost, (int*)dseq, (int*)dlen, (int*)dset, ddir);
  MP_HIP(ctx, hipGetLastError());
  mp_time_end(ctx);
  if ((st = mp_download(ctx, found, (const uint8_t*)dfound, nB))) return st;
  if ((st = mp_download(ctx, cost, (const double*)dcost, nB))) return st;
  if ((st = mp_download(ctx, seq, (const int32_t*)dseq, nB * V))) return st;
  if ((st = mp_download(ctx, seq_len, (const int32_t*)dlen, nB))) return st;
  if ((st = mp_download(ctx, settled, (const int32_t*)dset, nB))) return st;
  if ((st = mp_download(ctx, direct_free, (const uint8_t*)ddir, nB))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // table and direct stay alive until here
  return MP_OK;
}

}  // extern "C"
