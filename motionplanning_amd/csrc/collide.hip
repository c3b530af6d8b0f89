// collide.hip — batched collision detection for gfx950 (PathPlanning/CollisionDetection/src/utils.jl,
// HybridAstar/src/hybrid_astar_utils.jl:180-204 block_collision_check) + C-ABI.
//
// collide_block_pts_kernel   GetRectanglePts (utils.jl:14-25), one lane per block.
// collide_convex_kernel      SeparatingAxisTheorem / ConvexCollision (utils.jl:37-74) on general column
//                            lists, one lane per pair (a_i, b_j) of a scene; the scene's polygons are
//                            staged in LDS when they fit, read from global memory otherwise.
// collide_path_kernel        block_collision_check for B scenes: block (chunk, scene), one checked pose
//                            per lane.  The pose's four corners and its own per-edge SAT table
//                            [bx, by, nx, ny, min, max] stay in registers; the scene's walls pass through
//                            LDS in tiles of WALL_TILE as corners + the wall-side table, built once per
//                            tile by the block.  Per scene the blocks reduce (lowest hit pose, its lowest
//                            wall) and the hit count in the wave, then in LDS, then with one 64-bit
//                            atomic min on (pose << 32 | wall) and one atomic add per block.
//
// Every product is rounded as the reference's BLAS does (oracle/or_blas.h): R*pts as dgemm with K = 2,
// fma(a1, b1, a0*b0), and transpose(pts .- bg)*normal as dgemv 'T' on two rows, fma(m0, n0, m1*n1).
// minimum / maximum are Julia's: a NaN among the projections makes both NaN, and then neither `<=` of
// utils.jl:57 holds.  The minima are taken with fmin / fmax (which skip a NaN) beside an unordered test
// of the projections; the sign of a zero does not reach a `<=`.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

// per-lane early exits (hit poses stop, separated pairs stop): lane-safe libm, no wave-level ballots in it
#define MPJ_LANE_SAFE 1
#include "../../include/mp_jlmath.h"
#include "collide_device.hpp"
#include "runtime.hpp"

namespace {

constexpr int POSE_CHUNK = 256;  // checked poses per block of collide_path_kernel, one per lane
constexpr int PAIR_BLOCK = 256;  // pairs per block of collide_convex_kernel
constexpr int CONVEX_LDS_DOUBLES = 4096;  // a scene's polygons are staged in LDS up to this many doubles (32 KiB)

// -------------------------------------------------------------------- GetRectanglePts
__global__ void __launch_bounds__(256) collide_block_pts_kernel(long long n, const double* __restrict__ blocks,
                                                                double* __restrict__ pts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* b = blocks + 5 * i;
  double s, c, q[8];
  mpj_sincos_bl(b[2], &s, &c);
  rect_pts4(b[0], b[1], c, s, b[3], b[4], q);
  double* o = pts + 10 * i;
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = q[j];
  o[8] = q[0];
  o[9] = q[1];
}

// -------------------------------------------------------------------- general convex polygons
// SeparatingAxisTheorem(base, other) on column lists [cols][2]; loops bounded by the column counts.
__device__ __forceinline__ bool sat_general(const double* base, int cb, const double* other, int co) {
  for (int e = 0; e + 1 < cb; e++) {
    const double bx = base[2 * e], by = base[2 * e + 1];
    const double vx = base[2 * e + 2] - bx, vy = base[2 * e + 3] - by;
    const double nx = -vy, ny = vx;
    double mnb = 0, mxb = 0, mno = 0, mxo = 0;
    bool nan = false;
#pragma unroll 1
    for (int j = 0; j < cb; j++) {
      const double d = sat_dp(base[2 * j] - bx, base[2 * j + 1] - by, nx, ny);
      nan |= d != d;
      mnb = j ? __builtin_fmin(mnb, d) : d;
      mxb = j ? __builtin_fmax(mxb, d) : d;
    }
#pragma unroll 1
    for (int j = 0; j < co; j++) {
      const double d = sat_dp(other[2 * j] - bx, other[2 * j + 1] - by, nx, ny);
      nan |= d != d;
      mno = j ? __builtin_fmin(mno, d) : d;
      mxo = j ? __builtin_fmax(mxo, d) : d;
    }
    if (!nan && ((mxo <= mnb) || (mxb <= mno))) return true;
  }
  return false;
}

// grid (ceil(na*nb / PAIR_BLOCK), B).  kLds: the scene's polygons ([na][ma][2] then [nb][mb][2]) are copied to
// LDS first (dynamic, (na*ma + nb*mb)*2 doubles); else they are read where they lie.
template <bool kLds>
__global__ void __launch_bounds__(PAIR_BLOCK) collide_convex_kernel(int mode, int na, int ma, const double* __restrict__ pa,
                                                                    const int* __restrict__ a_cols, int nb, int mb,
                                                                    const double* __restrict__ pb,
                                                                    const int* __restrict__ b_cols,
                                                                    unsigned char* __restrict__ free_) {
  extern __shared__ double sm[];
  const int s = blockIdx.y;
  const size_t da = (size_t)na * ma * 2, db = (size_t)nb * mb * 2;
  const double* A = pa + s * da;
  const double* Bp = pb + s * db;
  if (kLds) {
    for (int i = threadIdx.x; i < (int)da; i += PAIR_BLOCK) sm[i] = A[i];
    for (int i = threadIdx.x; i < (int)db; i += PAIR_BLOCK) sm[da + i] = Bp[i];
    __syncthreads();
    A = sm;
    Bp = sm + da;
  }
  const long long pair = (long long)blockIdx.x * PAIR_BLOCK + threadIdx.x;
  if (pair >= (long long)na * nb) return;
  const int i = (int)(pair / nb), j = (int)(pair % nb);
  const int ca = a_cols ? a_cols[(size_t)s * na + i] : ma, cb = b_cols ? b_cols[(size_t)s * nb + j] : mb;
  const double* a = A + (size_t)i * ma * 2;
  const double* b = Bp + (size_t)j * mb * 2;
  bool fr = sat_general(a, ca, b, cb);
  if (mode == MP_SAT_BOTH) {
    if (fr) fr = sat_general(b, cb, a, ca);
  } else if (mode == MP_SAT_EITHER) {
    if (!fr) fr = sat_general(b, cb, a, ca);
  }
  free_[((size_t)s * na + i) * nb + j] = fr ? 1 : 0;
}

// -------------------------------------------------------------------- swept paths
struct PathDev {
  double half_len, half_wid, shift;
  int stride, mode, n_poses, n_walls;
};

// Checked poses of a scene with cnt poses (hybrid_astar_utils.jl:182-190): 1:sparcity_num:end when
// cnt > sparcity_num, the first pose alone otherwise.
__host__ __device__ inline int checked_count(int cnt, int stride) {
  if (cnt <= 0) return 0;
  return cnt > stride ? (cnt - 1) / stride + 1 : 1;
}

// grid (ceil(max checked / POSE_CHUNK), B), POSE_CHUNK threads.  key[B] starts at ~0, n_hit[B] at 0 and
// pose_free (optional) at 2.
__global__ void __launch_bounds__(POSE_CHUNK) collide_path_kernel(PathDev P, const double* __restrict__ poses,
                                                                  const int* __restrict__ pose_count,
                                                                  const double* __restrict__ walls,
                                                                  const int* __restrict__ wall_count,
                                                                  unsigned long long* __restrict__ key,
                                                                  int* __restrict__ n_hit,
                                                                  unsigned char* __restrict__ pose_free) {
  __shared__ double wt[WALL_TILE * WALL_ROW];
  __shared__ unsigned long long red_key[POSE_CHUNK / 64];
  __shared__ int red_cnt[POSE_CHUNK / 64];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int cnt = pose_count ? pose_count[s] : P.n_poses;
  const int nchk = checked_count(cnt, P.stride);
  if ((int)blockIdx.x * POSE_CHUNK >= nchk) return;  // block-uniform
  const int nw = wall_count ? wall_count[s] : P.n_walls;
  const int k = blockIdx.x * POSE_CHUNK + tid;
  const bool active = k < nchk;
  const int pidx = active ? k * P.stride : 0;  // < cnt <= n_poses

  // the pose's rectangle (hybrid_astar_utils.jl:193) and its own SAT table, in registers
  double vq[8], vt[24];
  const double* q = poses + ((size_t)s * P.n_poses + pidx) * 3;
  vehicle_rect(q[0], q[1], q[2], P.shift, P.half_len, P.half_wid, vq, vt);

  int first_wall = -1;
  for (int w0 = 0; w0 < nw; w0 += WALL_TILE) {
    const int tw = min(WALL_TILE, nw - w0);
    // the tile's wall rows, built by the block (what wall_row does for one wall): corners, then edges
    if (tid < tw) {
      const double* wl = walls + ((size_t)s * P.n_walls + w0 + tid) * 5;
      double sw, cw;
      mpj_sincos_bl(wl[2], &sw, &cw);
      rect_pts4(wl[0], wl[1], cw, sw, wl[3], wl[4], wt + tid * WALL_ROW);
    }
    __syncthreads();
    if (tid < 4 * tw) rect_edge(wt + (tid >> 2) * WALL_ROW, tid & 3, wt + (tid >> 2) * WALL_ROW + 8 + 6 * (tid & 3));
    __syncthreads();
    if (active && first_wall < 0) {
      const int w = tile_first_hit(P.mode, wt, tw, vq, vt);
      if (w >= 0) first_wall = w0 + w;
    }
    __syncthreads();  // the tile is rebuilt next
  }

  const bool hit = active && first_wall >= 0;
  if (pose_free && active) pose_free[(size_t)s * P.n_poses + pidx] = hit ? 0 : 1;
  unsigned long long kk = hit ? (((unsigned long long)(unsigned)pidx << 32) | (unsigned)first_wall) : ~0ull;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(kk, o, 64);
    kk = other < kk ? other : kk;
  }
  const int hits = __popcll(__ballot(hit));
  if ((tid & 63) == 0) {
    red_key[tid >> 6] = kk;
    red_cnt[tid >> 6] = hits;
  }
  __syncthreads();
  if (tid == 0) {
    int c = 0;
#pragma unroll
    for (int i = 0; i < POSE_CHUNK / 64; i++) {
      kk = red_key[i] < kk ? red_key[i] : kk;
      c += red_cnt[i];
    }
    if (c) {
      atomicMin(key + s, kk);
      atomicAdd(n_hit + s, c);
    }
  }
}

}  // namespace

extern "C" {

int mp_block_pts(mp_ctx* ctx, int64_t n, const double* blocks, double* pts) {
  if (!ctx) return mp_fail(nullptr, MP_ERR_INVALID, "mp_block_pts: NULL context");
  MP_CHECK(ctx, n >= 0, "mp_block_pts: n (%lld) must be >= 0", (long long)n);
  if (n == 0) return MP_OK;
  MP_CHECK(ctx, blocks && pts, "mp_block_pts: NULL argument");
  MP_CHECK(ctx, n <= (int64_t)1 << 31, "mp_block_pts: n (%lld) above 2^31", (long long)n);
  MP_CHECK(ctx, mp_all_finite(blocks, 5 * (size_t)n), "mp_block_pts: non-finite block");
  int st = MP_OK;
  const double* db = mp_upload(ctx, WS_IO0, blocks, 5 * (size_t)n, &st);
  double* dp = mp_alloc_out(ctx, WS_IO1, pts, 10 * (size_t)n, &st);
  if (st) return st;
  hipLaunchKernelGGL(collide_block_pts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                     (long long)n, db, dp);
  MP_HIP(ctx, hipGetLastError());
  if ((st = mp_download(ctx, pts, (const double*)dp, 10 * (size_t)n))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

// cols of every polygon in range and its first cols rows finite
static int check_polys(mp_ctx* ctx, const char* which, int B, int n, int m, const double* polys, const int32_t* cols) {
  for (size_t k = 0; k < (size_t)B * n; k++) {
    const int c = cols ? cols[k] : m;
    MP_CHECK(ctx, c >= 2 && c <= m && c <= MP_COLLIDE_MAX_COLS,
             "mp_convex_collision: polygon %zu of %s has %d columns, outside [2, min(%d, %d)]", k, which, c, m,
             MP_COLLIDE_MAX_COLS);
    MP_CHECK(ctx, mp_all_finite(polys + k * m * 2, 2 * (size_t)c), "mp_convex_collision: non-finite vertex in polygon %zu of %s",
             k, which);
  }
  return MP_OK;
}

int mp_convex_collision(mp_ctx* ctx, int32_t mode, int32_t B, int32_t na, int32_t ma, const double* polys_a,
                        const int32_t* a_cols, int32_t nb, int32_t mb, const double* polys_b, const int32_t* b_cols,
                        uint8_t* free_) {
  if (!ctx) return mp_fail(nullptr, MP_ERR_INVALID, "mp_convex_collision: NULL context");
  MP_CHECK(ctx, B >= 0 && na >= 0 && nb >= 0 && ma >= 0 && mb >= 0, "mp_convex_collision: negative size");
  MP_CHECK(ctx, mode == MP_SAT_BOTH || mode == MP_SAT_EITHER || mode == MP_SAT_BASE_A,
           "mp_convex_collision: unknown mode %d", mode);
  if (B == 0 || na == 0 || nb == 0) return MP_OK;
  MP_CHECK(ctx, polys_a && polys_b && free_, "mp_convex_collision: NULL argument");
  int st;
  if ((st = check_polys(ctx, "a", B, na, ma, polys_a, a_cols))) return st;
  if ((st = check_polys(ctx, "b", B, nb, mb, polys_b, b_cols))) return st;
  MP_CHECK(ctx, (long long)na * nb <= (1ll << 31) - PAIR_BLOCK && B <= 65535,
           "mp_convex_collision: na*nb (%lld) or B (%d) too large for one launch", (long long)na * nb, B);
  const size_t da = (size_t)B * na * ma * 2, db = (size_t)B * nb * mb * 2, nf = (size_t)B * na * nb;
  st = MP_OK;
  const double* dpa = mp_upload(ctx, WS_IO0, polys_a, da, &st);
  const double* dpb = mp_upload(ctx, WS_IO1, polys_b, db, &st);
  const int* dca = mp_upload(ctx, WS_IO2, a_cols, (size_t)B * na, &st);
  const int* dcb = mp_upload(ctx, WS_IO3, b_cols, (size_t)B * nb, &st);
  uint8_t* dfr = mp_alloc_out(ctx, WS_IO4, free_, nf, &st);
  if (st) return st;
  const dim3 grid((unsigned)(((long long)na * nb + PAIR_BLOCK - 1) / PAIR_BLOCK), (unsigned)B);
  const size_t scene = ((size_t)na * ma + (size_t)nb * mb) * 2;
  mp_time_begin(ctx);
  if (scene <= (size_t)CONVEX_LDS_DOUBLES)
    hipLaunchKernelGGL(collide_convex_kernel<true>, grid, dim3(PAIR_BLOCK), scene * sizeof(double), ctx->stream, mode, na,
                       ma, dpa, dca, nb, mb, dpb, dcb, dfr);
  else
    hipLaunchKernelGGL(collide_convex_kernel<false>, grid, dim3(PAIR_BLOCK), 0, ctx->stream, mode, na, ma, dpa, dca, nb,
                       mb, dpb, dcb, dfr);
  mp_time_end(ctx);
  MP_HIP(ctx, hipGetLastError());
  if ((st = mp_download(ctx, free_, (const uint8_t*)dfr, nf))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

int mp_path_collision(mp_ctx* ctx, const mp_collide_params_t* p, int32_t B, int32_t n_poses, const double* poses,
                      const int32_t* pose_count, int32_t n_walls, const int32_t* wall_count, const double* walls,
                      uint8_t* scene_free, int32_t* first_pose, int32_t* first_wall, int32_t* n_hit, uint8_t* pose_free) {
  if (!ctx) return mp_fail(nullptr, MP_ERR_INVALID, "mp_path_collision: NULL context");
  MP_CHECK(ctx, p, "mp_path_collision: NULL params");
  MP_CHECK(ctx, B >= 0 && n_poses >= 0 && n_walls >= 0, "mp_path_collision: negative size");
  MP_CHECK(ctx, p->stride >= 1, "mp_path_collision: stride (%d) must be >= 1", p->stride);
  MP_CHECK(ctx, p->mode == MP_SAT_BOTH || p->mode == MP_SAT_EITHER || p->mode == MP_SAT_BASE_A,
           "mp_path_collision: unknown mode %d", p->mode);
  MP_CHECK(ctx, std::isfinite(p->half_len) && std::isfinite(p->half_wid) && std::isfinite(p->center_shift),
           "mp_path_collision: non-finite vehicle size or centre shift");
  if (B == 0) return MP_OK;
  MP_CHECK(ctx, scene_free && first_pose && first_wall && n_hit, "mp_path_collision: NULL output");
  MP_CHECK(ctx, (poses || n_poses == 0) && (walls || n_walls == 0), "mp_path_collision: NULL input");
  MP_CHECK(ctx, B <= 65535, "mp_path_collision: B (%d) above 65535 scenes per call", B);
  int max_chk = 0;
  for (int b = 0; b < B; b++) {
    const int cnt = pose_count ? pose_count[b] : n_poses, nw = wall_count ? wall_count[b] : n_walls;
    MP_CHECK(ctx, cnt >= 0 && cnt <= n_poses, "mp_path_collision: pose_count[%d] = %d outside [0, %d]", b, cnt, n_poses);
    MP_CHECK(ctx, nw >= 0 && nw <= n_walls, "mp_path_collision: wall_count[%d] = %d outside [0, %d]", b, nw, n_walls);
    const int nchk = checked_count(cnt, p->stride);
    for (int k = 0; k < nchk; k++)
      MP_CHECK(ctx, mp_all_finite(poses + ((size_t)b * n_poses + (size_t)k * p->stride) * 3, 3),
               "mp_path_collision: non-finite pose %d of scene %d", k * p->stride, b);
    MP_CHECK(ctx, nw == 0 || mp_all_finite(walls + (size_t)b * n_walls * 5, 5 * (size_t)nw),
             "mp_path_collision: non-finite wall in scene %d", b);
    max_chk = std::max(max_chk, nchk);
  }
  const size_t nb = (size_t)B, npf = nb * n_poses;
  if (max_chk == 0) {  // nothing is checked: every scene is free
    for (size_t b = 0; b < nb; b++) {
      scene_free[b] = 1;
      first_pose[b] = first_wall[b] = -1;
      n_hit[b] = 0;
    }
    if (pose_free) memset(pose_free, 2, npf);
    return MP_OK;
  }
  int st = MP_OK;
  const double* dposes = mp_upload(ctx, WS_IO0, poses, 3 * npf, &st);
  const int* dpc = mp_upload(ctx, WS_IO1, pose_count, nb, &st);
  const double* dwalls = mp_upload(ctx, WS_IO2, walls, 5 * nb * n_walls, &st);
  const int* dwc = mp_upload(ctx, WS_IO3, wall_count, nb, &st);
  unsigned long long* dkey = (unsigned long long*)mp_ws(ctx, WS_IO4, nb * sizeof(unsigned long long));
  int* dnh = mp_alloc_out(ctx, WS_IO5, n_hit, nb, &st);
  uint8_t* dpf = mp_alloc_out(ctx, WS_IO6, pose_free, npf, &st);
  if (!dkey) return MP_ERR_NOMEM;
  if (st) return st;
  MP_HIP(ctx, hipMemsetAsync(dkey, 0xff, nb * sizeof(unsigned long long), ctx->stream));
  MP_HIP(ctx, hipMemsetAsync(dnh, 0, nb * sizeof(int), ctx->stream));
  if (dpf) MP_HIP(ctx, hipMemsetAsync(dpf, 2, npf, ctx->stream));
  PathDev D;
  D.half_len = p->half_len;
  D.half_wid = p->half_wid;
  D.shift = p->center_shift;
  D.stride = p->stride;
  D.mode = p->mode;
  D.n_poses = n_poses;
  D.n_walls = n_walls;
  mp_time_begin(ctx);
  hipLaunchKernelGGL(collide_path_kernel, dim3((unsigned)((max_chk + POSE_CHUNK - 1) / POSE_CHUNK), (unsigned)B),
                     dim3(POSE_CHUNK), 0, ctx->stream, D, dposes, dpc, dwalls, dwc, dkey, dnh, dpf);
  mp_time_end(ctx);
  MP_HIP(ctx, hipGetLastError());
  std::vector<unsigned long long> hkey(nb);
  MP_HIP(ctx, hipMemcpyAsync(hkey.data(), dkey, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  if ((st = mp_download(ctx, n_hit, (const int32_t*)dnh, nb))) return st;
  if ((st = mp_download(ctx, pose_free, (const uint8_t*)dpf, npf))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t b = 0; b < nb; b++) {
    const bool hit = hkey[b] != ~0ull;
    scene_free[b] = hit ? 0 : 1;
    first_pose[b] = hit ? (int32_t)(hkey[b] >> 32) : -1;
    first_wall[b] = hit ? (int32_t)(hkey[b] & 0xffffffffu) : -1;
  }
  return MP_OK;
}

}  // extern "C"
