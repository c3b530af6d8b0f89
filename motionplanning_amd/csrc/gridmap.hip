// gridmap.hip — tools on occupancy maps for gfx950 (an extension, include/mpgpu.h "occupancy maps"): the exact
// squared Euclidean distance transform of a free-cell mask, inflation by a robot radius, and the clearance of a
// path + C-ABI: mp_grid_distance, mp_grid_inflate, mp_grid_path_clearance.  (mp_grid_rasterize is in astar.hip,
// beside the cell test it shares with the planners.)
//
// The transform is the separable one: d2(x, y) = min over y' of g(x, y')^2 + (y - y')^2, g the distance along row
// y' to its nearest blocked cell.  Everything is integer arithmetic, so any exact algorithm gives these bytes.
//
// map_row_kernel      g for every row, one wavefront per row, 64 cells a step: a wave-inclusive max-scan of the
//                     last blocked index (read off the step's ballot) with a carry between steps, and its mirror
//                     image from right to left.
// map_col_kernel      one lane per cell, a wavefront on 64 consecutive x of one row (every read of g is one
//                     coalesced line), four rows a block.  A lane searches outward, y -+ k, keeps
//                     best = min(g^2 + k^2) and stops once k^2 >= best: the work is the distance found.
//                     <false> writes d2; <true>, the capped instance behind mp_grid_inflate, also stops once
//                     k^2 > r2 or best <= r2 -- the verdict is known -- and writes the mask byte.
// map_clear_kernel    one wavefront per path over the d2 of its map: a wave min-reduction on (d2, index).
//
// Every loop's bound reads off the code (the row's step count, k < ny, the path's length), no block waits for
// another, there are no atomics, and every write is a plain vector store.
#include <climits>
#include <cstdint>

#include "runtime.hpp"

namespace {

constexpr unsigned short MAP_G_NONE = 0xFFFF;  // no blocked cell in the row (never squared)
constexpr int MAP_FAR = 1 << 30;               // "no blocked index yet" of the row scans: MAP_FAR +- x fits int
constexpr int MAP_MAX_STEPS = MP_MAP_MAX_SIDE / 64;  // 64-cell steps of the longest row

// rows = B*ny rows of nx cells; a block's four waves take four adjacent rows.  A step's blocked cells are one
// 64-bit ballot, so the wave-inclusive max-scan of the last blocked index is, for a lane, the highest set bit at or
// below it, and its mirror image the lowest set bit at or above it; the carry is the step's highest (lowest) bit.
// The right-to-left sweep comes first and leaves only its carries, one per step, so that g is written once.
__global__ __launch_bounds__(256) void map_row_kernel(size_t rows, int nx, int border,
                                                      const unsigned char* __restrict__ mask,
                                                      unsigned short* __restrict__ g) {
  __shared__ int right[4][MAP_MAX_STEPS];  // the first blocked index beyond each step of a wave's row
  const int lane = threadIdx.x & 63;
  const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // (wave-uniform; the kernel has no barrier)
  const unsigned char* m = mask + r * nx;
  unsigned short* gr = g + r * nx;
  int* rc = right[threadIdx.x >> 6];
  const int steps = (nx + 63) / 64;
  // Both sweeps take four steps a turn: the four loads (clamped into the row, so unconditional) are in flight
  // together, and a step outside the row has an empty ballot.
  // right to left: the first blocked index at or after x (the frame's cell is index nx).  Every lane writes the
  // wave-uniform carry, so each lane later reads a word it wrote itself.
  int carry = border ? nx : MAP_FAR;
  for (int s0 = steps - 1; s0 >= 0; s0 -= 4) {
    unsigned char v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = m[min(max((s0 - j) * 64 + lane, 0), nx - 1)];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int s = s0 - j, x = s * 64 + lane;
      if (s >= 0) rc[s] = carry;
      const unsigned long long bits = __ballot((unsigned)x < (unsigned)nx && v[j] == 0);
      if (bits) carry = s * 64 + __ffsll(bits) - 1;
    }
  }
  // left to right: the last blocked index at or before x (the frame's cell is index -1)
  carry = border ? -1 : -MAP_FAR;
  for (int s0 = 0; s0 < steps; s0 += 4) {
    unsigned char v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = m[min((s0 + j) * 64 + lane, nx - 1)];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int s = s0 + j, x = s * 64 + lane;
      const unsigned long long bits = __ballot(x < nx && v[j] == 0);
      const unsigned long long le = bits & (~0ull >> (63 - lane)), ge = bits >> lane;
      const int last = le ? s * 64 + 63 - __clzll(le) : carry;
      const int next = ge ? x + __ffsll(ge) - 1 : rc[min(s, steps - 1)];
      if (x < nx) gr[x] = (unsigned short)min(min(x - last, next - x), (int)MAP_G_NONE);
      if (bits) carry = s * 64 + 63 - __clzll(bits);
    }
  }
}

// blockIdx.x = (map * tiles_y + tile_y) * tiles_x + tile_x; a tile is 64 cells of x by 4 rows
template <bool CAPPED>
__global__ __launch_bounds__(256) void map_col_kernel(int nx, int ny, int tiles_x, int tiles_y, int border,
                                                      int occupied, const unsigned short* __restrict__ g,
                                                      const int* __restrict__ r2, int* __restrict__ d2,
                                                      unsigned char* __restrict__ out) {
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
  const size_t b = blockIdx.x / tiles_x / tiles_y;
  const int x = tx * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
  if (x >= nx || y >= ny) return;
  const size_t cell = (b * ny + y) * nx + x;
  const unsigned short* gc = g + cell;  // g(x, y +- k) = gc[+- k*nx]
  int best = MP_MAP_D2_NONE;
  if (border) {
    const int e = min(y + 1, ny - y);
    best = e * e;
  }
  const int g0 = gc[0];
  if (g0 != MAP_G_NONE) best = min(best, g0 * g0);
  const int cap = CAPPED ? r2[b] : 0;
  for (int k = 1; k < ny; k++) {
    const int kk = k * k;
    if (kk >= best) break;
    if (CAPPED && (kk > cap || best <= cap)) break;
    if (y >= k) {
      const int gv = gc[-(ptrdiff_t)k * nx];
      if (gv != MAP_G_NONE) best = min(best, gv * gv + kk);
    }
    if (y + k < ny) {
      const int gv = gc[(ptrdiff_t)k * nx];
      if (gv != MAP_G_NONE) best = min(best, gv * gv + kk);
    }
  }
  if (CAPPED) {  // (a blocked cell has best = 0 <= r2)
    const int is_free = best > cap;
    out[cell] = (unsigned char)(occupied ? !is_free : is_free);
  } else {
    d2[cell] = best;
  }
}

// one wavefront per path, four paths a block
__global__ __launch_bounds__(256) void map_clear_kernel(int B, int N, int stride, const int* __restrict__ d2,
                                                        const int* __restrict__ path, const int* __restrict__ path_n,
                                                        int* __restrict__ min_d2, int* __restrict__ at) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int* p = path + (size_t)b * stride;
  const int* d = d2 + (size_t)b * N;
  const int n = path_n[b];
  int best = MP_MAP_D2_NONE, idx = INT_MAX;  // INT_MAX: no entry yet
  for (int i = lane; i < n; i += 64) {
    const int e = p[i];
    if (e == 0) continue;  // a start off the map
    const int v = d[e - 1];
    if (idx == INT_MAX || v < best) {
      best = v;
      idx = i;
    }
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int ov = __shfl_xor(best, s, 64), oi = __shfl_xor(idx, s, 64);
    if (ov < best || (ov == best && oi < idx)) {
      best = ov;
      idx = oi;
    }
  }
  if (lane == 0) {
    min_d2[b] = best;
    at[b] = idx == INT_MAX ? -1 : idx;
  }
}

// ---------------------------------------------------------------- host
int map_check(mp_ctx* ctx, int flags, int known, int B, int nx, int ny) {
  MP_CHECK(ctx, (flags & ~known) == 0, "unknown flags");
  MP_CHECK(ctx, nx >= 2 && ny >= 2 && (long long)nx * ny <= MP_GRID_MAX_CELLS && nx <= MP_MAP_MAX_SIDE &&
                    ny <= MP_MAP_MAX_SIDE,
           "map %d x %d: each side must be 2 .. %d and nx*ny <= %d", nx, ny, MP_MAP_MAX_SIDE, MP_GRID_MAX_CELLS);
  MP_CHECK(ctx, B >= 1 && (long long)B * nx * ny <= MP_MAP_MAX_BATCH_CELLS, "B = %d maps: B >= 1 and B*nx*ny <= %d", B,
           MP_MAP_MAX_BATCH_CELLS);
  return MP_OK;
}

// the row pass, then the column pass into d2 (r2 null) or, capped by r2, into the mask bytes of out
int map_launch(mp_ctx* ctx, int flags, int B, int nx, int ny, const unsigned char* mask, unsigned short* g,
               const int* r2, int* d2, unsigned char* out) {
  const int border = (flags & MP_MAP_BORDER) != 0;
  const size_t rows = (size_t)B * ny;
  const int tiles_x = (nx + 63) / 64, tiles_y = (ny + 3) / 4;
  const dim3 tiles((unsigned)((size_t)B * tiles_x * tiles_y));  // <= 2^28 / 4 blocks
  mp_time_begin(ctx);
  hipLaunchKernelGGL(map_row_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, ctx->stream, rows, nx, border, mask,
                     g);
  if (r2)
    hipLaunchKernelGGL(map_col_kernel<true>, tiles, dim3(256), 0, ctx->stream, nx, ny, tiles_x, tiles_y, border,
                       (flags & MP_MAP_OUT_OCCUPIED) != 0, g, r2, nullptr, out);
  else
    hipLaunchKernelGGL(map_col_kernel<false>, tiles, dim3(256), 0, ctx->stream, nx, ny, tiles_x, tiles_y, border, 0, g,
                       nullptr, d2, nullptr);
  mp_time_end(ctx);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace

extern "C" {

int mp_grid_distance(mp_ctx* ctx, int32_t flags, int32_t B, int32_t nx, int32_t ny, const uint8_t* mask, int32_t* d2) {
  if (!ctx) return MP_ERR_INVALID;
  int st = map_check(ctx, flags, MP_MAP_BORDER, B, nx, ny);
  if (st) return st;
  MP_CHECK(ctx, mask && d2, "mask or d2 is NULL");
  MP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cells = (size_t)B * nx * ny;
  // every workspace before the first copy or launch
  unsigned char* dm = (unsigned char*)mp_ws(ctx, WS_MAP_MASK, cells);
  unsigned short* g = (unsigned short*)mp_ws(ctx, WS_MAP_ROW, 2 * cells);
  int* dd = (int*)mp_ws(ctx, WS_MAP_D2, 4 * cells);
  if (!dm || !g || !dd) return MP_ERR_NOMEM;
  MP_HIP(ctx, hipMemcpyAsync(dm, mask, cells, hipMemcpyHostToDevice, ctx->stream));
  if ((st = map_launch(ctx, flags, B, nx, ny, dm, g, nullptr, dd, nullptr))) return st;
  if ((st = mp_download(ctx, d2, (const int32_t*)dd, cells))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

int mp_grid_inflate(mp_ctx* ctx, int32_t flags, int32_t B, int32_t nx, int32_t ny, const uint8_t* mask,
                    const int32_t* r2, uint8_t* mask_out) {
  if (!ctx) return MP_ERR_INVALID;
  int st = map_check(ctx, flags, MP_MAP_BORDER | MP_MAP_OUT_OCCUPIED, B, nx, ny);
  if (st) return st;
  MP_CHECK(ctx, mask && r2 && mask_out, "mask, r2 or mask_out is NULL");
  for (int b = 0; b < B; b++) MP_CHECK(ctx, r2[b] >= 0, "r2[%d] = %d is negative", b, r2[b]);
  MP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cells = (size_t)B * nx * ny;
  unsigned char* dm = (unsigned char*)mp_ws(ctx, WS_MAP_MASK, cells);
  unsigned short* g = (unsigned short*)mp_ws(ctx, WS_MAP_ROW, 2 * cells);
  unsigned char* dout = (unsigned char*)mp_ws(ctx, WS_MAP_OUT, cells);
  int* dr = (int*)mp_ws(ctx, WS_MAP_R2, sizeof(int) * (size_t)B);
  if (!dm || !g || !dout || !dr) return MP_ERR_NOMEM;
  MP_HIP(ctx, hipMemcpyAsync(dm, mask, cells, hipMemcpyHostToDevice, ctx->stream));
  MP_HIP(ctx, hipMemcpyAsync(dr, r2, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
  if ((st = map_launch(ctx, flags, B, nx, ny, dm, g, dr, nullptr, dout))) return st;
  if ((st = mp_download(ctx, mask_out, (const uint8_t*)dout, cells))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

int mp_grid_path_clearance(mp_ctx* ctx, int32_t flags, int32_t B, int32_t nx, int32_t ny, const uint8_t* mask,
                           const int32_t* path, const int32_t* path_n, int32_t stride, int32_t* min_d2, int32_t* at) {
  if (!ctx) return MP_ERR_INVALID;
  int st = map_check(ctx, flags, MP_MAP_BORDER, B, nx, ny);
  if (st) return st;
  MP_CHECK(ctx, mask && path && path_n && min_d2 && at, "mask, path, path_n, min_d2 or at is NULL");
  MP_CHECK(ctx, stride >= 1, "stride must be >= 1");
  const int N = nx * ny;
  for (int b = 0; b < B; b++) {  // the device indexes d2 with the entries: they are checked here
    MP_CHECK(ctx, path_n[b] >= 0 && path_n[b] <= stride, "path_n[%d] = %d is outside 0 .. stride", b, path_n[b]);
    const int32_t* p = path + (size_t)b * stride;
    for (int i = 0; i < path_n[b]; i++)
      MP_CHECK(ctx, p[i] >= 0 && p[i] <= N, "path %d, entry %d: %d is outside 0 .. nx*ny", b, i, p[i]);
  }
  MP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cells = (size_t)B * N, nB = (size_t)B;
  unsigned char* dm = (unsigned char*)mp_ws(ctx, WS_MAP_MASK, cells);
  unsigned short* g = (unsigned short*)mp_ws(ctx, WS_MAP_ROW, 2 * cells);
  int* dd = (int*)mp_ws(ctx, WS_MAP_D2, 4 * cells);
  int* dp = (int*)mp_ws(ctx, WS_MAP_PATH, sizeof(int) * nB * stride);
  int* dn = (int*)mp_ws(ctx, WS_MAP_PN, sizeof(int) * nB);
  int* res = (int*)mp_ws(ctx, WS_MAP_RES, sizeof(int) * 2 * nB);
  if (!dm || !g || !dd || !dp || !dn || !res) return MP_ERR_NOMEM;
  MP_HIP(ctx, hipMemcpyAsync(dm, mask, cells, hipMemcpyHostToDevice, ctx->stream));
  MP_HIP(ctx, hipMemcpyAsync(dp, path, sizeof(int) * nB * stride, hipMemcpyHostToDevice, ctx->stream));
  MP_HIP(ctx, hipMemcpyAsync(dn, path_n, sizeof(int) * nB, hipMemcpyHostToDevice, ctx->stream));
  if ((st = map_launch(ctx, flags, B, nx, ny, dm, g, nullptr, dd, nullptr))) return st;
  hipLaunchKernelGGL(map_clear_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, ctx->stream, B, N, stride, dd, dp, dn,
                     res, res + nB);
  MP_HIP(ctx, hipGetLastError());
  if ((st = mp_download(ctx, min_d2, (const int32_t*)res, nB))) return st;
  if ((st = mp_download(ctx, at, (const int32_t*)(res + nB), nB))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

}  // extern "C"
