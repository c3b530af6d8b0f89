// gridfield.hip — goal-distance fields on occupancy maps for gfx950 (an extension, include/mpgpu.h "goal-distance
// fields"): the cost from one source cell to every cell of a map, and paths read off the field + C-ABI: mp_grid_field.
//
// The field is the unique fixed point of f[source] = 0, f[v] = min over moves u -> v of fl(f[u] + c(u -> v)): the
// labels planDKA! leaves once its open list is empty.  Every value a cell ever holds is the left-fold cost of some
// walk from the source, so it is an upper bound of the fixed point, and values only decrease: any order of
// relaxations that ends in a round without a change ends at the same bits.
//
// field_init_kernel    f = +Inf, f[source] = 0; the tiles that hold the source or have it in their halo dirty.
// field_relax_kernel   one workgroup per 64 x 64 tile, a launch per round.  A tile that is not dirty leaves at once.
//                      A dirty one stages its cells and a one-cell halo of f in LDS (66 x 66 doubles), each thread
//                      relaxes its 16 cells against the LDS copy until a sweep changes nothing, then writes back the
//                      cells that decreased: every cell has one writer, the stores are plain 8-byte stores, and a
//                      neighbour that reads the old value reads a valid upper bound.  A changed cell on the tile's
//                      rim marks the tiles that hold it in their halo dirty for the next round.  <true> relaxes the
//                      reversed graph (MP_FIELD_TO_SOURCE).
// field_walk_kernel    one lane per query: q_cost, then the walk from the query's cell by the path rule, a chain of
//                      dependent loads; the path in travel order and the planners' length fold (as_path_length).
//
// The host launches rounds until one changes nothing (the proof of the fixed point: every write is visible across a
// launch boundary), reading a change stamp back through pinned memory.  No workgroup waits for another, there are no
// atomics, and every loop is bounded: the sweeps by the tile's cells, the rounds by nx*ny + 1, a walk by nx*ny.
#include <cstdlib>
#include <cstring>

#define MPJ_LANE_SAFE 1
#include "gridsearch.hpp"

namespace {

constexpr int FT = 64, FW = FT + 2;             // tile side, and with its halo
constexpr int FIELD_THREADS = 256, FIELD_CPT = FT * FT / FIELD_THREADS;  // cells per thread: rows ly, ly + 4, ...
constexpr int FIELD_REC = 12;                   // doubles per map: c(d) of the 8 moves (+Inf: not in the set) | ge[4]
constexpr int FIELD_CHECK_EVERY = 1;            // rounds launched between two reads of the change stamp

// the neighbours in the order of the moves' bits (dka_utils.jl:177's first occurrences, then (-1, +1))
__host__ __device__ constexpr int field_dx(int d) { return d == 0 || d == 1 || d == 7 ? -1 : (d == 5 || d == 6 ? 0 : 1); }
__host__ __device__ constexpr int field_dy(int d) { return d == 1 || d == 2 || d == 5 ? -1 : (d == 0 || d == 3 ? 0 : 1); }

struct FieldArgs {
  int nx, ny, tiles_x, tiles_y;
  size_t tiles;               // B * tiles_x * tiles_y
  double* f;                  // [B][ny][nx]
  const unsigned char* mask;  // [B][ny][nx]
  const double* rec;          // [B][FIELD_REC]
  const int* src;             // [B] the source's cell (0-based), -1 off the grid
  unsigned char* dirty;       // [2][tiles]: round r reads [r & 1] and marks [(r + 1) & 1]
  int* cnt;                   // [tiles] finite cells of the tile
  int* stamp;                 // [0] 1 + the last round that changed a cell; [1] a walk found no way on
};

__global__ __launch_bounds__(256) void field_init_kernel(FieldArgs A, size_t cells) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const size_t N = (size_t)A.nx * A.ny, b = i / N;
  const int c = (int)(i - b * N);
  const bool is_src = c == A.src[b];
  A.f[i] = is_src ? 0.0 : __builtin_inf();
  if (!is_src) return;
  // round 0 is due in every tile that holds the source or has it in its halo: the tiles of the source's neighbours
  const int sx = c % A.nx, sy = c / A.nx;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const int x = sx + dx, y = sy + dy;
      if (x >= 0 && x < A.nx && y >= 0 && y < A.ny) A.dirty[(b * A.tiles_y + y / FT) * A.tiles_x + x / FT] = 1;
    }
}

// blockIdx.x = (map * tiles_y + tile_y) * tiles_x + tile_x
template <bool TO_SOURCE>
__global__ __launch_bounds__(FIELD_THREADS) void field_relax_kernel(FieldArgs A, int round) {
  __shared__ double s_f[FW * FW];
  __shared__ int s_cnt[FIELD_THREADS / 64];
  __shared__ int s_go;
  const int tid = threadIdx.x;
  const size_t tile = blockIdx.x;
  unsigned char* dcur = A.dirty + (size_t)(round & 1) * A.tiles;
  unsigned char* dnext = A.dirty + (size_t)((round + 1) & 1) * A.tiles;
  if (tid == 0) s_go = dcur[tile];
  __syncthreads();
  if (!s_go) return;  // (block-uniform)
  if (tid == 0) dcur[tile] = 0;  // this block is the flag's only reader; it is marked again in the other half
  const int nx = A.nx, ny = A.ny;
  const int tx = (int)(tile % A.tiles_x), ty = (int)(tile / A.tiles_x % A.tiles_y);
  const size_t b = tile / A.tiles_x / A.tiles_y;
  const int x0 = tx * FT, y0 = ty * FT;
  double* f = A.f + b * (size_t)nx * ny;
  const unsigned char* mk = A.mask + b * (size_t)nx * ny;
  const double* rec = A.rec + b * FIELD_REC;
  const int src = A.src[b];
  for (int i = tid; i < FW * FW; i += FIELD_THREADS) {
    const int gx = x0 + i % FW - 1, gy = y0 + i / FW - 1;
    s_f[i] = (gx >= 0 && gx < nx && gy >= 0 && gy < ny) ? f[(size_t)gy * nx + gx] : __builtin_inf();
  }
  double c[8];
#pragma unroll
  for (int d = 0; d < 8; d++) c[d] = rec[d];
  // this thread's cells: column lx, rows ly + 4k.  Only members are relaxed; the rest keep their +Inf.
  const int lx = tid & 63, ly = tid >> 6, gx = x0 + lx;
  const int base = (ly + 1) * FW + lx + 1;
  unsigned int member = 0;
#pragma unroll
  for (int k = 0; k < FIELD_CPT; k++) {
    const int gy = y0 + ly + 4 * k;
    if (gx < nx && gy < ny) {
      const int cell = gy * nx + gx;
      if (mk[cell] != 0 || cell == src) member |= 1u << k;
    }
  }
  __syncthreads();
  // Sweeps race inside the tile, and that is harmless: a value read is an upper bound whenever it is read, and the
  // sweep that ends the loop wrote nothing, so every one of its reads saw the final values.
  for (int it = 0; it <= FT * FT; it++) {
    int changed = 0;
#pragma unroll
    for (int k = 0; k < FIELD_CPT; k++) {
      if (!((member >> k) & 1)) continue;
      const int idx = base + 4 * k * FW;
      const double cur = s_f[idx];
      double best = cur;
#pragma unroll
      for (int d = 0; d < 8; d++) {
        const int off = field_dy(d) * FW + field_dx(d);
        const double v = s_f[TO_SOURCE ? idx + off : idx - off] + c[d];
        if (v < best) best = v;
      }
      if (best < cur) {
        s_f[idx] = best;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  // write back what decreased; a changed rim cell is in the halo of up to three other tiles
  int wrote = 0, finite = 0;
#pragma unroll
  for (int k = 0; k < FIELD_CPT; k++) {
    const int yy = ly + 4 * k, gy = y0 + yy;
    if (gx >= nx || gy >= ny) continue;
    const double v = s_f[base + 4 * k * FW];
    finite += v < __builtin_inf();
    const size_t cell = (size_t)gy * nx + gx;
    if (!(v < f[cell])) continue;
    f[cell] = v;
    wrote = 1;
    const bool w = lx == 0 && tx > 0, e = lx == FT - 1 && tx + 1 < A.tiles_x;
    const bool n = yy == 0 && ty > 0, s = yy == FT - 1 && ty + 1 < A.tiles_y;
    if (w) dnext[tile - 1] = 1;
    if (e) dnext[tile + 1] = 1;
    if (n) dnext[tile - A.tiles_x] = 1;
    if (s) dnext[tile + A.tiles_x] = 1;
    if (n && w) dnext[tile - A.tiles_x - 1] = 1;
    if (n && e) dnext[tile - A.tiles_x + 1] = 1;
    if (s && w) dnext[tile + A.tiles_x - 1] = 1;
    if (s && e) dnext[tile + A.tiles_x + 1] = 1;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) finite += __shfl_xor(finite, off);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = finite;
  const int any = __syncthreads_or(wrote);
  if (tid == 0) {
    A.cnt[tile] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (any) A.stamp[0] = round + 1;
  }
}

struct WalkArgs {
  int nx, ny, Q, stride, moves, to_source;
  const double* f;
  const double* rec;
  const int* src;
  const int* q_map;        // [Q]
  const int* q_cell;       // [Q] Encode index of the query's cell, 0 off the grid
  const long long* q_off;  // [Q + 1] the walk's place in `walk`
  int* walk;               // the cells in walk order, Encode indices
  double* q_cost;          // [Q]
  int* path;               // [Q][stride], or null: costs only
  int* path_n;             // [Q]
  double* path_len;        // [Q]
  int* err;
};

__global__ __launch_bounds__(64) void field_walk_kernel(WalkArgs A) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= A.Q) return;
  const int nx = A.nx, ny = A.ny, N = nx * ny;
  const int b = A.q_map[q], e = A.q_cell[q];
  const double* f = A.f + (size_t)b * N;
  const double cost = e ? f[e - 1] : __builtin_inf();
  A.q_cost[q] = cost;
  if (!A.path) return;
  const double* rec = A.rec + (size_t)b * FIELD_REC;
  int* w = A.walk + A.q_off[q];
  const int cap = (int)(A.q_off[q + 1] - A.q_off[q]);
  const int src = A.src[b];
  int n = 0;
  if (cost < __builtin_inf()) {
    int v = e - 1;
    bool ok = false;
    for (int step = 0; step < N && n < cap; step++) {
      w[n++] = v + 1;
      if (v == src) {
        ok = true;
        break;
      }
      const double fv = f[v];
      const int vx = v % nx, vy = v / nx;
      int u = -1;
#pragma unroll
      for (int d = 7; d >= 0; d--) {  // (downwards: the lowest bit is assigned last)
        if (!((A.moves >> d) & 1)) continue;
        const int ux = A.to_source ? vx + field_dx(d) : vx - field_dx(d);
        const int uy = A.to_source ? vy + field_dy(d) : vy - field_dy(d);
        if (ux < 0 || ux >= nx || uy < 0 || uy >= ny) continue;
        const int uc = uy * nx + ux;
        if (f[uc] + rec[d] == fv) u = uc;  // (fv is finite, so f[uc] is: a member that was reached)
      }
      if (u < 0) break;
      v = u;
    }
    if (!ok) {
      *A.err = 1;
      n = 0;
    }
  }
  const int m = n < A.stride ? n : A.stride;
  int* p = A.path + (size_t)q * A.stride;
  if (A.to_source) {  // walked in travel order; the fold takes the far end first
    for (int i = 0; i < m; i++) p[i] = w[i];
    for (int i = 0; i < n / 2; i++) {
      const int t = w[i];
      w[i] = w[n - 1 - i];
      w[n - 1 - i] = t;
    }
  } else {
    for (int i = 0; i < m; i++) p[i] = w[n - 1 - i];
  }
  A.path_n[q] = n;
  A.path_len[q] = as_path_length(w, n, nx, 0, 0, rec[10], rec[11], rec + 8);
}

int field_check_every() {
  const char* s = std::getenv("MPGPU_FIELD_CHECK_EVERY");  // tools/gridfield_time.py measures the choice
  const int k = s ? std::atoi(s) : FIELD_CHECK_EVERY;
  return k < 1 ? 1 : (k > 64 ? 64 : k);
}

}  // namespace

extern "C" {

int mp_grid_field(mp_ctx* ctx, int32_t flags, int32_t moves, int32_t B, int32_t nx, int32_t ny, const double* bound,
                  const double* source_real, const uint8_t* mask, double* field, int32_t* n_reached, int32_t Q,
                  const int32_t* q_map, const double* q_real, int32_t stride, double* q_cost, int32_t* path,
                  int32_t* path_n, double* path_length) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, (flags & ~MP_FIELD_TO_SOURCE) == 0, "unknown flags");
  MP_CHECK(ctx, moves >= 1 && moves <= 0xFF, "moves = %d: a set of 1 .. 8 of the moves, 0x01 .. 0xFF", moves);
  MP_CHECK(ctx, nx >= 2 && ny >= 2 && (long long)nx * ny <= MP_GRID_MAX_CELLS,
           "grid %d x %d: each side must be >= 2 and nx*ny <= %d", nx, ny, MP_GRID_MAX_CELLS);
  MP_CHECK(ctx, B >= 1 && (long long)B * nx * ny <= MP_FIELD_MAX_BATCH_CELLS, "B = %d maps: B >= 1 and B*nx*ny <= %d", B,
           MP_FIELD_MAX_BATCH_CELLS);
  MP_CHECK(ctx, bound && source_real && mask, "bound, source_real or mask is NULL");
  MP_CHECK(ctx, Q >= 0, "Q must be >= 0");
  const bool paths = path != nullptr;
  if (Q == 0) {
    MP_CHECK(ctx, !q_map && !q_real && !q_cost && !path && !path_n && !path_length, "Q = 0 takes no query pointer");
  } else {
    MP_CHECK(ctx, q_map && q_real && q_cost, "Q > 0 needs q_map, q_real and q_cost");
    MP_CHECK(ctx, paths == (path_n != nullptr) && paths == (path_length != nullptr),
             "path, path_n and path_length go together");
    MP_CHECK(ctx, !paths || stride >= 1, "stride must be >= 1");
  }
  MP_CHECK(ctx, field || n_reached || Q > 0, "no output asked for");
  const int N = nx * ny;
  const size_t nB = (size_t)B, nQ = (size_t)Q, cells = nB * N;
  MP_CHECK(ctx, mp_all_finite(source_real, 2 * nB), "source_real must be finite");
  std::vector<double> rec(FIELD_REC * nB);
  std::vector<int> src(nB);
  for (int b = 0; b < B; b++) {
    double* r = &rec[FIELD_REC * (size_t)b];
    double* ge = r + 8;
    MP_CHECK(ctx, as_factors(bound + 4 * (size_t)b, nx, ny, ge) && ge[2] > 0.0 && ge[3] > 0.0,
             "bound %d must be finite with xmax > xmin and ymax > ymin", b);
    const double xf2 = ge[2] * ge[2], yf2 = ge[3] * ge[3];
    for (int d = 0; d < 8; d++) {  // dka_utils.jl:189
      const int dx = field_dx(d), dy = field_dy(d);
      r[d] = (moves >> d) & 1 ? std::sqrt((double)(dx * dx) * xf2 + (double)(dy * dy) * yf2) : INFINITY;
      MP_CHECK(ctx, !((moves >> d) & 1) || (std::isfinite(r[d]) && r[d] > 0.0), "map %d: the cost of move %d is not positive and finite", b, d);
    }
    int sc[2];
    const bool on = as_cell(ge, source_real + 2 * (size_t)b, sc) && sc[0] >= 1 && sc[0] <= nx && sc[1] >= 1 && sc[1] <= ny;
    src[b] = on ? (sc[1] - 1) * nx + sc[0] - 1 : -1;  // Encode - 1
  }
  std::vector<int> qcell(nQ);
  std::vector<long long> qoff(nQ + 1, 0);
  if (Q > 0) {
    MP_CHECK(ctx, mp_all_finite(q_real, 2 * nQ), "q_real must be finite");
    for (int q = 0; q < Q; q++) {
      MP_CHECK(ctx, q_map[q] >= 0 && q_map[q] < B, "q_map[%d] = %d is outside 0 .. B-1", q, q_map[q]);
      int c[2];
      const bool on = as_cell(&rec[FIELD_REC * (size_t)q_map[q] + 8], q_real + 2 * (size_t)q, c) && c[0] >= 1 && c[0] <= nx &&
                      c[1] >= 1 && c[1] <= ny;
      qcell[q] = on ? (c[1] - 1) * nx + c[0] : 0;  // Encode
    }
  }
  if (paths) {  // a walk visits each member of its map at most once
    std::vector<long long> members(nB, -1);
    for (int q = 0; q < Q; q++) {
      long long& m = members[q_map[q]];
      if (m < 0) {
        const uint8_t* mk = mask + (size_t)q_map[q] * N;
        m = 1;  // (the source)
        for (int i = 0; i < N; i++) m += mk[i] != 0;
        if (m > N) m = N;
      }
      qoff[q + 1] = qoff[q] + m;
    }
  }
  MP_HIP(ctx, hipSetDevice(ctx->device));
  // every workspace before the first copy or launch
  const int tiles_x = (nx + FT - 1) / FT, tiles_y = (ny + FT - 1) / FT;
  const size_t tiles = nB * tiles_x * tiles_y;
  double* df = (double*)mp_ws(ctx, WS_FIELD_F, sizeof(double) * cells);
  unsigned char* dm = (unsigned char*)mp_ws(ctx, WS_FIELD_MASK, cells);
  // [rec B*12 doubles | src B ints]
  char* dmap = (char*)mp_ws(ctx, WS_FIELD_MAP, (sizeof(double) * FIELD_REC + sizeof(int)) * nB);
  // [cnt tiles ints | stamp 2 ints | dirty 2*tiles bytes]
  char* dtile = (char*)mp_ws(ctx, WS_FIELD_TILE, sizeof(int) * (tiles + 2) + 2 * tiles);
  // [q_off Q+1 int64 | q_cost Q doubles | path_len Q doubles | q_map, q_cell, path_n Q ints each]
  char* dq = Q ? (char*)mp_ws(ctx, WS_FIELD_Q, 8 * (nQ + 1) + 16 * nQ + 12 * nQ) : nullptr;
  int* dpath = paths ? (int*)mp_ws(ctx, WS_FIELD_PATH, sizeof(int) * nQ * stride) : nullptr;
  int* dwalk = paths ? (int*)mp_ws(ctx, WS_FIELD_WALK, sizeof(int) * (size_t)qoff[nQ]) : nullptr;
  int* pin = (int*)mp_pinned(ctx, 2 * sizeof(int));
  if (!df || !dm || !dmap || !dtile || (Q && !dq) || (paths && (!dpath || !dwalk))) return MP_ERR_NOMEM;
  if (!pin) return mp_fail(ctx, MP_ERR_NOMEM, "no pinned memory for the change stamp");
  FieldArgs A{};
  A.nx = nx;
  A.ny = ny;
  A.tiles_x = tiles_x;
  A.tiles_y = tiles_y;
  A.tiles = tiles;
  A.f = df;
  A.mask = dm;
  A.rec = (double*)dmap;
  A.src = (int*)(dmap + sizeof(double) * FIELD_REC * nB);
  A.cnt = (int*)dtile;
  A.stamp = A.cnt + tiles;
  A.dirty = (unsigned char*)(A.stamp + 2);
  MP_HIP(ctx, hipMemcpyAsync(dm, mask, cells, hipMemcpyHostToDevice, ctx->stream));
  MP_HIP(ctx, hipMemcpyAsync((void*)A.rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice, ctx->stream));
  MP_HIP(ctx, hipMemcpyAsync((void*)A.src, src.data(), sizeof(int) * nB, hipMemcpyHostToDevice, ctx->stream));
  MP_HIP(ctx, hipMemsetAsync(dtile, 0, sizeof(int) * (tiles + 2) + 2 * tiles, ctx->stream));
  hipLaunchKernelGGL(field_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, A, cells);
  MP_HIP(ctx, hipGetLastError());
  // rounds until one changes nothing
  const long long max_rounds = (long long)N + 1;
  const int every = field_check_every();
  const bool to_source = (flags & MP_FIELD_TO_SOURCE) != 0;
  for (long long r = 0;;) {
    const long long r_end = r + every < max_rounds ? r + every : max_rounds;
    for (; r < r_end; r++) {
      mp_time_begin(ctx);
      if (to_source)
        hipLaunchKernelGGL(field_relax_kernel<true>, dim3((unsigned)tiles), dim3(FIELD_THREADS), 0, ctx->stream, A, (int)r);
      else
        hipLaunchKernelGGL(field_relax_kernel<false>, dim3((unsigned)tiles), dim3(FIELD_THREADS), 0, ctx->stream, A, (int)r);
      mp_time_end(ctx);
    }
    MP_HIP(ctx, hipGetLastError());
    MP_HIP(ctx, hipMemcpyAsync(pin, A.stamp, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (pin[0] < r) break;  // round r - 1 changed nothing
    if (r >= max_rounds) return mp_fail(ctx, MP_ERR_NUMERIC, "mp_grid_field: no fixed point after nx*ny + 1 rounds");
  }
  WalkArgs W{};
  if (Q) {
    W.nx = nx;
    W.ny = ny;
    W.Q = Q;
    W.stride = stride;
    W.moves = moves;
    W.to_source = to_source;
    W.f = df;
    W.rec = A.rec;
    W.src = A.src;
    long long* doff = (long long*)dq;
    W.q_off = doff;
    W.q_cost = (double*)(doff + nQ + 1);
    W.path_len = W.q_cost + nQ;
    int* dqm = (int*)(W.path_len + nQ);
    W.q_map = dqm;
    W.q_cell = dqm + nQ;
    W.path_n = dqm + 2 * nQ;
    W.walk = dwalk;
    W.path = dpath;
    W.err = A.stamp + 1;
    MP_HIP(ctx, hipMemcpyAsync(doff, qoff.data(), 8 * (nQ + 1), hipMemcpyHostToDevice, ctx->stream));
    MP_HIP(ctx, hipMemcpyAsync(dqm, q_map, sizeof(int) * nQ, hipMemcpyHostToDevice, ctx->stream));
    MP_HIP(ctx, hipMemcpyAsync(dqm + nQ, qcell.data(), sizeof(int) * nQ, hipMemcpyHostToDevice, ctx->stream));
    mp_time_begin(ctx);
    hipLaunchKernelGGL(field_walk_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, ctx->stream, W);
    mp_time_end(ctx);
    MP_HIP(ctx, hipGetLastError());
    MP_HIP(ctx, hipMemcpyAsync(pin + 1, W.err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (pin[1]) return mp_fail(ctx, MP_ERR_NUMERIC, "mp_grid_field: a walk found no way on (the field is no fixed point)");
  }
  // outputs: nothing has been written so far
  int st;
  if ((st = mp_download(ctx, field, (const double*)df, cells))) return st;
  std::vector<int> cnt(n_reached ? tiles : 0), pn(paths ? nQ : 0), pbuf(paths ? nQ * stride : 0);
  if ((st = mp_download(ctx, n_reached ? cnt.data() : nullptr, (const int*)A.cnt, tiles))) return st;
  if (Q) {
    if ((st = mp_download(ctx, q_cost, (const double*)W.q_cost, nQ))) return st;
    if ((st = mp_download(ctx, path_length, (const double*)W.path_len, nQ))) return st;
    if ((st = mp_download(ctx, paths ? pn.data() : nullptr, (const int*)W.path_n, nQ))) return st;
    if ((st = mp_download(ctx, paths ? pbuf.data() : nullptr, (const int*)dpath, nQ * stride))) return st;
  }
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_reached) {
    const size_t per = (size_t)tiles_x * tiles_y;
    for (size_t b = 0; b < nB; b++) {
      int s = 0;
      for (size_t t = 0; t < per; t++) s += cnt[b * per + t];
      n_reached[b] = s;
    }
  }
  if (paths)
    for (size_t q = 0; q < nQ; q++) {  // only the entries that exist
      path_n[q] = pn[q];
      const size_t m = pn[q] < stride ? pn[q] : stride;
      std::memcpy(path + q * stride, &pbuf[q * stride], sizeof(int) * m);
    }
  return MP_OK;
}

}  // extern "C"
