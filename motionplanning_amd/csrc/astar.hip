// astar.hip — the grid planners for gfx950: A* (PathPlanning/Astar/src/{setup,astar_utils}.jl,
// CollisionDetection/src/utils.jl), Dijkstra (PathPlanning/Dijkstra/src/dka_utils.jl) and breadth-first search
// (PathPlanning/BreadthFirst/src/bfs_utils.jl) + C-ABI: mp_astar_plan, mp_dka_plan, mp_bfs_plan (B independent
// planAstar! / planDKA! / planBFS! searches) and mp_ha_astar_table (Hybrid A*'s astar_heuristic,
// hybrid_astar_utils.jl:375-387, for every cell).
//
// as_wall_kernel    Block2Pts: the 2x5 corner points of every block obstacle, once per scene.
// as_mask_kernel    checkObsSafety for every cell of every scene, once per scene (one thread per cell):
//                   a search only reads the scene's free-cell mask.
// as_search_kernel  planAstar! + FindNewNode, one wavefront per search, the node table (Dict) and the
//                   open list in LDS, no global hand-offs.  A scene's searches (one in plan mode, one per
//                   start cell in table mode) share its mask.  as_search_kernel<true> is planDKA!: h = 0, so
//                   f is g and one array holds both.
// bfs_search_kernel planBFS! + FindNewNode, one wavefront per search, level by level: the FIFO never sorts
//                   and a cell enters it once, so the queue is the pop sequence and a whole level expands
//                   at once in the sequential loop's order.
// mp_grid_plan is the same host side (as_plan) without the 51 x 51 limit and with caller-supplied masks: above
// the limit, or when forced, as_launch hands the searches to gridbig.hip's global-memory kernels.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#define MPJ_LANE_SAFE 1
#include "../../include/mp_jlmath.h"
#include "gridsearch.hpp"
#include "runtime.hpp"

namespace {

constexpr int AS_MAX_CELLS = 51 * 51;  // the node table of one search must fit one block's LDS
constexpr int AS_HA_N = 11;            // astar_heuristic's mapbound [11, 11]
constexpr double AS_EPS = 1e-1;        // checkObsSafety's epsilon (astar_utils.jl:267)
enum { ST_FREE = 1, ST_EXIST = 2, ST_OPEN = 4 };
constexpr unsigned short AS_NOPAR = 0xFFFF;
// LDS of one search, M = cells + 1 slots (slot 0: a start cell off the grid, Encode = 0): g, f and the
// open list's sort keys (double), parent and two open-list buffers (uint16), the state bits (uint8)
// (Dijkstra: f is g, two double arrays)
constexpr size_t as_lds_bytes(int M, bool dka = false) { return (size_t)M * ((dka ? 2 : 3) * 8 + 3 * 2 + 1); }
// ... of one breadth-first search: the claim word (uint32), parent and queue (uint16), the state bits (uint8)
constexpr size_t bfs_lds_bytes(int M) { return (size_t)M * (4 + 2 * 2 + 1); }

// The reference's BLAS-dispatched products round as Julia's OpenBLAS does (oracle/or_blas.h), as in
// hastar.hip: R*pts is dgemm with K = 2, transpose(pts .- bg_pt)*normal_vec is dgemv 'T' on two rows.
__device__ __forceinline__ double as_dp(double mx, double my, double nx, double ny) {
  return __builtin_fma(mx, nx, my * ny);
}
__device__ __forceinline__ void as_rect_pts(double ox, double oy, double c, double s, double l, double w, double* pts) {
  const double px[5] = {-l, -l, l, l, -l}, py[5] = {w, -w, -w, w, w};
#pragma unroll
  for (int j = 0; j < 5; j++) {
    pts[2 * j] = __builtin_fma(-s, py[j], c * px[j]) + ox;
    pts[2 * j + 1] = __builtin_fma(c, py[j], s * px[j]) + oy;
  }
}

// SeparatingAxisTheorem (utils.jl:37-62) on an NB-point base (NB - 1 edges) and an NO-point other
template <int NB, int NO>
__device__ __forceinline__ int as_sat(const double* base, const double* other) {
  for (int e = 0; e < NB - 1; e++) {
    const double bx = base[2 * e], by = base[2 * e + 1];
    const double vx = base[2 * e + 2] - bx, vy = base[2 * e + 3] - by;
    const double nx = -vy, ny = vx;
    double mnb = 0, mxb = 0, mno = 0, mxo = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const double d = as_dp(base[2 * j] - bx, base[2 * j + 1] - by, nx, ny);
      if (j == 0 || d < mnb) mnb = d;
      if (j == 0 || d > mxb) mxb = d;
    }
#pragma unroll
    for (int j = 0; j < NO; j++) {
      const double d = as_dp(other[2 * j] - bx, other[2 * j + 1] - by, nx, ny);
      if (j == 0 || d < mno) mno = d;
      if (j == 0 || d > mxo) mxo = d;
    }
    if ((mxo <= mnb) || (mxb <= mno)) return 1;
  }
  return 0;
}

__global__ __launch_bounds__(64) void as_wall_kernel(int n, const double* __restrict__ obs, double* __restrict__ wpts) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double* o = obs + (size_t)i * 5;
  as_rect_pts(o[0], o[1], mpj_cos(o[2]), mpj_sin(o[2]), o[3], o[4], wpts + (size_t)i * 10);
}

// geo[scene][4] = xmin, ymin, x_factor, y_factor; mask[scene][ny][nx] (cell (ix, iy) at (iy-1)*nx + ix-1)
__global__ __launch_bounds__(256) void as_mask_kernel(int scenes, int nx, int ny, const double* __restrict__ geo,
                                                      int kind, int n_obs, const double* __restrict__ obs,
                                                      const double* __restrict__ wpts,
                                                      unsigned char* __restrict__ mask) {
  const int N = nx * ny;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)scenes * N) return;
  const int s = (int)(i / N), c = (int)(i % N);
  const int ix = c % nx + 1, iy = c / nx + 1;
  const double* ge = geo + (size_t)s * 4;
  // TransferCoordinate (astar_utils.jl:237-240)
  const double tx = ((double)ix - 1.0) * ge[2] + ge[0], ty = ((double)iy - 1.0) * ge[3] + ge[1];
  int ok = 1;
  if (kind == 3) {
    for (int k = 0; k < n_obs && ok; k++) {
      const double* o = obs + ((size_t)s * n_obs + k) * 3;
      const double dx = tx - o[0], dy = ty - o[1];
      if (dx * dx + dy * dy < o[2] * o[2]) ok = 0;
    }
  } else {
    // mypts (:268): the first and last point coincide, there is no (x, y - eps)
    const double mp[8] = {tx, ty + AS_EPS, tx - AS_EPS, ty, tx + AS_EPS, ty, tx, ty + AS_EPS};
    for (int k = 0; k < n_obs && ok; k++) {
      const double* w = wpts + ((size_t)s * n_obs + k) * 10;
      // ConvexCollision(wall, mypts) (utils.jl:64-74): both directions must separate
      if (!(as_sat<5, 4>(w, mp) && as_sat<4, 5>(mp, w))) ok = 0;
    }
  }
  mask[i] = (unsigned char)ok;
}

// FindNewNode's directions as written (astar_utils.jl:192); entries 2 and 7 repeat 1 and 3: a repeat finds
// the node its first occurrence just wrote with the same tentative g and changes nothing
__device__ const signed char AS_DX[9] = {-1, -1, -1, 1, 1, 1, 0, 1, 0};
__device__ const signed char AS_DY[9] = {0, -1, -1, -1, 0, 1, -1, -1, 1};

// DKA: planDKA! (dka_utils.jl:69-126, FindNewNode :175-215) -- the same directions, sort and InOpen rule with
// no temp_h: f = g + 0.0 = g exactly, so f aliases g and the update test reads f (:193)
template <bool DKA>
__global__ __launch_bounds__(64) void as_search_kernel(AsArgs A) {
  extern __shared__ double as_sm[];
  __shared__ int s_cur;
  const int nx = A.nx, ny = A.ny, N = nx * ny, M = N + 1;
  const int lane = threadIdx.x, q = blockIdx.x, scene = q / A.per_scene;
  double* g = as_sm;
  double* f = DKA ? g : g + M;
  double* kf = f + M;
  unsigned short* par = reinterpret_cast<unsigned short*>(kf + M);
  unsigned short* cur_o = par + M;
  unsigned short* nxt_o = cur_o + M;
  unsigned char* st = reinterpret_cast<unsigned char*>(nxt_o + M);
  const double* ge = A.geo + (size_t)scene * 4;
  const double xf = ge[2], yf = ge[3];
  const double xf2 = xf * xf, yf2 = yf * yf;
  int sx, sy;
  if (A.per_scene == 1) {
    sx = A.scell[2 * q];
    sy = A.scell[2 * q + 1];
  } else {
    const int c = q % A.per_scene;
    sx = c % nx + 1;
    sy = c / nx + 1;
  }
  const int gx = A.gcell[2 * scene], gy = A.gcell[2 * scene + 1];
  const unsigned char* mk = A.mask + (size_t)scene * N;
  for (int i = lane; i < M; i += 64) st[i] = (i > 0 && mk[i - 1]) ? ST_FREE : 0;
  __syncthreads();
  // Encode (astar_utils.jl:176-188)
  const int s_enc = (sx < 1 || sx > nx || sy < 1 || sy > ny) ? 0 : (sy - 1) * nx + sx;
  if (lane == 0) {  // starting_node (setup.jl:19,22): g = h = f = 0, in nodes_collection and the open list
    g[s_enc] = 0.0;
    f[s_enc] = 0.0;
    par[s_enc] = AS_NOPAR;
    st[s_enc] |= ST_EXIST | ST_OPEN;
    cur_o[0] = (unsigned short)s_enc;
  }
  __syncthreads();
  int n_open = 1, nn = 1, loop = 0, found = 0, capped = 0, last = -1;
  double fc = 0.0;
  int* pseq = A.pop_seq ? A.pop_seq + (size_t)q * A.cap : nullptr;
  while (n_open > 0) {
    if (loop >= A.cap) {
      capped = 1;
      break;
    }
    loop++;
    // sort!(open_list) (stable, by isless on f) + popfirst!: every entry's rank among the others
    for (int i = lane; i < n_open; i += 64) kf[i] = f[cur_o[i]];
    __syncthreads();
    for (int i = lane; i < n_open; i += 64) {
      const double fi = kf[i];
      int r = 0;
      for (int j = 0; j < n_open; j++) {
        const double fj = kf[j];
        r += mpj_isless(fj, fi) | (!mpj_isless(fi, fj) & (j < i));
      }
      const unsigned short c = cur_o[i];
      if (r == 0)
        s_cur = c;
      else
        nxt_o[r - 1] = c;
    }
    __syncthreads();
    const int cur = s_cur;
    n_open--;
    {
      unsigned short* t = cur_o;
      cur_o = nxt_o;
      nxt_o = t;
    }
    const int cx = cur == 0 ? sx : (cur - 1) % nx + 1, cy = cur == 0 ? sy : (cur - 1) / nx + 1;
    if (lane == 0) {
      st[cur] &= ~ST_OPEN;
      if (pseq) pseq[loop - 1] = cur;
    }
    if (cx == gx && cy == gy) {  // :107-108 (start == goal: cost 0, found -- the reference throws at :110)
      found = 1;
      fc = g[cur];
      last = cur;
      break;
    }
    // FindNewNode (:190-235): the seven distinct directions touch seven distinct cells, one lane each;
    // push! order is direction order (the ballot prefix)
    const double gc = g[cur];
    bool app = false, isnew = false;
    int ncell = 0;
    if (lane < 9 && lane != 2 && lane != 7) {
      const int dx = AS_DX[lane], dy = AS_DY[lane];
      const int px = cx + dx, py = cy + dy;
      if (px >= 1 && px <= nx && py >= 1 && py <= ny) {  // checkPositionValidity (:243-250)
        ncell = (py - 1) * nx + px;
        const unsigned char sv = st[ncell];
        if (sv & ST_FREE) {
          const double tg = gc + mpj_sqrt((double)(dx * dx) * xf2 + (double)(dy * dy) * yf2);
          double tf = tg;
          if constexpr (!DKA) {
            const int hx = px - gx, hy = py - gy;
            const double th = mpj_sqrt((double)((long long)hx * hx) * xf2 + (double)((long long)hy * hy) * yf2);
            tf = tg + th;
          }
          bool upd = false;
          if (sv & ST_EXIST) {
            upd = DKA ? tf < f[ncell] : tg < g[ncell];
          } else {
            upd = true;
            isnew = true;
          }
          if (upd) {
            g[ncell] = tg;
            if constexpr (!DKA) f[ncell] = tf;
            par[ncell] = (unsigned short)cur;
            app = !(sv & ST_OPEN);  // InOpen (:145-152)
            st[ncell] = sv | ST_EXIST | ST_OPEN;
          }
        }
      }
    }
    const unsigned long long am = __ballot(app), nm = __ballot(isnew);
    if (app) cur_o[n_open + __popcll(am & ((1ull << lane) - 1))] = (unsigned short)ncell;
    n_open += __popcll(am);
    nn += __popcll(nm);
    __syncthreads();
  }
  // astarpath (:109-121) by the parent chain, goal side first into the spare open buffer
  if (lane == 0) {
    int cnt = 0;
    if (found)
      for (int c = last; c != AS_NOPAR && cnt < M; c = par[c]) nxt_o[cnt++] = (unsigned short)c;
    s_cur = cnt;
  }
  __syncthreads();
  const int cnt = s_cur;
  if (A.path)
    for (int i = lane; i < cnt; i += 64) A.path[(size_t)q * M + i] = nxt_o[cnt - 1 - i];
  if (lane == 0) {
    if (A.cost) A.cost[q] = fc;
    if (A.found) A.found[q] = found;
    if (A.pops) A.pops[q] = loop;
    if (A.n_nodes) A.n_nodes[q] = nn;
    if (A.path_n) A.path_n[q] = cnt;
    if (capped) *A.err = 1;
    if (A.path_len) A.path_len[q] = as_path_length(nxt_o, cnt, nx, sx, sy, xf, yf, ge);
  }
}

// FindNewNode's directions (bfs_utils.jl:140)
__device__ const signed char BFS_DX[4] = {-1, 1, 0, 0};
__device__ const signed char BFS_DY[4] = {0, 0, -1, 1};

// planBFS! (bfs_utils.jl:1-59) + FindNewNode (:137-161).  popfirst! on a list that is only ever push!-ed to, and
// haskey keeps a cell from entering twice: queue position i is pop i + 1, and a level (the nodes one hop
// further than the last) is a run of positions [h, tail).  Candidate c = 4*i + d is direction d of the node
// at position i; the sequential loop gives a new cell to the lowest candidate that reaches it, and appends
// the winners in candidate order.
__global__ __launch_bounds__(64) void bfs_search_kernel(AsArgs A) {
  extern __shared__ unsigned int bfs_sm[];
  __shared__ int s_goal, s_cnt;
  const int nx = A.nx, ny = A.ny, N = nx * ny, M = N + 1;
  const int lane = threadIdx.x, q = blockIdx.x;
  unsigned int* claim = bfs_sm;
  unsigned short* par = reinterpret_cast<unsigned short*>(claim + M);
  unsigned short* que = par + M;
  unsigned char* st = reinterpret_cast<unsigned char*>(que + M);
  const double* ge = A.geo + (size_t)q * 4;
  const int sx = A.scell[2 * q], sy = A.scell[2 * q + 1];
  const int gx = A.gcell[2 * q], gy = A.gcell[2 * q + 1];
  const unsigned char* mk = A.mask + (size_t)q * N;
  for (int i = lane; i < M; i += 64) {
    st[i] = (i > 0 && mk[i - 1]) ? ST_FREE : 0;
    claim[i] = 0xFFFFFFFFu;
  }
  __syncthreads();
  // Encode (bfs_utils.jl:123-135); a goal off the grid matches no cell a search can enter
  const int s_enc = (sx < 1 || sx > nx || sy < 1 || sy > ny) ? 0 : (sy - 1) * nx + sx;
  const int g_enc = (gx < 1 || gx > nx || gy < 1 || gy > ny) ? 0 : (gy - 1) * nx + gx;
  if (lane == 0) {  // starting_node (setup.jl:20-21), pushed at :3
    par[s_enc] = AS_NOPAR;
    st[s_enc] |= ST_EXIST;
    que[0] = (unsigned short)s_enc;
    s_goal = (sx == gx && sy == gy) ? 0 : -1;  // (start == goal: found at the first pop -- :25 throws)
  }
  __syncthreads();
  // the neighbour cell of candidate c (0: off the grid) and the cell it is reached from
  auto neighbour = [&](int c, int& cell) {
    cell = que[c >> 2];
    const int cx = cell == 0 ? sx : (cell - 1) % nx + 1, cy = cell == 0 ? sy : (cell - 1) / nx + 1;
    const int px = cx + BFS_DX[c & 3], py = cy + BFS_DY[c & 3];
    return (px >= 1 && px <= nx && py >= 1 && py <= ny) ? (py - 1) * nx + px : 0;  // checkPositionValidity (:169-176)
  };
  int h = 0, tail = 1, found = 0;
  int gpos = s_goal;  // the goal's queue position, known from the moment it is appended
  while (h < tail) {
    const int lvl_end = tail;
    int n_exp = lvl_end - h;
    if (gpos >= 0) {  // the goal is in this level: only the nodes ahead of it were popped before it (:23)
      found = 1;
      n_exp = gpos - h;
    }
    const int c0 = 4 * h, c1 = 4 * (h + n_exp);
    for (int c = c0 + lane; c < c1; c += 64) {
      int cell;
      const int nb = neighbour(c, cell);
      if (nb > 0 && (st[nb] & (ST_FREE | ST_EXIST)) == ST_FREE) atomicMin(&claim[nb], (unsigned int)c);  // (:147,:152)
    }
    __syncthreads();
    // a candidate is unique to its (position, direction), so claim[nb] == c only for this level's winner
    for (int base = c0; base < c1; base += 64) {
      const int c = base + lane;
      int cell = 0, nb = 0;
      bool win = false;
      if (c < c1) {
        nb = neighbour(c, cell);
        win = nb > 0 && claim[nb] == (unsigned int)c;
      }
      const unsigned long long wm = __ballot(win);
      if (win) {  // :153-155
        const int slot = tail + __popcll(wm & ((1ull << lane) - 1));
        par[nb] = (unsigned short)cell;
        st[nb] |= ST_EXIST;
        que[slot] = (unsigned short)nb;
        if (nb == g_enc) s_goal = slot;
      }
      tail += __popcll(wm);
    }
    __syncthreads();
    if (found) break;
    gpos = s_goal;
    h = lvl_end;
  }
  // every queued node is in nodes_collection; the pops are the queue up to the goal, or all of it
  const int pops = found ? gpos + 1 : tail;
  if (A.pop_seq)
    for (int i = lane; i < pops; i += 64) A.pop_seq[(size_t)q * A.cap + i] = que[i];
  // bfspath (:24-35) by the parent chain, goal side first into the claim words (the search is over)
  if (lane == 0) {
    int cnt = 0;
    if (found)
      for (int c = que[gpos]; c != AS_NOPAR && cnt < M; c = par[c]) claim[cnt++] = (unsigned int)c;
    s_cnt = cnt;
  }
  __syncthreads();
  const int cnt = s_cnt;
  if (A.path)
    for (int i = lane; i < cnt; i += 64) A.path[(size_t)q * M + i] = (int)claim[cnt - 1 - i];
  if (lane == 0) {
    if (A.found) A.found[q] = found;
    if (A.pops) A.pops[q] = pops;
    if (A.n_nodes) A.n_nodes[q] = tail;
    if (A.path_n) A.path_n[q] = cnt;
    if (A.path_len) A.path_len[q] = as_path_length(claim, cnt, nx, sx, sy, ge[2], ge[3], ge);
  }
}

// ---------------------------------------------------------------- host
}  // namespace

// defineAstar (setup.jl:15-18): factors and Int(floor(...)) cells; false when a cell is not an int (declared in
// gridsearch.hpp: gridfield.hip converts with the same code)
bool as_factors(const double* b, int nx, int ny, double* ge) {
  ge[0] = b[0];
  ge[1] = b[2];
  ge[2] = (b[1] - b[0]) / ((double)nx - 1);
  ge[3] = (b[3] - b[2]) / ((double)ny - 1);
  return std::isfinite(ge[0]) && std::isfinite(ge[1]) && std::isfinite(ge[2]) && std::isfinite(ge[3]);
}
bool as_cell(const double* ge, const double* real, int* cell) {
  const double cx = std::floor((real[0] - ge[0]) / ge[2] + 1), cy = std::floor((real[1] - ge[1]) / ge[3] + 1);
  if (!(std::fabs(cx) < 1e9) || !(std::fabs(cy) < 1e9)) return false;  // (Julia: InexactError)
  cell[0] = (int)cx;
  cell[1] = (int)cy;
  return true;
}

namespace {

// masks + searches on the context stream (no synchronisation).  obs_dev: [scenes][n_obs][kind] on the device;
// kind MP_GRID_OBS_MASK: the masks are in WS_AS_MASK already.  node_ws: the node workspace of gridbig.hip's
// kernels, which then run the searches (null: the LDS kernels, nx*ny <= AS_MAX_CELLS).
int as_launch(mp_ctx* ctx, int planner, int scenes, int kind, int n_obs, const double* obs_dev, AsArgs A,
              void* node_ws = nullptr) {
  const int N = A.nx * A.ny;
  unsigned char* mask = (unsigned char*)mp_ws(ctx, WS_AS_MASK, (size_t)scenes * N);
  int* err = (int*)mp_ws(ctx, WS_AS_ERR, sizeof(int));
  if (!mask || !err) return MP_ERR_NOMEM;
  MP_HIP(ctx, hipMemsetAsync(err, 0, sizeof(int), ctx->stream));
  const double* wpts = nullptr;
  if (kind == MP_GRID_OBS_MASK) {  // the caller's masks, uploaded by as_plan: nothing to compute
  } else if (n_obs == 0) {  // an empty obstacle list (A* indexes obstacle_list[1]; Dijkstra and BFS loop over 1:0): all free
    MP_HIP(ctx, hipMemsetAsync(mask, 1, (size_t)scenes * N, ctx->stream));
  } else {
    if (kind == 5) {
      double* w = (double*)mp_ws(ctx, WS_AS_WALL, sizeof(double) * 10 * (size_t)scenes * n_obs);
      if (!w) return MP_ERR_NOMEM;
      hipLaunchKernelGGL(as_wall_kernel, dim3((unsigned)((scenes * n_obs + 63) / 64)), dim3(64), 0, ctx->stream,
                         scenes * n_obs, obs_dev, w);
      MP_HIP(ctx, hipGetLastError());
      wpts = w;
    }
    hipLaunchKernelGGL(as_mask_kernel, dim3((unsigned)(((size_t)scenes * N + 255) / 256)), dim3(256), 0, ctx->stream,
                       scenes, A.nx, A.ny, A.geo, kind, n_obs, obs_dev, wpts, mask);
    MP_HIP(ctx, hipGetLastError());
  }
  A.mask = mask;
  A.err = err;
  A.cap = 2 * (N + 1);
  if (node_ws) return gb_launch(ctx, planner, scenes * A.per_scene, node_ws, A);
  const dim3 grid((unsigned)(scenes * A.per_scene));
  if (planner == AS_BFS) {  // 23.4 KB at the largest grid: no attribute to raise
    hipLaunchKernelGGL(bfs_search_kernel, grid, dim3(64), bfs_lds_bytes(N + 1), ctx->stream, A);
  } else if (planner == AS_DKA) {  // (the attribute is per kernel function: each instance has its own flag)
    const size_t lds = as_lds_bytes(N + 1, true);
    if (lds > 48 * 1024 && !ctx->dka_lds_attr) {
      MP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(as_search_kernel<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)as_lds_bytes(AS_MAX_CELLS + 1, true)));
      ctx->dka_lds_attr = true;
    }
    hipLaunchKernelGGL(as_search_kernel<true>, grid, dim3(64), lds, ctx->stream, A);
  } else {
    const size_t lds = as_lds_bytes(N + 1);
    if (lds > 48 * 1024 && !ctx->astar_lds_attr) {
      MP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(as_search_kernel<false>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)as_lds_bytes(AS_MAX_CELLS + 1)));
      ctx->astar_lds_attr = true;
    }
    hipLaunchKernelGGL(as_search_kernel<false>, grid, dim3(64), lds, ctx->stream, A);
  }
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int as_check_err(mp_ctx* ctx) {
  int err = 0;
  MP_HIP(ctx, hipMemcpyAsync(&err, mp_ws(ctx, WS_AS_ERR, sizeof(int)), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (err) return mp_fail(ctx, MP_ERR_NUMERIC, "grid search: a search reached its pop cap (2 * (nx*ny + 1))");
  return MP_OK;
}

// the body of mp_astar_plan / mp_dka_plan / mp_bfs_plan (max_cells = AS_MAX_CELLS) and of mp_grid_plan behind
// their argument checks (final_cost: null for BFS).  obs_kind MP_GRID_OBS_MASK (mp_grid_plan only): obstacles is
// the free-cell mask [B][ny][nx].  Grids above AS_MAX_CELLS, and every grid with force_global, run gridbig.hip's
// kernels.
int as_plan(mp_ctx* ctx, int planner, int B, int nx, int ny, const double* bound, const double* start_real,
            const double* goal_real, int obs_kind, int n_obs, const void* obstacles, double* final_cost, int32_t* found,
            int32_t* pops, int32_t* n_nodes, int32_t* pop_seq, int32_t* path, int32_t* path_n, double* path_length,
            int max_cells = AS_MAX_CELLS, bool force_global = false) {
  MP_CHECK(ctx, nx >= 2 && ny >= 2 && (long long)nx * ny <= max_cells,
           "grid %d x %d: each side must be >= 2 and nx*ny <= %d", nx, ny, max_cells);
  const bool masked = max_cells > AS_MAX_CELLS && obs_kind == MP_GRID_OBS_MASK;  // (the three older calls take lists)
  if (masked) {
    MP_CHECK(ctx, obstacles != nullptr, "the free-cell mask is NULL");
    n_obs = 0;
  } else {
    MP_CHECK(ctx, obs_kind == 3 || obs_kind == 5, "obstacle kind must be 3 (circles) or 5 (blocks)");
    MP_CHECK(ctx, n_obs >= 0 && (n_obs == 0 || obstacles), "bad obstacle list");
  }
  MP_CHECK(ctx, (path != nullptr) == (path_n != nullptr), "the path and path_n go together");
  MP_HIP(ctx, hipSetDevice(ctx->device));
  const int N = nx * ny, M = N + 1, cap = 2 * M;
  const size_t nB = (size_t)B;
  // every workspace before the first copy or launch: the node tables of the global-memory kernels ...
  void* node_ws = nullptr;
  if (N > AS_MAX_CELLS || force_global) {
    node_ws = mp_ws(ctx, WS_GB_NODE, gb_node_bytes(planner, nB, N));
    if (!node_ws) return MP_ERR_NOMEM;
  }
  // ... the masks, and the outputs: [cost B doubles | path_len B doubles | found, pops, n_nodes, path_n B ints
  // each | pop_seq | path]
  char* out = (char*)mp_ws(ctx, WS_AS_TABLE, nB * (16 + 16 + 4 * ((size_t)cap + M)));
  if (!out || !mp_ws(ctx, WS_AS_MASK, nB * N)) return MP_ERR_NOMEM;
  std::vector<double> ge(4 * nB);
  std::vector<int> sc(2 * nB), gc(2 * nB);
  for (int s = 0; s < B; s++) {
    MP_CHECK(ctx, as_factors(bound + 4 * (size_t)s, nx, ny, &ge[4 * s]), "bound %d must be finite", s);
    MP_CHECK(ctx, as_cell(&ge[4 * s], start_real + 2 * (size_t)s, &sc[2 * s]) &&
                      as_cell(&ge[4 * s], goal_real + 2 * (size_t)s, &gc[2 * s]),
             "search %d: a start or goal cell is not an integer", s);
  }
  int st = MP_OK;
  AsArgs A{};
  A.nx = nx;
  A.ny = ny;
  A.per_scene = 1;
  A.geo = mp_upload(ctx, WS_AS_GEO, ge.data(), ge.size(), &st);
  A.gcell = mp_upload(ctx, WS_AS_GCELL, gc.data(), gc.size(), &st);
  A.scell = mp_upload(ctx, WS_AS_SCELL, sc.data(), sc.size(), &st);
  const double* dobs = n_obs ? mp_upload(ctx, WS_AS_OBS, (const double*)obstacles, nB * n_obs * obs_kind, &st) : nullptr;
  if (masked && !mp_upload(ctx, WS_AS_MASK, (const unsigned char*)obstacles, nB * N, &st)) return st ? st : MP_ERR_NOMEM;
  if (st || !A.geo || !A.gcell || !A.scell || (n_obs && !dobs)) return st ? st : MP_ERR_NOMEM;
  double* dcost = (double*)out;
  A.cost = planner == AS_BFS ? nullptr : dcost;
  A.path_len = dcost + nB;
  A.found = (int*)(A.path_len + nB);
  A.pops = A.found + nB;
  A.n_nodes = A.pops + nB;
  A.path_n = A.n_nodes + nB;
  int* dseq = A.path_n + nB;
  int* dpath = dseq + nB * cap;
  A.pop_seq = pop_seq ? dseq : nullptr;
  A.path = path ? dpath : nullptr;
  if (pop_seq) MP_HIP(ctx, hipMemsetAsync(dseq, 0xff, sizeof(int) * nB * cap, ctx->stream));  // -1 past the pops
  if (path) MP_HIP(ctx, hipMemsetAsync(dpath, 0xff, sizeof(int) * nB * M, ctx->stream));
  if ((st = as_launch(ctx, planner, B, obs_kind, n_obs, dobs, A, node_ws))) return st;
  if ((st = mp_download(ctx, final_cost, (const double*)A.cost, nB))) return st;
  if ((st = mp_download(ctx, path_length, (const double*)A.path_len, nB))) return st;
  if ((st = mp_download(ctx, found, (const int32_t*)A.found, nB))) return st;
  if ((st = mp_download(ctx, pops, (const int32_t*)A.pops, nB))) return st;
  if ((st = mp_download(ctx, n_nodes, (const int32_t*)A.n_nodes, nB))) return st;
  if ((st = mp_download(ctx, path_n, (const int32_t*)A.path_n, nB))) return st;
  if ((st = mp_download(ctx, pop_seq, (const int32_t*)dseq, nB * cap))) return st;
  if ((st = mp_download(ctx, path, (const int32_t*)dpath, nB * M))) return st;
  return as_check_err(ctx);
}

}  // namespace

// astar_heuristic's table for B Hybrid A* scenes, enqueued on the context stream: goal on the host, walls
// on the device; *table_dev = [B][121] (valid once the stream reaches this point).  mp_as_table_status
// reports a pop cap afterwards (it synchronises).
int mp_as_table_dev(mp_ctx* ctx, const mp_ha_params* p, int B, const double* goal, const double* walls_dev,
                    const double** table_dev) {
  constexpr int N = AS_HA_N * AS_HA_N;
  std::vector<double>& ge = ctx->as_geo_host;  // (kept by the context: the uploads below are asynchronous)
  std::vector<int>& gc = ctx->as_gcell_host;
  ge.resize(4 * (size_t)B);
  gc.resize(2 * (size_t)B);
  const double b[4] = {p->stbound[0], p->stbound[1], p->stbound[2], p->stbound[3]};
  for (int s = 0; s < B; s++) {
    MP_CHECK(ctx, as_factors(b, AS_HA_N, AS_HA_N, &ge[4 * s]), "stbound must be finite");
    MP_CHECK(ctx, as_cell(&ge[4 * s], goal + 3 * (size_t)s, &gc[2 * s]), "goal %d: the grid cell is not an integer", s);
  }
  int st = MP_OK;
  AsArgs A{};
  A.nx = A.ny = AS_HA_N;
  A.per_scene = N;
  A.geo = mp_upload(ctx, WS_AS_GEO, ge.data(), ge.size(), &st);
  A.gcell = mp_upload(ctx, WS_AS_GCELL, gc.data(), gc.size(), &st);
  double* tab = (double*)mp_ws(ctx, WS_AS_TABLE, sizeof(double) * N * (size_t)B);
  if (st || !A.geo || !A.gcell || !tab) return st ? st : MP_ERR_NOMEM;
  A.cost = tab;
  if ((st = as_launch(ctx, AS_ASTAR, B, 5, p->n_walls, walls_dev, A))) return st;
  *table_dev = tab;
  return MP_OK;
}
int mp_as_table_status(mp_ctx* ctx) { return as_check_err(ctx); }

extern "C" {

int mp_astar_plan(mp_ctx* ctx, int32_t B, int32_t nx, int32_t ny, const double* bound, const double* start_real,
                  const double* goal_real, int32_t obs_kind, int32_t n_obs, const double* obstacles,
                  double* final_cost, int32_t* found, int32_t* pops, int32_t* n_nodes, int32_t* pop_seq,
                  int32_t* astarpath, int32_t* path_n, double* path_length) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, B >= 1 && bound && start_real && goal_real && final_cost && found && pops && n_nodes, "bad arguments");
  return as_plan(ctx, AS_ASTAR, B, nx, ny, bound, start_real, goal_real, obs_kind, n_obs, obstacles, final_cost, found,
                 pops, n_nodes, pop_seq, astarpath, path_n, path_length);
}

int mp_dka_plan(mp_ctx* ctx, int32_t B, int32_t nx, int32_t ny, const double* bound, const double* start_real,
                const double* goal_real, int32_t n_obs, const double* circles, double* final_cost, int32_t* found,
                int32_t* pops, int32_t* n_nodes, int32_t* pop_seq, int32_t* path, int32_t* path_n, double* path_length) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, B >= 1 && bound && start_real && goal_real && final_cost && found && pops && n_nodes, "bad arguments");
  return as_plan(ctx, AS_DKA, B, nx, ny, bound, start_real, goal_real, 3, n_obs, circles, final_cost, found, pops,
                 n_nodes, pop_seq, path, path_n, path_length);
}

int mp_bfs_plan(mp_ctx* ctx, int32_t B, int32_t nx, int32_t ny, const double* bound, const double* start_real,
                const double* goal_real, int32_t n_obs, const double* circles, int32_t* found, int32_t* pops,
                int32_t* n_nodes, int32_t* pop_seq, int32_t* path, int32_t* path_n, double* path_length) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, B >= 1 && bound && start_real && goal_real && found && pops && n_nodes, "bad arguments");
  return as_plan(ctx, AS_BFS, B, nx, ny, bound, start_real, goal_real, 3, n_obs, circles, nullptr, found, pops, n_nodes,
                 pop_seq, path, path_n, path_length);
}

int mp_grid_plan(mp_ctx* ctx, int32_t planner, int32_t flags, int32_t B, int32_t nx, int32_t ny, const double* bound,
                 const double* start_real, const double* goal_real, int32_t obs_kind, int32_t n_obs,
                 const void* obstacles, double* final_cost, int32_t* found, int32_t* pops, int32_t* n_nodes,
                 int32_t* pop_seq, int32_t* path, int32_t* path_n, double* path_length) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, planner == MP_GRID_ASTAR || planner == MP_GRID_DKA || planner == MP_GRID_BFS,
           "planner must be MP_GRID_ASTAR, MP_GRID_DKA or MP_GRID_BFS");
  MP_CHECK(ctx, (flags & ~MP_GRID_FORCE_GLOBAL) == 0, "unknown flags");
  MP_CHECK(ctx, B >= 1 && bound && start_real && goal_real && (final_cost || planner == MP_GRID_BFS) && found && pops &&
                    n_nodes,
           "bad arguments");
  MP_CHECK(ctx, obs_kind == 3 || obs_kind == 5 || obs_kind == MP_GRID_OBS_MASK,
           "obstacle kind must be 3 (circles), 5 (blocks) or MP_GRID_OBS_MASK");
  MP_CHECK(ctx, obs_kind != 5 || planner == MP_GRID_ASTAR, "blocks are obstacles of A* only: Dijkstra and BFS take circles");
  static_assert(MP_GRID_ASTAR == AS_ASTAR && MP_GRID_DKA == AS_DKA && MP_GRID_BFS == AS_BFS, "planner codes");
  return as_plan(ctx, planner, B, nx, ny, bound, start_real, goal_real, obs_kind, n_obs, obstacles,
                 planner == MP_GRID_BFS ? nullptr : final_cost, found, pops, n_nodes, pop_seq, path, path_n, path_length,
                 MP_GRID_MAX_CELLS, (flags & MP_GRID_FORCE_GLOBAL) != 0);
}

// the masks as_launch builds for a planner call with the same bound and obstacle list, copied out
int mp_grid_rasterize(mp_ctx* ctx, int32_t B, int32_t nx, int32_t ny, const double* bound, int32_t obs_kind,
                      int32_t n_obs, const double* obstacles, uint8_t* mask) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, nx >= 2 && ny >= 2 && (long long)nx * ny <= MP_GRID_MAX_CELLS,
           "grid %d x %d: each side must be >= 2 and nx*ny <= %d", nx, ny, MP_GRID_MAX_CELLS);
  MP_CHECK(ctx, B >= 1 && (long long)B * nx * ny <= MP_MAP_MAX_BATCH_CELLS, "B = %d maps: B >= 1 and B*nx*ny <= %d", B,
           MP_MAP_MAX_BATCH_CELLS);
  MP_CHECK(ctx, bound && mask, "bound or mask is NULL");
  MP_CHECK(ctx, obs_kind == 3 || obs_kind == 5, "obstacle kind must be 3 (circles) or 5 (blocks)");
  MP_CHECK(ctx, n_obs >= 0 && (n_obs == 0 || obstacles) && (long long)B * n_obs <= (1 << 28), "bad obstacle list");
  const int N = nx * ny;
  const size_t nB = (size_t)B;
  std::vector<double> ge(4 * nB);
  for (int s = 0; s < B; s++)
    MP_CHECK(ctx, as_factors(bound + 4 * (size_t)s, nx, ny, &ge[4 * s]), "bound %d must be finite", s);
  MP_HIP(ctx, hipSetDevice(ctx->device));
  // every workspace before the first copy or launch
  unsigned char* dmask = (unsigned char*)mp_ws(ctx, WS_AS_MASK, nB * N);
  if (!dmask || !mp_ws(ctx, WS_AS_GEO, sizeof(double) * 4 * nB)) return MP_ERR_NOMEM;
  if (n_obs && (!mp_ws(ctx, WS_AS_OBS, sizeof(double) * nB * n_obs * obs_kind) ||
                (obs_kind == 5 && !mp_ws(ctx, WS_AS_WALL, sizeof(double) * 10 * nB * n_obs))))
    return MP_ERR_NOMEM;
  if (n_obs == 0) {
    MP_HIP(ctx, hipMemsetAsync(dmask, 1, nB * N, ctx->stream));
  } else {
    int st = MP_OK;
    const double* geo = mp_upload(ctx, WS_AS_GEO, ge.data(), ge.size(), &st);
    const double* dobs = mp_upload(ctx, WS_AS_OBS, obstacles, nB * n_obs * obs_kind, &st);
    if (st || !geo || !dobs) return st ? st : MP_ERR_NOMEM;
    double* wpts = nullptr;
    if (obs_kind == 5) {
      wpts = (double*)mp_ws(ctx, WS_AS_WALL, sizeof(double) * 10 * nB * n_obs);
      hipLaunchKernelGGL(as_wall_kernel, dim3((unsigned)((B * n_obs + 63) / 64)), dim3(64), 0, ctx->stream, B * n_obs, dobs,
                         wpts);
      MP_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(as_mask_kernel, dim3((unsigned)((nB * N + 255) / 256)), dim3(256), 0, ctx->stream, B, nx, ny, geo,
                       obs_kind, n_obs, dobs, wpts, dmask);
    MP_HIP(ctx, hipGetLastError());
  }
  int st = mp_download(ctx, mask, (const uint8_t*)dmask, nB * N);
  if (st) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (ge outlives its upload)
  return MP_OK;
}

int mp_ha_astar_table(mp_ctx* ctx, const mp_ha_params* p, int32_t B, const double* goal, const double* walls,
                      double* table) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, p != nullptr, "params is NULL");
  MP_CHECK(ctx, B >= 1 && goal && table && p->n_walls >= 0 && (walls || p->n_walls == 0), "bad arguments");
  MP_HIP(ctx, hipSetDevice(ctx->device));
  int st = MP_OK;
  const double* dw = p->n_walls ? mp_upload(ctx, WS_AS_OBS, walls, 5 * (size_t)p->n_walls * B, &st) : nullptr;
  if (st || (p->n_walls && !dw)) return st ? st : MP_ERR_NOMEM;
  const double* tab = nullptr;
  if ((st = mp_as_table_dev(ctx, p, B, goal, dw, &tab))) return st;
  if ((st = mp_download(ctx, table, tab, (size_t)AS_HA_N * AS_HA_N * B))) return st;
  return as_check_err(ctx);
}

}  // extern "C"
