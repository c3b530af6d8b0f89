// gridbig.hip — the grid planners of astar.hip for grids beyond one block's LDS (mp_grid_plan above 51 x 51
// cells, or with MP_GRID_FORCE_GLOBAL): one workgroup of four wavefronts per search, the node tables in a global
// workspace, int32 cell indices.  Masks, walls and geometry come from astar.hip's kernels; every output is what
// as_search_kernel / bfs_search_kernel write.
//
// gb_search_kernel  planAstar! / planDKA! (<true>).  The reference stable-sorts the open list by f every
//                   iteration; the same pop order results from taking the open entry with the smallest
//                   (f, number), numbers handed out once an iteration's direction loop has run: first to the
//                   open nodes whose f strictly decreased, in the order of their old (f, number), then to the
//                   nodes appended, in direction order; an update that leaves f equal keeps its number
//                   (tests/gridkey_ref.py).  So the open list is an unordered array of
//                   16-byte records with a slot index per cell: a strided scan by all lanes and a wave / block
//                   min take the head, swap-remove pops it, a decrease is written in place.
// gb_bfs_kernel     planBFS!, bfs_search_kernel's level-at-a-time scheme with the claim words, the parents and
//                   the queue in global memory.
//
// Every loop is bounded (the pop cap, the queue length); no workgroup waits for another.  Writes of one phase
// are read in the next across a __syncthreads (a workgroup's waves share their CU's vector L1).
#define MPJ_LANE_SAFE 1
#include "gridsearch.hpp"

namespace {

constexpr int GB_THREADS = 256, GB_WAVES = GB_THREADS / 64;
struct __align__(16) GbRec {
  double f;
  unsigned int seq;
  int cell;
};
// slot[cell] (A*, Dijkstra) >= 0: the cell's record in the open list; par[cell] (BFS) >= 0: the parent
enum : int { GB_NOPAR = -1, GB_CLOSED = -1, GB_FREE = -2, GB_BLOCKED = -3 };

// FindNewNode's directions (astar.hip's AS_DX / AS_DY, BFS_DX / BFS_DY)
__device__ const signed char GB_DX[9] = {-1, -1, -1, 1, 1, 1, 0, 1, 0};
__device__ const signed char GB_DY[9] = {0, -1, -1, -1, 0, 1, -1, -1, 1};
__device__ const signed char GB_BDX[4] = {-1, 1, 0, 0};
__device__ const signed char GB_BDY[4] = {0, 0, -1, 1};

// (fa, sa) sorts ahead of (fb, sb): isless on f, as the reference's sort, then the number
__device__ __forceinline__ bool gb_before(double fa, unsigned int sa, double fb, unsigned int sb) {
  return mpj_isless(fa, fb) | (!mpj_isless(fb, fa) & (sa < sb));
}

template <bool DKA>
__global__ __launch_bounds__(GB_THREADS) void gb_search_kernel(AsArgs A, GbRec* __restrict__ recs_all,
                                                               double* __restrict__ g_all, int* __restrict__ par_all,
                                                               int* __restrict__ slot_all) {
  __shared__ double s_f[GB_WAVES];
  __shared__ unsigned int s_seq[GB_WAVES];
  __shared__ int s_idx[GB_WAVES], s_cell[GB_WAVES];
  __shared__ int s_nopen, s_cnt;
  const int nx = A.nx, ny = A.ny, N = nx * ny, M = N + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x, scene = q / A.per_scene;
  const size_t base = (size_t)q * M;
  GbRec* recs = recs_all + base;  // the open list, unordered
  double* g = g_all + base;       // (Dijkstra: f)
  int* par = par_all + base;
  int* slot = slot_all + base;
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
  for (int i = tid; i < M; i += GB_THREADS) slot[i] = (i > 0 && mk[i - 1]) ? GB_FREE : GB_BLOCKED;
  __syncthreads();
  // Encode (astar_utils.jl:176-188)
  const int s_enc = (sx < 1 || sx > nx || sy < 1 || sy > ny) ? 0 : (sy - 1) * nx + sx;
  if (tid == 0) {  // starting_node (setup.jl:19,22).  Its g = 0 is never undercut, so a start on a blocked cell
    g[s_enc] = 0.0;  // (or off the grid) stays closed once popped, as without ST_FREE in as_search_kernel
    par[s_enc] = GB_NOPAR;
    slot[s_enc] = 0;
    recs[0] = GbRec{0.0, 0u, s_enc};
  }
  __syncthreads();
  int n_open = 1, nn = 1, loop = 0, found = 0, capped = 0, last = -1;
  unsigned int counter = 1;  // the next number; at most 7 per pop
  int* pseq = A.pop_seq ? A.pop_seq + (size_t)q * A.cap : nullptr;
  while (n_open > 0) {
    if (loop >= A.cap) {
      capped = 1;
      break;
    }
    loop++;
    // sort!(open_list) + popfirst!: the entry with the smallest (f, number)
    double bf = 0.0;
    unsigned int bs = 0;
    int bi = -1, bc = 0;
    for (int i = tid; i < n_open; i += GB_THREADS) {
      const GbRec r = recs[i];
      if (bi < 0 || gb_before(r.f, r.seq, bf, bs)) {
        bf = r.f;
        bs = r.seq;
        bi = i;
        bc = r.cell;
      }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const double of = __shfl_xor(bf, off);
      const unsigned int os = __shfl_xor(bs, off);
      const int oi = __shfl_xor(bi, off), oc = __shfl_xor(bc, off);
      if (oi >= 0 && (bi < 0 || gb_before(of, os, bf, bs))) {
        bf = of;
        bs = os;
        bi = oi;
        bc = oc;
      }
    }
    if (lane == 0) {
      s_f[wave] = bf;
      s_seq[wave] = bs;
      s_idx[wave] = bi;
      s_cell[wave] = bc;
    }
    __syncthreads();
    bf = s_f[0];
    bs = s_seq[0];
    bi = s_idx[0];
    bc = s_cell[0];
#pragma unroll
    for (int w = 1; w < GB_WAVES; w++) {
      const int oi = s_idx[w];
      if (oi >= 0 && (bi < 0 || gb_before(s_f[w], s_seq[w], bf, bs))) {
        bf = s_f[w];
        bs = s_seq[w];
        bi = oi;
        bc = s_cell[w];
      }
    }
    const int idx = bi, cur = bc;
    const int cx = cur == 0 ? sx : (cur - 1) % nx + 1, cy = cur == 0 ? sy : (cur - 1) / nx + 1;
    if (tid == 0 && pseq) pseq[loop - 1] = cur;
    if (cx == gx && cy == gy) {  // :107-108 (start == goal: cost 0, found -- the reference throws at :110)
      found = 1;
      last = cur;
      break;
    }
    if (wave == 0) {
      // FindNewNode (:190-235): the seven distinct directions touch seven distinct cells, one lane each.  Every
      // load of the iteration comes before its stores, and no two lanes store to one address: the record that
      // swap-remove moves (the list's last, into the popped slot) is written by the lane that updates it, if any
      const int n1 = n_open - 1;
      const GbRec tail = recs[n1];
      const double gc = g[cur];
      bool upd = false, app = false, isnew = false, dec = false, inopen = false;
      int ncell = 0, sv = GB_BLOCKED;
      double tg = 0.0, tf = 0.0, of = 0.0;
      unsigned int os = 0;
      if (lane < 9 && lane != 2 && lane != 7) {
        const int dx = GB_DX[lane], dy = GB_DY[lane];
        const int px = cx + dx, py = cy + dy;
        if (px >= 1 && px <= nx && py >= 1 && py <= ny) {  // checkPositionValidity (:243-250)
          ncell = (py - 1) * nx + px;
          sv = slot[ncell];
          if (sv != GB_BLOCKED) {
            tg = gc + mpj_sqrt((double)(dx * dx) * xf2 + (double)(dy * dy) * yf2);
            tf = tg;
            if constexpr (!DKA) {
              const int hx = px - gx, hy = py - gy;
              const double th = mpj_sqrt((double)((long long)hx * hx) * xf2 + (double)((long long)hy * hy) * yf2);
              tf = tg + th;
            }
            if (sv == GB_FREE) {
              upd = app = isnew = true;
            } else if (tg < g[ncell]) {  // (Dijkstra: tf < f, dka_utils.jl:193)
              upd = true;
              if (sv == GB_CLOSED) {
                app = true;  // InOpen (:145-152): a closed node is pushed again
              } else {
                inopen = true;
                if (sv == n1) {
                  of = tail.f;
                  os = tail.seq;
                } else {
                  const GbRec r = recs[sv];
                  of = r.f;
                  os = r.seq;
                }
                dec = tf < of;
              }
            }
          }
        }
      }
      const unsigned long long dm = __ballot(dec), am = __ballot(app), nm = __ballot(isnew);
      const int ndec = __popcll(dm), napp = __popcll(am);
      int rank = 0;  // among this iteration's decreases, by the old (f, number)
      if (ndec >= 2) {
        for (int l = 0; l < 9; l++) {
          const double lf = __shfl(of, l);
          const unsigned int ls = __shfl(os, l);
          if (((dm >> l) & 1) && l != lane && gb_before(lf, ls, of, os)) rank++;
        }
      }
      const int apos = n1 + __popcll(am & ((1ull << lane) - 1));  // push! order is direction order
      unsigned int nseq = os;
      if (dec) nseq = counter + (unsigned int)rank;
      if (app) nseq = counter + (unsigned int)(ndec + apos - n1);
      counter += (unsigned int)(ndec + napp);
      const bool moved = inopen && sv == n1 && idx != n1;
      const bool any_moved = __ballot(moved) != 0;
      if (upd) {
        g[ncell] = tg;
        par[ncell] = cur;
        if (app) {
          recs[apos] = GbRec{tf, nseq, ncell};
          slot[ncell] = apos;
        } else {
          if (dec || moved) recs[moved ? idx : sv] = GbRec{dec ? tf : of, nseq, ncell};
          if (moved) slot[ncell] = idx;
        }
      }
      if (lane == 0) {
        slot[cur] = GB_CLOSED;
        if (idx != n1 && !any_moved) {
          recs[idx] = tail;
          slot[tail.cell] = idx;
        }
        s_nopen = n1 + napp;
      }
      nn += __popcll(nm);
    }
    __syncthreads();
    n_open = s_nopen;
  }
  // astarpath (:109-121) by the parent chain, goal side first into the record array (the search is over)
  int* rev = reinterpret_cast<int*>(recs);
  double fc = 0.0;
  if (tid == 0) {
    int cnt = 0;
    if (found) {
      fc = g[last];
      for (int c = last; c != GB_NOPAR && cnt < M; c = par[c]) rev[cnt++] = c;
    }
    s_cnt = cnt;
  }
  __syncthreads();
  const int cnt = s_cnt;
  if (A.path)
    for (int i = tid; i < cnt; i += GB_THREADS) A.path[(size_t)q * M + i] = rev[cnt - 1 - i];
  if (tid == 0) {
    if (A.cost) A.cost[q] = fc;
    if (A.found) A.found[q] = found;
    if (A.pops) A.pops[q] = loop;
    if (A.n_nodes) A.n_nodes[q] = nn;
    if (A.path_n) A.path_n[q] = cnt;
    if (capped) *A.err = 1;
    if (A.path_len) A.path_len[q] = as_path_length(rev, cnt, nx, sx, sy, xf, yf, ge);
  }
}

// planBFS! as bfs_search_kernel runs it: queue position i is pop i + 1, a level is a run of positions, candidate
// c = 4*i + d (< 2^24 + 4) is direction d of the node at position i; a new cell goes to the lowest candidate
// that reaches it (atomicMin on its claim word) and the winners are appended in candidate order.
__global__ __launch_bounds__(GB_THREADS) void gb_bfs_kernel(AsArgs A, unsigned int* __restrict__ claim_all,
                                                            int* __restrict__ par_all, int* __restrict__ que_all) {
  __shared__ int s_goal, s_cnt, s_wcnt[GB_WAVES];
  const int nx = A.nx, ny = A.ny, N = nx * ny, M = N + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
  const size_t base = (size_t)q * M;
  unsigned int* claim = claim_all + base;
  int* par = par_all + base;  // GB_FREE: a free cell not yet in nodes_collection
  int* que = que_all + base;
  const double* ge = A.geo + (size_t)q * 4;
  const int sx = A.scell[2 * q], sy = A.scell[2 * q + 1];
  const int gx = A.gcell[2 * q], gy = A.gcell[2 * q + 1];
  const unsigned char* mk = A.mask + (size_t)q * N;
  for (int i = tid; i < M; i += GB_THREADS) {
    par[i] = (i > 0 && mk[i - 1]) ? GB_FREE : GB_BLOCKED;
    claim[i] = 0xFFFFFFFFu;
  }
  __syncthreads();
  // Encode (bfs_utils.jl:123-135); a goal off the grid matches no cell a search can enter
  const int s_enc = (sx < 1 || sx > nx || sy < 1 || sy > ny) ? 0 : (sy - 1) * nx + sx;
  const int g_enc = (gx < 1 || gx > nx || gy < 1 || gy > ny) ? 0 : (gy - 1) * nx + gx;
  if (tid == 0) {  // starting_node (setup.jl:20-21), pushed at :3
    par[s_enc] = GB_NOPAR;
    que[0] = s_enc;
    s_goal = (sx == gx && sy == gy) ? 0 : -1;  // (start == goal: found at the first pop -- :25 throws)
  }
  __syncthreads();
  // the neighbour cell of candidate c (0: off the grid) and the cell it is reached from
  auto neighbour = [&](int c, int& cell) {
    cell = que[c >> 2];
    const int cx = cell == 0 ? sx : (cell - 1) % nx + 1, cy = cell == 0 ? sy : (cell - 1) / nx + 1;
    const int px = cx + GB_BDX[c & 3], py = cy + GB_BDY[c & 3];
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
    for (int c = c0 + tid; c < c1; c += GB_THREADS) {
      int cell;
      const int nb = neighbour(c, cell);
      if (nb > 0 && par[nb] == GB_FREE) atomicMin(&claim[nb], (unsigned int)c);  // (:147,:152)
    }
    __syncthreads();
    // a candidate is unique to its (position, direction), so claim[nb] == c only for this level's winner
    for (int cb = c0; cb < c1; cb += GB_THREADS) {
      const int c = cb + tid;
      int cell = 0, nb = 0;
      bool win = false;
      if (c < c1) {
        nb = neighbour(c, cell);
        win = nb > 0 && claim[nb] == (unsigned int)c;
      }
      const unsigned long long wm = __ballot(win);
      if (lane == 0) s_wcnt[wave] = __popcll(wm);
      __syncthreads();
      int ahead = 0, all = 0;
#pragma unroll
      for (int w = 0; w < GB_WAVES; w++) {
        const int n = s_wcnt[w];
        if (w < wave) ahead += n;
        all += n;
      }
      if (win) {  // :153-155
        const int pos = tail + ahead + __popcll(wm & ((1ull << lane) - 1));
        par[nb] = cell;
        que[pos] = nb;
        if (nb == g_enc) s_goal = pos;
      }
      tail += all;
      __syncthreads();
    }
    if (found) break;
    gpos = s_goal;
    h = lvl_end;
  }
  // every queued node is in nodes_collection; the pops are the queue up to the goal, or all of it
  const int pops = found ? gpos + 1 : tail;
  if (A.pop_seq)
    for (int i = tid; i < pops; i += GB_THREADS) A.pop_seq[(size_t)q * A.cap + i] = que[i];
  // bfspath (:24-35) by the parent chain, goal side first into the claim words (the search is over)
  if (tid == 0) {
    int cnt = 0;
    if (found)
      for (int c = que[gpos]; c != GB_NOPAR && cnt < M; c = par[c]) claim[cnt++] = (unsigned int)c;
    s_cnt = cnt;
  }
  __syncthreads();
  const int cnt = s_cnt;
  if (A.path)
    for (int i = tid; i < cnt; i += GB_THREADS) A.path[(size_t)q * M + i] = (int)claim[cnt - 1 - i];
  if (tid == 0) {
    if (A.found) A.found[q] = found;
    if (A.pops) A.pops[q] = pops;
    if (A.n_nodes) A.n_nodes[q] = tail;
    if (A.path_n) A.path_n[q] = cnt;
    if (A.path_len) A.path_len[q] = as_path_length(claim, cnt, nx, sx, sy, ge[2], ge[3], ge);
  }
}

}  // namespace

// A*, Dijkstra: records (16 B) | g (8 B) | parent | slot per cell; BFS: claim | parent | queue
size_t gb_node_bytes(int planner, size_t searches, int N) {
  return searches * ((size_t)N + 1) * (planner == AS_BFS ? 12 : 32);
}

int gb_launch(mp_ctx* ctx, int planner, int searches, void* node_ws, const AsArgs& A) {
  const size_t n = (size_t)searches * ((size_t)A.nx * A.ny + 1);
  const dim3 grid((unsigned)searches), block(GB_THREADS);
  if (planner == AS_BFS) {
    unsigned int* claim = (unsigned int*)node_ws;
    int* par = (int*)(claim + n);
    hipLaunchKernelGGL(gb_bfs_kernel, grid, block, 0, ctx->stream, A, claim, par, par + n);
  } else {
    GbRec* recs = (GbRec*)node_ws;
    double* g = (double*)(recs + n);
    int* par = (int*)(g + n);
    if (planner == AS_DKA)
      hipLaunchKernelGGL(gb_search_kernel<true>, grid, block, 0, ctx->stream, A, recs, g, par, par + n);
    else
      hipLaunchKernelGGL(gb_search_kernel<false>, grid, block, 0, ctx->stream, A, recs, g, par, par + n);
  }
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}
