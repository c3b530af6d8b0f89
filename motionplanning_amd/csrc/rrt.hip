// rrt.hip — the sampling planner for gfx950 (PathPlanning/RRT/src/{rrt_utils,setup,types}.jl: planRRT!, RRT
// and RRT*) + C-ABI: mp_rrt_plan (B independent trees in one launch).
//
// rrt_plan_kernel  the whole planRRT! loop (rrt_utils.jl:341-412) of one scene per workgroup, no host round
//                  trip per iteration.  The tree (x, y, cost, parent, first-child / sibling links, the
//                  propagation queue) is SoA in the context workspace; LDS holds the reductions, the
//                  in-disk candidates, the near set and the rewire list.  Every value that steers the
//                  control flow (sample, nearest node, steer, collision, counts) is computed or read
//                  identically by all lanes, so the loop needs no broadcasts; the lanes split the
//                  snapshot scans, the near set and the cost propagation.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#define MPJ_LANE_SAFE 1
#include "../../include/mp_jlmath.h"
#include "runtime.hpp"

namespace {

constexpr int RRT_T = 512;          // threads per workgroup (8 wavefronts)
constexpr int RRT_W = RRT_T / 64;
constexpr int RRT_NEAR = 100;       // planRRT!'s cap on the near set (:375-377)
constexpr int RRT_WAYS = 7;         // thresholds per counting scan of that search
constexpr int RRT_SET = 512;        // in-disk candidates LDS holds; beyond it the 100 nearest are searched for

struct RrtArgs {
  int n_iter, buffer_size, rrt_star, n_obs;
  double bias_rate, grow_min, grow_max, tol;
  const double *bound, *start, *goal, *obs, *uni;  // [B][4], [B][2], [B][2], [B][n_obs][3], [B][n_iter][3]
  const int* obs_count;                            // [B] or null
  // tree state, [B][n_iter + 1] each; links are 0-based node slots (-1: none), parent is 1-based (-1: root)
  double *x, *y, *cost;
  int *parent, *child, *next, *prev;
  unsigned long long* queue;  // cost propagation: (rewire slot << 32) | node slot
  int *n_nodes, *status, *best_idx, *path_n, *counters, *path_idx, *err;
  double* best_cost;
};

// round(v, digits = 2): Base's _round_digits with RoundNearest
__device__ __forceinline__ double rrt_round2(double v) { return __builtin_rint(v * 100.0) / 100.0; }
// Base.sign: +-1, and x itself (+-0, NaN) otherwise
__device__ __forceinline__ double rrt_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : x); }

// ProjectionStates (:112-134) of (bx, by) seen from (ax, ay)
struct RrtProj {
  double p1, p2;
};
__device__ __forceinline__ RrtProj rrt_proj(double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay;
  const double nrm = mpj_sqrt(dx * dx + dy * dy);
  double rho = 0.0, dpsi = 0.0;
  if (nrm >= 0.001) {
    rho = nrm;
    const double ux = dx / nrm, uy = dy / nrm;
    dpsi = mpj_atan(uy / mpj_fabs(ux)) * rrt_sign(ux);  // sign(0.0) = 0: a vertical segment has dpsi = 0
  }
  return {rrt_round2(rho * mpj_cos(dpsi)), rrt_round2(rho * mpj_sin(dpsi))};
}

// neural_cost (:101-106)
__device__ __forceinline__ double rrt_ncost(double p1, double p2) { return 5.0 * mpj_sqrt(p1 * p1 + p2 * p2); }

__device__ __forceinline__ bool rrt_oob(double x, double y, double b0, double b1, double b2, double b3) {
  return x < b0 || x > b1 || y < b2 || y > b3;  // CheckWithinBoundary (:274-280)
}
// both end points of the segment against circle o (:302-308)
__device__ __forceinline__ bool rrt_hit(const double* __restrict__ o, double x1, double y1, double x2, double y2) {
  const double ox = o[0], oy = o[1], rr = o[2] * o[2];
  const double e1 = x1 - ox, f1 = y1 - oy, e2 = x2 - ox, f2 = y2 - oy;
  return (e1 * e1 + f1 * f1 <= rr) || (e2 * e2 + f2 * f2 <= rr);
}

__device__ __forceinline__ bool rrt_less(double d, int i, double od, int oi) { return d < od || (d == od && i < oi); }

// (d, i) -> the block's minimum by (d, then i), in every thread
__device__ __forceinline__ void rrt_block_argmin(double& d, int& i, double* sd, int* si) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const double od = __shfl_xor(d, off);
    const int oi = __shfl_xor(i, off);
    if (rrt_less(od, oi, d, i)) {
      d = od;
      i = oi;
    }
  }
  __syncthreads();  // the previous reduction's readers are done with sd / si
  if ((threadIdx.x & 63) == 0) {
    sd[threadIdx.x >> 6] = d;
    si[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  d = sd[0];
  i = si[0];
#pragma unroll
  for (int w = 1; w < RRT_W; w++)
    if (rrt_less(sd[w], si[w], d, i)) {
      d = sd[w];
      i = si[w];
    }
}

// cn[j] = the number of snapshot nodes whose key (bit pattern of the distance to (nx, ny), index) is at most
// (tk[j], ti[j]), in every thread
__device__ __forceinline__ void rrt_count_le(const double* X, const double* Y, int n_tree, double nx, double ny,
                                             const long long* tk, const int* ti, int* cn, int (*s_cw)[RRT_WAYS]) {
#pragma unroll
  for (int j = 0; j < RRT_WAYS; j++) cn[j] = 0;
  for (int i = threadIdx.x; i < n_tree; i += RRT_T) {
    const double ex = X[i] - nx, ey = Y[i] - ny;
    const long long kb = (long long)__double_as_longlong(mpj_sqrt(ex * ex + ey * ey));
#pragma unroll
    for (int j = 0; j < RRT_WAYS; j++) cn[j] += (kb < tk[j]) || (kb == tk[j] && i <= ti[j]);
  }
#pragma unroll
  for (int j = 0; j < RRT_WAYS; j++)
    for (int off = 32; off; off >>= 1) cn[j] += __shfl_xor(cn[j], off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < RRT_WAYS; j++) s_cw[threadIdx.x >> 6][j] = cn[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RRT_WAYS; j++) {
    int t = 0;
    for (int w = 0; w < RRT_W; w++) t += s_cw[w][j];
    cn[j] = t;
  }
}

__global__ __launch_bounds__(RRT_T) void rrt_plan_kernel(RrtArgs A) {
  __shared__ double s_rd[RRT_W];
  __shared__ int s_ri[RRT_W];
  __shared__ double s_nd[RRT_SET];   // in-disk candidates: distance, node slot
  __shared__ int s_ni[RRT_SET];
  __shared__ int s_near[RRT_NEAR];   // the near set
  __shared__ int s_rwi[RRT_NEAR];    // rewired nodes and their cost changes
  __shared__ double s_rwd[RRT_NEAR];
  __shared__ int s_cw[RRT_W][RRT_WAYS];  // per-wave counts of the search beyond RRT_SET
  __shared__ int s_cnt, s_sel, s_rw, s_tail;

  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int cap = A.n_iter + 1;
  const size_t base = (size_t)b * cap;
  double* X = A.x + base;
  double* Y = A.y + base;
  double* C = A.cost + base;
  int* par = A.parent + base;
  int* chd = A.child + base;
  int* nxt = A.next + base;
  int* prv = A.prev + base;
  unsigned long long* Q = A.queue + base;
  const double b0 = A.bound[4 * b], b1 = A.bound[4 * b + 1], b2 = A.bound[4 * b + 2], b3 = A.bound[4 * b + 3];
  const double gx = A.goal[2 * b], gy = A.goal[2 * b + 1];
  const double* __restrict__ obs = A.obs + (size_t)b * A.n_obs * 3;
  const int no = A.obs_count ? A.obs_count[b] : A.n_obs;
  const double* __restrict__ U = A.uni + (size_t)b * A.n_iter * 3;
  const double gamma = 0.01 * (b1 - b0) * (b3 - b2);  // nearDisk (:195)
  const double inf = __builtin_inf();

  if (tid == 0) {  // defineRRT (setup.jl:15-32): node 1 is the start
    X[0] = A.start[2 * b];
    Y[0] = A.start[2 * b + 1];
    C[0] = 0.0;
    par[0] = -1;
    chd[0] = nxt[0] = prv[0] = -1;
  }
  __syncthreads();

  int n = 1, n_tree = 1, buf = 0;              // sample_idx, the BallTree snapshot's size, buffer_idx
  int c_rej = 0, c_rew = 0, c_cap = 0, c_in = 0;
  bool cyc = false;
  double u0 = U[0], u1 = U[1], u2 = U[2];
  for (int it = 0; it < A.n_iter; it++) {
    // sampleRRT (:18-39)
    const double sx = u0 < A.bias_rate ? gx : u1 * (b1 - b0) + b0;
    const double sy = u0 < A.bias_rate ? gy : u2 * (b3 - b2) + b2;
    if (it + 1 < A.n_iter) {  // the next iteration's uniforms, ahead of their use
      u0 = U[3 * (it + 1)];
      u1 = U[3 * (it + 1) + 1];
      u2 = U[3 * (it + 1) + 2];
    }
    // knn(balltree, loc, 1) (:351) over the snapshot
    double bd = inf;
    int bi = INT_MAX;
    for (int i = tid; i < n_tree; i += RRT_T) {
      const double ex = X[i] - sx, ey = Y[i] - sy;
      const double d = ex * ex + ey * ey;
      if (d < bd) {
        bd = d;
        bi = i;
      }
    }
    rrt_block_argmin(bd, bi, s_rd, s_ri);
    if (bi == INT_MAX) bi = 0;  // no distance compares (NaN): node 1
    const double px = X[bi], py = Y[bi], pc = C[bi];

    // steer (:159-191)
    double nx = sx, ny = sy, nc;
    RrtProj P = rrt_proj(px, py, sx, sy);
    double p1 = P.p1, p2 = P.p2;
    const double dist = mpj_sqrt(p1 * p1 + p2 * p2);
    if (dist <= A.grow_max && dist >= A.grow_min) {
      nc = pc + rrt_ncost(p1, p2);
      c_in++;
    } else {
      if (dist > 0.001) {
        const double k = A.grow_max / dist;
        nx = px + p1 * k;  // FromProj2Real (:138-144)
        ny = py + p2 * k;
      }
      P = rrt_proj(px, py, nx, ny);
      p1 = mpj_fabs(P.p1) <= 0.01 ? 0.01 : P.p1;
      nx = px + p1;
      ny = py + P.p2;
      P = rrt_proj(px, py, nx, ny);
      nc = pc + rrt_ncost(P.p1, P.p2);
    }

    // collision (:282-311): every wavefront tests all circles, so the result needs no exchange
    bool col = rrt_oob(nx, ny, b0, b1, b2, b3);
    if (!col) {
      bool h = false;
      for (int k = lane; k < no; k += 64) h |= rrt_hit(obs + 3 * k, px, py, nx, ny);
      col = __any(h);
    }
    if (col) {
      c_rej++;
      continue;
    }

    // registerNode (:326-335)
    const int me = n;
    if (tid == 0) {
      X[me] = nx;
      Y[me] = ny;
      C[me] = nc;
      par[me] = bi + 1;
      chd[me] = -1;
      prv[me] = -1;
      const int f = chd[bi];
      nxt[me] = f;
      if (f >= 0) prv[f] = me;
      chd[bi] = me;
    }
    n++;
    buf++;

    if (A.rrt_star) {
      // nearDisk (:194-197); minimum([a, 50]) propagates a NaN
      const double a = gamma * mpj_sqrt(mpj_log((double)n) / (double)n);
      const double r = (a < 50.0 || a != a) ? a : 50.0;
      if (tid == 0) s_cnt = s_sel = s_rw = 0;
      __syncthreads();
      // inrange(balltree, new, r) (:374) over the snapshot (the new node is not in it)
      for (int i = tid; i < n_tree; i += RRT_T) {
        const double ex = X[i] - nx, ey = Y[i] - ny;
        const double ds = mpj_sqrt(ex * ex + ey * ey);
        if (ds <= r) {
          const int p = atomicAdd(&s_cnt, 1);
          if (p < RRT_SET) {
            s_nd[p] = ds;
            s_ni[p] = i;
          }
        }
      }
      __syncthreads();
      const int M = s_cnt;
      int nn = M;
      if (M < RRT_NEAR) {
        if (tid < M) s_near[tid] = s_ni[tid];
      } else if (M <= RRT_SET) {
        // knn(balltree, new, 100) (:376): the 100 nearest lie in the disk; rank by (distance, index)
        c_cap++;
        nn = RRT_NEAR;
        for (int e = tid; e < M; e += RRT_T) {
          const double de = s_nd[e];
          const int ie = s_ni[e];
          int rank = 0;
          for (int j = 0; j < M; j++) rank += rrt_less(s_nd[j], s_ni[j], de, ie);
          if (rank < RRT_NEAR) {
            const int p = atomicAdd(&s_sel, 1);
            if (p < RRT_NEAR) s_near[p] = ie;
          }
        }
      } else {
        // more candidates than LDS holds: the 100th smallest (distance, index) by search over the snapshot,
        // first on the distance's bit pattern (monotone for non-negative doubles), then on the index among its
        // ties; every counting scan tests seven thresholds, so the interval shrinks eightfold per scan
        c_cap++;
        nn = RRT_NEAR;
        long long klo = -1, khi = r > 0.0 ? (long long)__double_as_longlong(r) : 0;
        int ilo = -1, ihi = n_tree - 1;
        long long tk[RRT_WAYS];
        int ti[RRT_WAYS], cn[RRT_WAYS];
        // a tree piled up on the new node (duplicates of the goal): 100 ties at distance zero settle phase 0
#pragma unroll
        for (int j = 0; j < RRT_WAYS; j++) {
          tk[j] = 0;
          ti[j] = INT_MAX;
        }
        rrt_count_le(X, Y, n_tree, nx, ny, tk, ti, cn, s_cw);
        if (cn[0] >= RRT_NEAR) khi = 0;
        for (int phase = 0; phase < 2; phase++) {
          while (phase == 0 ? khi - klo > 1 : ihi - ilo > 1) {
#pragma unroll
            for (int j = 0; j < RRT_WAYS; j++) {
              if (phase == 0) {
                const long long w = khi - klo;
                tk[j] = klo + (w >> 3) * (j + 1) + (((w & 7) * (j + 1)) >> 3);
                ti[j] = INT_MAX;
              } else {
                tk[j] = khi;
                ti[j] = ilo + (int)(((long long)(ihi - ilo) * (j + 1)) >> 3);
              }
            }
            rrt_count_le(X, Y, n_tree, nx, ny, tk, ti, cn, s_cw);
            bool done = false;  // the first threshold that 100 keys reach is the new upper end
#pragma unroll
            for (int j = 0; j < RRT_WAYS; j++) {
              if (done) continue;
              if (cn[j] >= RRT_NEAR) {
                if (phase == 0) khi = tk[j]; else ihi = ti[j];
                done = true;
              } else {
                if (phase == 0) klo = tk[j]; else ilo = ti[j];
              }
            }
          }
        }
        for (int i = tid; i < n_tree; i += RRT_T) {
          const double ex = X[i] - nx, ey = Y[i] - ny;
          const long long kb = (long long)__double_as_longlong(mpj_sqrt(ex * ex + ey * ey));
          if ((kb < khi) || (kb == khi && i <= ihi)) {
            const int p = atomicAdd(&s_sel, 1);
            if (p < RRT_NEAR) s_near[p] = i;
          }
        }
      }
      __syncthreads();
      if (M >= RRT_NEAR) nn = min(s_sel, RRT_NEAR);

      // rewire (:216-238), root_idx = min_idx: one near node per lane; the tests read only costs that
      // this loop does not change
      if (tid < nn) {
        const int j = s_near[tid];
        if (j != bi) {
          const double jx = X[j], jy = Y[j];
          const RrtProj Pj = rrt_proj(jx, jy, nx, ny);
          const double change = (nc + rrt_ncost(Pj.p1, Pj.p2)) - C[j];
          if (change < 0.0 && par[j] >= 1) {
            bool hit = rrt_oob(jx, jy, b0, b1, b2, b3);
            for (int k = 0; k < no && !hit; k++) hit = rrt_hit(obs + 3 * k, nx, ny, jx, jy);
            if (!hit) {
              const int p = atomicAdd(&s_rw, 1);
              s_rwi[p] = j;
              s_rwd[p] = change;
            }
          }
        }
      }
      __syncthreads();
      const int R = s_rw;
      c_rew += R;
      if (R > 0) {
        if (tid == 0) {  // move every rewired node under the new one
          for (int k = 0; k < R; k++) {
            const int j = s_rwi[k], op = par[j] - 1;
            const int pj = prv[j], nj = nxt[j];
            if (pj >= 0) nxt[pj] = nj; else chd[op] = nj;
            if (nj >= 0) prv[nj] = pj;
            const int f = chd[me];
            nxt[j] = f;
            prv[j] = -1;
            if (f >= 0) prv[f] = j;
            chd[me] = j;
            par[j] = me + 1;
            Q[k] = ((unsigned long long)k << 32) | (unsigned)j;
          }
          s_tail = R;
        }
        __syncthreads();
        // costPropogation (:240-268): the rewired subtrees are disjoint and every node in them receives one
        // cost += costchange, so the order is free: breadth first, the lanes split each level
        int head = 0, tail = R;
        while (head < tail) {
          for (int q = head + tid; q < tail; q += RRT_T) {
            const unsigned long long e = Q[q];
            const int v = (int)(unsigned)e, slot = (int)(e >> 32);
            C[v] = C[v] + s_rwd[slot];
            for (int c = chd[v]; c >= 0; c = nxt[c]) {
              const int p = atomicAdd(&s_tail, 1);
              if (p < cap) Q[p] = ((unsigned long long)slot << 32) | (unsigned)c;
            }
          }
          __syncthreads();
          head = tail;
          tail = s_tail;
          __syncthreads();
          if (tail > cap) {  // more entries than nodes: the links hold a cycle (never in a tree)
            cyc = true;
            break;
          }
        }
      }
    }

    if (buf == A.buffer_size) {  // BallTree rebuild (:386-389)
      // thread 0 registered the nodes that enter the snapshot here and every thread reads them from the next
      // scan on; without rrt_star nothing else orders those stores before these loads
      __syncthreads();
      n_tree = n;
      buf = 0;
    }
  }
  __syncthreads();

  // findBestIdx (:414-422) over all nodes
  const double tol2 = A.tol * A.tol;
  double bc = inf;
  int bi = INT_MAX;
  for (int i = tid; i < n; i += RRT_T) {
    const double ex = X[i] - gx, ey = Y[i] - gy;
    if (ex * ex + ey * ey <= tol2) {
      const double c = C[i];
      if (bi == INT_MAX || c < bc) {
        bc = c;
        bi = i;
      }
    }
  }
  rrt_block_argmin(bc, bi, s_rd, s_ri);
  const int solved = bi != INT_MAX;
  // getBestIdxs (:433-441): goal side first, ending in node 1
  int* path = A.path_idx + base;
  if (tid == 0) {
    int cnt = 0;
    if (solved) {
      int k = bi;
      path[cnt++] = k + 1;
      while (k != 0 && cnt < n) {
        k = par[k] - 1;
        path[cnt++] = k + 1;
      }
    }
    s_cnt = cnt;
    A.n_nodes[b] = n;
    A.status[b] = solved;
    A.best_idx[b] = solved ? bi + 1 : 0;
    A.best_cost[b] = solved ? bc : 0.0;
    A.path_n[b] = cnt;
    A.counters[4 * b] = c_rej;
    A.counters[4 * b + 1] = c_rew;
    A.counters[4 * b + 2] = c_cap;
    A.counters[4 * b + 3] = c_in;
    if (cyc) *A.err = 1;
  }
  __syncthreads();
  // slots past the last node read as zero
  for (int i = s_cnt + tid; i < cap; i += RRT_T) path[i] = 0;
  for (int i = n + tid; i < cap; i += RRT_T) {
    X[i] = 0.0;
    Y[i] = 0.0;
    C[i] = 0.0;
    par[i] = 0;
  }
}

bool rrt_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace

extern "C" {

int mp_rrt_plan(mp_ctx* ctx, const mp_rrt_params_t* p, int32_t B, const double* bound, const double* start,
                const double* goal, int32_t n_obs, const int32_t* obs_count, const double* obstacles,
                const double* uniforms, int32_t* n_nodes, int32_t* status, int32_t* best_idx, double* best_cost,
                double* loc, double* cost, int32_t* parent, int32_t* path_idx, int32_t* path_n, int32_t* counters) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, p != nullptr, "params is NULL");
  MP_CHECK(ctx, p->n_iter >= 1 && p->n_iter <= MP_RRT_MAX_ITER, "n_iter %d: must be in 1 .. %d", p->n_iter,
           MP_RRT_MAX_ITER);
  MP_CHECK(ctx, p->buffer_size >= 1, "buffer_size %d: must be >= 1", p->buffer_size);
  MP_CHECK(ctx, p->rrt_star == 0 || p->rrt_star == 1, "rrt_star must be 0 or 1");
  MP_CHECK(ctx, B >= 1 && bound && start && goal && uniforms && n_nodes && status && best_idx && best_cost,
           "bad arguments");
  MP_CHECK(ctx, n_obs >= 0 && (n_obs == 0 || obstacles), "bad obstacle list");
  MP_CHECK(ctx, (path_idx != nullptr) == (path_n != nullptr), "path_idx and path_n go together");
  const size_t nB = (size_t)B, cap = (size_t)p->n_iter + 1, no = (size_t)n_obs;
  if (obs_count)
    for (int s = 0; s < B; s++)
      MP_CHECK(ctx, obs_count[s] >= 0 && obs_count[s] <= n_obs, "obs_count[%d] = %d: must be in 0 .. n_obs", s,
               obs_count[s]);
  MP_CHECK(ctx, rrt_finite(bound, 4 * nB) && rrt_finite(start, 2 * nB) && rrt_finite(goal, 2 * nB) &&
                    std::isfinite(p->bias_rate) && std::isfinite(p->grow_min) && std::isfinite(p->grow_max) &&
                    std::isfinite(p->goal_tolerance),
           "bounds, start, goal and settings must be finite");
  MP_HIP(ctx, hipSetDevice(ctx->device));

  // inputs: [bound 4B | start 2B | goal 2B | obstacles 3 n_obs B] doubles, the counts, the uniforms
  std::vector<double> in(nB * (8 + 3 * no));
  std::copy(bound, bound + 4 * nB, in.begin());
  std::copy(start, start + 2 * nB, in.begin() + 4 * nB);
  std::copy(goal, goal + 2 * nB, in.begin() + 6 * nB);
  if (n_obs) std::copy(obstacles, obstacles + 3 * no * nB, in.begin() + 8 * nB);
  int st = MP_OK;
  const double* din = mp_upload(ctx, WS_RRT_IN, in.data(), in.size(), &st);
  const int* dcnt = obs_count ? mp_upload(ctx, WS_RRT_CNT, (const int*)obs_count, nB, &st) : nullptr;
  const double* duni = mp_upload(ctx, WS_RRT_UNI, uniforms, 3 * (size_t)p->n_iter * nB, &st);
  // tree: x, y, cost (double), queue (u64), parent, child, next, prev (int); then the path and the scalars
  char* tree = (char*)mp_ws(ctx, WS_RRT_TREE, nB * cap * (4 * 8 + 4 * 4));
  char* out = (char*)mp_ws(ctx, WS_RRT_OUT, nB * cap * 4 + nB * (8 + 8 * 4) + 8);
  if (st || !din || (obs_count && !dcnt) || !duni || !tree || !out) return st ? st : MP_ERR_NOMEM;

  RrtArgs A{};
  A.n_iter = p->n_iter;
  A.buffer_size = p->buffer_size;
  A.rrt_star = p->rrt_star;
  A.n_obs = n_obs;
  A.bias_rate = p->bias_rate;
  A.grow_min = p->grow_min;
  A.grow_max = p->grow_max;
  A.tol = p->goal_tolerance;
  A.bound = din;
  A.start = din + 4 * nB;
  A.goal = din + 6 * nB;
  A.obs = din + 8 * nB;
  A.uni = duni;
  A.obs_count = dcnt;
  A.x = (double*)tree;
  A.y = A.x + nB * cap;
  A.cost = A.y + nB * cap;
  A.queue = (unsigned long long*)(A.cost + nB * cap);
  A.parent = (int*)(A.queue + nB * cap);
  A.child = A.parent + nB * cap;
  A.next = A.child + nB * cap;
  A.prev = A.next + nB * cap;
  A.best_cost = (double*)out;
  A.n_nodes = (int*)(A.best_cost + nB);
  A.status = A.n_nodes + nB;
  A.best_idx = A.status + nB;
  A.path_n = A.best_idx + nB;
  A.counters = A.path_n + nB;
  A.err = A.counters + 4 * nB;
  A.path_idx = A.err + 2;
  MP_HIP(ctx, hipMemsetAsync(A.err, 0, sizeof(int), ctx->stream));
  mp_time_begin(ctx);
  hipLaunchKernelGGL(rrt_plan_kernel, dim3((unsigned)B), dim3(RRT_T), 0, ctx->stream, A);
  MP_HIP(ctx, hipGetLastError());
  mp_time_end(ctx);

  int err = 0;
  if ((st = mp_download(ctx, n_nodes, (const int32_t*)A.n_nodes, nB))) return st;
  if ((st = mp_download(ctx, status, (const int32_t*)A.status, nB))) return st;
  if ((st = mp_download(ctx, best_idx, (const int32_t*)A.best_idx, nB))) return st;
  if ((st = mp_download(ctx, best_cost, (const double*)A.best_cost, nB))) return st;
  if ((st = mp_download(ctx, path_n, (const int32_t*)A.path_n, nB))) return st;
  if ((st = mp_download(ctx, counters, (const int32_t*)A.counters, 4 * nB))) return st;
  if ((st = mp_download(ctx, path_idx, (const int32_t*)A.path_idx, nB * cap))) return st;
  if ((st = mp_download(ctx, cost, (const double*)A.cost, nB * cap))) return st;
  if ((st = mp_download(ctx, parent, (const int32_t*)A.parent, nB * cap))) return st;
  if ((st = mp_download(ctx, &err, (const int*)A.err, 1))) return st;
  std::vector<double> xy;
  if (loc) {
    xy.resize(2 * nB * cap);
    if ((st = mp_download(ctx, xy.data(), (const double*)A.x, 2 * nB * cap))) return st;  // x then y
  }
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (loc)
    for (size_t i = 0; i < nB * cap; i++) {
      loc[2 * i] = xy[i];
      loc[2 * i + 1] = xy[nB * cap + i];
    }
  if (err) return mp_fail(ctx, MP_ERR_NUMERIC, "RRT*: the child links of a tree hold a cycle");
  return MP_OK;
}

}  // extern "C"
