// rrt_common.hpp — what the sampling planners share: rrt.hip (points, Euclidean distance, the tree as arrays) and
// rrtnh.hip (poses, MyMetrics, a node and a link record per node).  Device side: the geometry tests, the block
// reductions, the near set among the in-disk candidates, a rewire's re-linking and cost propagation and the kernel's
// tail.  Host side: the argument checks, the inputs and results in the WS_RRT_* slots, and the downloads.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "runtime.hpp"

constexpr int RC_T = 512;    // threads per workgroup (8 wavefronts)
constexpr int RC_W = RC_T / 64;
constexpr int RC_WAYS = 7;   // thresholds per counting scan of the search beyond the LDS set

// the kernel arguments both planners have, the settings as given first; RrtArgs and NhArgs add their tree
struct RcArgs : mp_rrt_params_t {
  int n_obs;
  const double *bound, *start, *goal, *obs, *uni;  // [B][4], [B][start_w], [B][2], [B][n_obs][3], [B][n_iter][n_uni]
  const int* obs_count;                            // [B] or null
  int *n_nodes, *status, *best_idx, *path_n, *counters, *path_idx, *err;
  double* best_cost;
};

// a workgroup's LDS: the reductions, the in-disk candidates (SET), the near set and the rewire list (NEAR each)
template <int NEAR, int SET>
struct RcLds {
  double rd[RC_W], nd[SET], rwd[NEAR];  // reduction slots; candidates' distances; rewired nodes' cost changes
  int ri[RC_W], ni[SET], near[NEAR], rwi[NEAR];
  int cw[RC_W][RC_WAYS];  // per-wave counts of the search beyond SET
  int cnt, sel, rw, tail;
};

// round(v, digits = 2): Base's _round_digits with RoundNearest
__device__ __forceinline__ double rc_round2(double v) { return __builtin_rint(v * 100.0) / 100.0; }
// Base.sign: +-1, and x itself (+-0, NaN) otherwise
__device__ __forceinline__ double rc_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : x); }

__device__ __forceinline__ bool rc_oob(double x, double y, double b0, double b1, double b2, double b3) {
  return x < b0 || x > b1 || y < b2 || y > b3;  // CheckWithinBoundary
}
// both end points of the segment against circle o
__device__ __forceinline__ bool rc_hit(const double* __restrict__ o, double x1, double y1, double x2, double y2) {
  const double ox = o[0], oy = o[1], rr = o[2] * o[2];
  const double e1 = x1 - ox, f1 = y1 - oy, e2 = x2 - ox, f2 = y2 - oy;
  return (e1 * e1 + f1 * f1 <= rr) || (e2 * e2 + f2 * f2 <= rr);
}

__device__ __forceinline__ bool rc_less(double d, int i, double od, int oi) { return d < od || (d == od && i < oi); }

// (d, i) -> the block's minimum by (d, then i), in every thread
__device__ __forceinline__ void rc_block_argmin(double& d, int& i, double* sd, int* si) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const double od = __shfl_xor(d, off);
    const int oi = __shfl_xor(i, off);
    if (rc_less(od, oi, d, i)) {
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
  for (int w = 1; w < RC_W; w++)
    if (rc_less(sd[w], si[w], d, i)) {
      d = sd[w];
      i = si[w];
    }
}

// cn[j] = the number of snapshot nodes whose (key(i), i) is at most (tk[j], ti[j]), in every thread
template <typename Key>
__device__ __forceinline__ void rc_count_le(const Key& key, int n_tree, const long long* tk, const int* ti, int* cn,
                                            int (*s_cw)[RC_WAYS]) {
#pragma unroll
  for (int j = 0; j < RC_WAYS; j++) cn[j] = 0;
  for (int i = threadIdx.x; i < n_tree; i += RC_T) {
    const long long kb = key(i);
#pragma unroll
    for (int j = 0; j < RC_WAYS; j++) cn[j] += (kb < tk[j]) || (kb == tk[j] && i <= ti[j]);
  }
#pragma unroll
  for (int j = 0; j < RC_WAYS; j++)
    for (int off = 32; off; off >>= 1) cn[j] += __shfl_xor(cn[j], off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < RC_WAYS; j++) s_cw[threadIdx.x >> 6][j] = cn[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RC_WAYS; j++) {
    int t = 0;
    for (int w = 0; w < RC_W; w++) t += s_cw[w][j];
    cn[j] = t;
  }
}

// The near set of the new node, S.near[0 .. return value), from the M snapshot nodes within r, of which S.nd / S.ni
// hold the first SET (S.sel is 0, and a barrier lies behind the candidates' stores).  Fewer than NEAR: all of them.
// Up to SET: knn(balltree, new, NEAR), the NEAR smallest by (distance, index), ranked in LDS.  More than LDS holds:
// the NEAR-th smallest (key, index) by search over the snapshot, first on the key (the distance's bit pattern,
// monotone for non-negative doubles), then on the index among its ties; a counting scan tests seven thresholds, so
// the interval shrinks eightfold per scan.  ZERO_PILE: one scan up front settles NEAR ties at distance zero
template <bool ZERO_PILE, int NEAR, int SET, typename Key>
__device__ __forceinline__ int rc_near_set(RcLds<NEAR, SET>& S, int M, int n_tree, double r, const Key& key) {
  const int tid = threadIdx.x;
  if (M < NEAR) {
    if (tid < M) S.near[tid] = S.ni[tid];
  } else if (M <= SET) {
    for (int e = tid; e < M; e += RC_T) {
      const double de = S.nd[e];
      const int ie = S.ni[e];
      int rank = 0;
      for (int j = 0; j < M; j++) rank += rc_less(S.nd[j], S.ni[j], de, ie);
      if (rank < NEAR) {
        const int p = atomicAdd(&S.sel, 1);
        if (p < NEAR) S.near[p] = ie;
      }
    }
  } else {
    long long klo = -1, khi = r > 0.0 ? (long long)__double_as_longlong(r) : 0;
    int ilo = -1, ihi = n_tree - 1;
    long long tk[RC_WAYS];
    int ti[RC_WAYS], cn[RC_WAYS];
    if (ZERO_PILE) {
#pragma unroll
      for (int j = 0; j < RC_WAYS; j++) {
        tk[j] = 0;
        ti[j] = INT_MAX;
      }
      rc_count_le(key, n_tree, tk, ti, cn, S.cw);
      if (cn[0] >= NEAR) khi = 0;
    }
    for (int phase = 0; phase < 2; phase++) {
      while (phase == 0 ? khi - klo > 1 : ihi - ilo > 1) {
#pragma unroll
        for (int j = 0; j < RC_WAYS; j++) {
          if (phase == 0) {
            const long long w = khi - klo;
            tk[j] = klo + (w >> 3) * (j + 1) + (((w & 7) * (j + 1)) >> 3);
            ti[j] = INT_MAX;
          } else {
            tk[j] = khi;
            ti[j] = ilo + (int)(((long long)(ihi - ilo) * (j + 1)) >> 3);
          }
        }
        rc_count_le(key, n_tree, tk, ti, cn, S.cw);
        bool done = false;  // the first threshold that NEAR keys reach is the new upper end
#pragma unroll
        for (int j = 0; j < RC_WAYS; j++) {
          if (done) continue;
          if (cn[j] >= NEAR) {
            if (phase == 0) khi = tk[j]; else ihi = ti[j];
            done = true;
          } else {
            if (phase == 0) klo = tk[j]; else ilo = ti[j];
          }
        }
      }
    }
    for (int i = tid; i < n_tree; i += RC_T) {
      const long long kb = key(i);
      if ((kb < khi) || (kb == khi && i <= ihi)) {
        const int p = atomicAdd(&S.sel, 1);
        if (p < NEAR) S.near[p] = i;
      }
    }
  }
  __syncthreads();
  return M < NEAR ? M : min(S.sel, NEAR);
}

// A tree view T gives references into one scene's storage: parent(i) (1-based, -1: root), child(i), next(i),
// prev(i) (0-based node slots, -1: none), cost(i), x(i), y(i); clear(i) zeroes the outputs of an unused slot.
//
// The R accepted rewires of S.rwi / S.rwd (a barrier lies behind their stores): thread 0 moves every rewired node
// under the new node `me`; then costPropogation: the rewired subtrees are disjoint and every node in them receives
// one cost += costchange, so the order is free: breadth first over Q ((rewire slot << 32) | node slot), the lanes
// split each level.  More entries than nodes: the links hold a cycle (never in a tree), *err is set
template <int NEAR, int SET, typename Tree>
__device__ __forceinline__ void rc_rewire_apply(const Tree& T, RcLds<NEAR, SET>& S, unsigned long long* Q, int me,
                                                int R, int cap, int* err) {
  const int tid = threadIdx.x;
  if (R <= 0) return;
  if (tid == 0) {
    for (int k = 0; k < R; k++) {
      const int j = S.rwi[k], op = T.parent(j) - 1;
      const int pj = T.prev(j), nj = T.next(j);
      if (pj >= 0) T.next(pj) = nj; else T.child(op) = nj;
      if (nj >= 0) T.prev(nj) = pj;
      const int f = T.child(me);
      T.next(j) = f;
      T.prev(j) = -1;
      if (f >= 0) T.prev(f) = j;
      T.child(me) = j;
      T.parent(j) = me + 1;
      Q[k] = ((unsigned long long)k << 32) | (unsigned)j;
    }
    S.tail = R;
  }
  __syncthreads();
  int head = 0, tail = R;
  while (head < tail) {
    for (int q = head + tid; q < tail; q += RC_T) {
      const unsigned long long e = Q[q];
      const int v = (int)(unsigned)e, slot = (int)(e >> 32);
      T.cost(v) = T.cost(v) + S.rwd[slot];
      for (int c = T.child(v); c >= 0; c = T.next(c)) {
        const int p = atomicAdd(&S.tail, 1);
        if (p < cap) Q[p] = ((unsigned long long)slot << 32) | (unsigned)c;
      }
    }
    __syncthreads();
    head = tail;
    tail = S.tail;
    __syncthreads();
    if (tail > cap) {
      if (tid == 0) *err = 1;
      return;
    }
  }
}

// The kernel's tail for a tree of n nodes: findBestIdx over all nodes, getBestIdxs (goal side first, ending in
// node 1), the scene's scalar outputs with the NC counters of ctr, and zeroes in the slots past the last node
template <int NC, int NEAR, int SET, typename Tree>
__device__ __forceinline__ void rc_finish(const RcArgs& A, const Tree& T, RcLds<NEAR, SET>& S, int n, const int* ctr) {
  const int tid = threadIdx.x, b = blockIdx.x, cap = A.n_iter + 1;
  const double gx = A.goal[2 * b], gy = A.goal[2 * b + 1], tol2 = A.goal_tolerance * A.goal_tolerance;
  double bc = __builtin_inf();
  int bi = INT_MAX;
  for (int i = tid; i < n; i += RC_T) {
    const double ex = T.x(i) - gx, ey = T.y(i) - gy;
    if (ex * ex + ey * ey <= tol2) {
      const double c = T.cost(i);
      if (bi == INT_MAX || c < bc) {
        bc = c;
        bi = i;
      }
    }
  }
  rc_block_argmin(bc, bi, S.rd, S.ri);
  const int solved = bi != INT_MAX;
  int* path = A.path_idx + (size_t)b * cap;
  if (tid == 0) {
    int cnt = 0;
    if (solved) {
      int k = bi;
      path[cnt++] = k + 1;
      while (k != 0 && cnt < n) {
        k = T.parent(k) - 1;
        path[cnt++] = k + 1;
      }
    }
    S.cnt = cnt;
    A.n_nodes[b] = n;
    A.status[b] = solved;
    A.best_idx[b] = solved ? bi + 1 : 0;
    A.best_cost[b] = solved ? bc : 0.0;
    A.path_n[b] = cnt;
    for (int k = 0; k < NC; k++) A.counters[NC * b + k] = ctr[k];
  }
  __syncthreads();
  for (int i = S.cnt + tid; i < cap; i += RC_T) path[i] = 0;
  for (int i = n + tid; i < cap; i += RC_T) T.clear(i);
}

// ---- host side: the arguments mp_rrt_plan and mp_rrtnh_plan have in common, in their order
struct RcCall {
  const mp_rrt_params_t* p;
  int32_t B;
  const double *bound, *start, *goal;  // start: [B][start_w]
  int32_t n_obs;
  const int32_t* obs_count;
  const double *obstacles, *uniforms;
  int32_t *n_nodes, *status, *best_idx;
  double* best_cost;
  int32_t *path_idx, *path_n, *counters;
};

inline int rc_validate(mp_ctx* ctx, const RcCall& C, int start_w) {
  if (!ctx) return MP_ERR_INVALID;
  const mp_rrt_params_t* p = C.p;
  MP_CHECK(ctx, p != nullptr, "params is NULL");
  MP_CHECK(ctx, p->n_iter >= 1 && p->n_iter <= MP_RRT_MAX_ITER, "n_iter %d: must be in 1 .. %d", p->n_iter,
           MP_RRT_MAX_ITER);
  MP_CHECK(ctx, p->buffer_size >= 1, "buffer_size %d: must be >= 1", p->buffer_size);
  MP_CHECK(ctx, p->rrt_star == 0 || p->rrt_star == 1, "rrt_star must be 0 or 1");
  MP_CHECK(ctx, C.B >= 1 && C.bound && C.start && C.goal && C.uniforms && C.n_nodes && C.status && C.best_idx &&
                    C.best_cost,
           "bad arguments");
  MP_CHECK(ctx, C.n_obs >= 0 && (C.n_obs == 0 || C.obstacles), "bad obstacle list");
  MP_CHECK(ctx, (C.path_idx != nullptr) == (C.path_n != nullptr), "path_idx and path_n go together");
  if (C.obs_count)
    for (int s = 0; s < C.B; s++)
      MP_CHECK(ctx, C.obs_count[s] >= 0 && C.obs_count[s] <= C.n_obs, "obs_count[%d] = %d: must be in 0 .. n_obs", s,
               C.obs_count[s]);
  const size_t nB = (size_t)C.B;
  MP_CHECK(ctx, mp_all_finite(C.bound, 4 * nB) && mp_all_finite(C.start, start_w * nB) &&
                    mp_all_finite(C.goal, 2 * nB) && std::isfinite(p->bias_rate) && std::isfinite(p->grow_min) && std::isfinite(p->grow_max) &&
                    std::isfinite(p->goal_tolerance),
           "bounds, start, goal and settings must be finite");
  return MP_OK;
}

// Fills A: the inputs on the device, [bound 4B | start start_w B | goal 2B | obstacles 3 n_obs B] doubles (packed in
// `in`, which outlives the call's last synchronise), the counts, n_uni uniforms per iteration; *tree = node_bytes per
// node and scene; the results: best_cost, 4 + n_ctr ints per scene, the error word (cleared), the paths
inline int rc_stage(mp_ctx* ctx, const RcCall& C, int start_w, int n_uni, int n_ctr, size_t node_bytes,
                    std::vector<double>* in, RcArgs* A, char** tree) {
  const size_t nB = (size_t)C.B, cap = (size_t)C.p->n_iter + 1, no = (size_t)C.n_obs, sw = (size_t)start_w;
  MP_HIP(ctx, hipSetDevice(ctx->device));
  in->resize(nB * (6 + sw + 3 * no));
  std::copy(C.bound, C.bound + 4 * nB, in->begin());
  std::copy(C.start, C.start + sw * nB, in->begin() + 4 * nB);
  std::copy(C.goal, C.goal + 2 * nB, in->begin() + (4 + sw) * nB);
  if (no) std::copy(C.obstacles, C.obstacles + 3 * no * nB, in->begin() + (6 + sw) * nB);
  int st = MP_OK;
  const double* din = mp_upload(ctx, WS_RRT_IN, in->data(), in->size(), &st);
  const int* dcnt = C.obs_count ? mp_upload(ctx, WS_RRT_CNT, (const int*)C.obs_count, nB, &st) : nullptr;
  const double* duni = mp_upload(ctx, WS_RRT_UNI, C.uniforms, (size_t)n_uni * C.p->n_iter * nB, &st);
  *tree = (char*)mp_ws(ctx, WS_RRT_TREE, nB * cap * node_bytes);
  char* out = (char*)mp_ws(ctx, WS_RRT_OUT, nB * cap * 4 + nB * (8 + (4 + (size_t)n_ctr) * 4) + 8);
  if (st || !din || (C.obs_count && !dcnt) || !duni || !*tree || !out) return st ? st : MP_ERR_NOMEM;
  static_cast<mp_rrt_params_t&>(*A) = *C.p;
  A->n_obs = C.n_obs;
  A->bound = din;
  A->start = din + 4 * nB;
  A->goal = din + (4 + sw) * nB;
  A->obs = din + (6 + sw) * nB;
  A->uni = duni;
  A->obs_count = dcnt;
  A->best_cost = (double*)out;
  A->n_nodes = (int*)(A->best_cost + nB);
  A->status = A->n_nodes + nB;
  A->best_idx = A->status + nB;
  A->path_n = A->best_idx + nB;
  A->counters = A->path_n + nB;
  A->err = A->counters + (size_t)n_ctr * nB;
  A->path_idx = A->err + 2;
  MP_HIP(ctx, hipMemsetAsync(A->err, 0, sizeof(int), ctx->stream));
  return MP_OK;
}

// the scalar outputs, the paths and the error word, enqueued on the context stream (the caller synchronises)
inline int rc_fetch(mp_ctx* ctx, const RcCall& C, int n_ctr, const RcArgs& A, int* err) {
  const size_t nB = (size_t)C.B, cap = (size_t)C.p->n_iter + 1;
  int st;
  if ((st = mp_download(ctx, C.n_nodes, (const int32_t*)A.n_nodes, nB))) return st;
  if ((st = mp_download(ctx, C.status, (const int32_t*)A.status, nB))) return st;
  if ((st = mp_download(ctx, C.best_idx, (const int32_t*)A.best_idx, nB))) return st;
  if ((st = mp_download(ctx, C.best_cost, (const double*)A.best_cost, nB))) return st;
  if ((st = mp_download(ctx, C.path_n, (const int32_t*)A.path_n, nB))) return st;
  if ((st = mp_download(ctx, C.counters, (const int32_t*)A.counters, (size_t)n_ctr * nB))) return st;
  if ((st = mp_download(ctx, C.path_idx, (const int32_t*)A.path_idx, nB * cap))) return st;
  return mp_download(ctx, err, (const int*)A.err, 1);
}
