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
#define MPJ_LANE_SAFE 1
#include "../../include/mp_jlmath.h"
#include "rrt_common.hpp"

namespace {

constexpr int RRT_NEAR = 100;  // planRRT!'s cap on the near set (:375-377)
constexpr int RRT_SET = 512;   // in-disk candidates LDS holds; beyond it the 100 nearest are searched for

struct RrtArgs : RcArgs {  // bound [B][4], start [B][2], uni [B][n_iter][3]
  // tree state, [B][n_iter + 1] each; links are 0-based node slots (-1: none), parent is 1-based (-1: root)
  double *x, *y, *cost;
  int *parent, *child, *next, *prev;
  unsigned long long* queue;  // cost propagation: (rewire slot << 32) | node slot
};

struct RrtTree {  // one scene's slice of the arrays
  double *X, *Y, *C;
  int *par, *chd, *nxt, *prv;
  __device__ __forceinline__ double& x(int i) const { return X[i]; }
  __device__ __forceinline__ double& y(int i) const { return Y[i]; }
  __device__ __forceinline__ double& cost(int i) const { return C[i]; }
  __device__ __forceinline__ int& parent(int i) const { return par[i]; }
  __device__ __forceinline__ int& child(int i) const { return chd[i]; }
  __device__ __forceinline__ int& next(int i) const { return nxt[i]; }
  __device__ __forceinline__ int& prev(int i) const { return prv[i]; }
  __device__ __forceinline__ void clear(int i) const {
    X[i] = Y[i] = C[i] = 0.0;
    par[i] = 0;
  }
};

// a snapshot node's key in the search beyond RRT_SET: the bit pattern of its distance to (nx, ny), recomputed
struct RrtKey {
  const double *X, *Y;
  double nx, ny;
  __device__ __forceinline__ long long operator()(int i) const {
    const double ex = X[i] - nx, ey = Y[i] - ny;
    return (long long)__double_as_longlong(mpj_sqrt(ex * ex + ey * ey));
  }
};

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
    dpsi = mpj_atan(uy / mpj_fabs(ux)) * rc_sign(ux);  // sign(0.0) = 0: a vertical segment has dpsi = 0
  }
  return {rc_round2(rho * mpj_cos(dpsi)), rc_round2(rho * mpj_sin(dpsi))};
}

// neural_cost (:101-106)
__device__ __forceinline__ double rrt_ncost(double p1, double p2) { return 5.0 * mpj_sqrt(p1 * p1 + p2 * p2); }

__global__ __launch_bounds__(RC_T) void rrt_plan_kernel(RrtArgs A) {
  __shared__ RcLds<RRT_NEAR, RRT_SET> S;

  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int cap = A.n_iter + 1;
  const size_t base = (size_t)b * cap;
  double *X = A.x + base, *Y = A.y + base, *C = A.cost + base;
  int *par = A.parent + base, *chd = A.child + base, *nxt = A.next + base, *prv = A.prev + base;
  unsigned long long* Q = A.queue + base;
  const RrtTree T{X, Y, C, par, chd, nxt, prv};
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
    for (int i = tid; i < n_tree; i += RC_T) {
      const double ex = X[i] - sx, ey = Y[i] - sy;
      const double d = ex * ex + ey * ey;
      if (d < bd) {
        bd = d;
        bi = i;
      }
    }
    rc_block_argmin(bd, bi, S.rd, S.ri);
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
    bool col = rc_oob(nx, ny, b0, b1, b2, b3);
    if (!col) {
      bool h = false;
      for (int k = lane; k < no; k += 64) h |= rc_hit(obs + 3 * k, px, py, nx, ny);
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
      if (tid == 0) S.cnt = S.sel = S.rw = 0;
      __syncthreads();
      // inrange(balltree, new, r) (:374) over the snapshot (the new node is not in it)
      for (int i = tid; i < n_tree; i += RC_T) {
        const double ex = X[i] - nx, ey = Y[i] - ny;
        const double ds = mpj_sqrt(ex * ex + ey * ey);
        if (ds <= r) {
          const int p = atomicAdd(&S.cnt, 1);
          if (p < RRT_SET) {
            S.nd[p] = ds;
            S.ni[p] = i;
          }
        }
      }
      __syncthreads();
      const int M = S.cnt;
      // fewer than 100: the near set; else knn(balltree, new, 100) (:376): the 100 nearest lie in the disk
      if (M >= RRT_NEAR) c_cap++;
      const int nn = rc_near_set<true>(S, M, n_tree, r, RrtKey{X, Y, nx, ny});

      // rewire (:216-238), root_idx = min_idx: one near node per lane; the tests read only costs that
      // this loop does not change
      if (tid < nn) {
        const int j = S.near[tid];
        if (j != bi) {
          const double jx = X[j], jy = Y[j];
          const RrtProj Pj = rrt_proj(jx, jy, nx, ny);
          const double change = (nc + rrt_ncost(Pj.p1, Pj.p2)) - C[j];
          if (change < 0.0 && par[j] >= 1) {
            bool hit = rc_oob(jx, jy, b0, b1, b2, b3);
            for (int k = 0; k < no && !hit; k++) hit = rc_hit(obs + 3 * k, nx, ny, jx, jy);
            if (!hit) {
              const int p = atomicAdd(&S.rw, 1);
              S.rwi[p] = j;
              S.rwd[p] = change;
            }
          }
        }
      }
      __syncthreads();
      const int R = S.rw;
      c_rew += R;
      rc_rewire_apply(T, S, Q, me, R, cap, A.err);  // re-linking, costPropogation (:240-268)
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

  const int ctr[4] = {c_rej, c_rew, c_cap, c_in};
  rc_finish<4>(A, T, S, n, ctr);  // findBestIdx (:414-422), getBestIdxs (:433-441), outputs
}

}  // namespace

extern "C" {

int mp_rrt_plan(mp_ctx* ctx, const mp_rrt_params_t* p, int32_t B, const double* bound, const double* start,
                const double* goal, int32_t n_obs, const int32_t* obs_count, const double* obstacles,
                const double* uniforms, int32_t* n_nodes, int32_t* status, int32_t* best_idx, double* best_cost,
                double* loc, double* cost, int32_t* parent, int32_t* path_idx, int32_t* path_n, int32_t* counters) {
  const RcCall C{p,        B,       bound,  start,    goal,      n_obs,    obs_count, obstacles,
                 uniforms, n_nodes, status, best_idx, best_cost, path_idx, path_n,    counters};
  if (int st = rc_validate(ctx, C, 2)) return st;
  const size_t nB = (size_t)B, cap = (size_t)p->n_iter + 1;
  RrtArgs A{};
  std::vector<double> in;
  char* tree;
  // tree: x, y, cost (double), queue (u64), parent, child, next, prev (int)
  if (int st = rc_stage(ctx, C, 2, 3, 4, 4 * 8 + 4 * 4, &in, &A, &tree)) return st;
  A.x = (double*)tree;
  A.y = A.x + nB * cap;
  A.cost = A.y + nB * cap;
  A.queue = (unsigned long long*)(A.cost + nB * cap);
  A.parent = (int*)(A.queue + nB * cap);
  A.child = A.parent + nB * cap;
  A.next = A.child + nB * cap;
  A.prev = A.next + nB * cap;
  mp_time_begin(ctx);
  hipLaunchKernelGGL(rrt_plan_kernel, dim3((unsigned)B), dim3(RC_T), 0, ctx->stream, A);
  MP_HIP(ctx, hipGetLastError());
  mp_time_end(ctx);

  int err = 0, st;
  if ((st = rc_fetch(ctx, C, 4, A, &err))) return st;
  if ((st = mp_download(ctx, cost, (const double*)A.cost, nB * cap))) return st;
  if ((st = mp_download(ctx, parent, (const int32_t*)A.parent, nB * cap))) return st;
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