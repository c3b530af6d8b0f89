// rrtnh.hip — the car-like sampling planner for gfx950 (PathPlanning/RRTNonholonomic/src/{rrt_utils,setup,
// types}.jl: planRRT!, RRT and RRT* over poses [x, y, psi]) + C-ABI: mp_rrtnh_plan (B independent trees in one
// launch).
//
// rrtnh_plan_kernel  the whole planRRT! loop (rrt_utils.jl:528-583) of one scene per workgroup, no host round
//                    trip per iteration.  The tree lives in the context workspace, one record (x, y, psi,
//                    cost) and one of links (parent, first child, siblings) per node, plus the propagation
//                    queue; LDS holds the reductions, the in-disk candidates, the near set, the rewire list
//                    and the counters.  Every value that steers the control flow (sample, nearest node, steer,
//                    collision, counts) is computed or read identically by all lanes, so the loop needs no
//                    broadcasts; the lanes split the snapshot scans (one MyMetrics value per node and scan), the
//                    near set and the cost propagation.  The near-set scan keeps every node's metric value in a
//                    per-scene array, so the search for the 30 smallest among more candidates than LDS holds
//                    ranks stored values instead of recomputing atan and sin.
#define MPJ_LANE_SAFE 1
#include "../../include/mp_jlmath.h"
#include "rrt_common.hpp"

namespace {

constexpr int NH_NEAR = 30;          // planRRT!'s cap on the near set (:547-549)
constexpr int NH_SET = 256;          // in-disk candidates LDS holds; beyond it the 30 smallest are searched for
constexpr double NH_RADIUS = 24.0;   // nearDisk's cap (:372)
constexpr double NH_MAX_ANG = 0.1;   // get_max_ang_ratio (:116)
constexpr double NH_PI = 3.141592653589793;  // Float64(pi)

// One record per node and one per node's links keep the pointers the loop holds few (they live in scalar
// registers); a scan reads x, y and psi of a node together
struct NhNode {
  double x, y, psi, cost;
};
struct NhLink {  // child, next, prev: 0-based node slots (-1: none); parent is 1-based (-1: root)
  int parent, child, next, prev;
};

struct NhArgs : RcArgs {  // bound [B][4], start [B][3], uni [B][n_iter][6]
  // tree state, [B][n_iter + 1] each
  NhNode* node;
  NhLink* link;
  double* met;                // MyMetrics of every snapshot node to the newest node
  unsigned long long* queue;  // cost propagation: (rewire slot << 32) | node slot
};

struct NhTree {  // one scene's records
  NhNode* N;
  NhLink* L;
  __device__ __forceinline__ double& x(int i) const { return N[i].x; }
  __device__ __forceinline__ double& y(int i) const { return N[i].y; }
  __device__ __forceinline__ double& cost(int i) const { return N[i].cost; }
  __device__ __forceinline__ int& parent(int i) const { return L[i].parent; }
  __device__ __forceinline__ int& child(int i) const { return L[i].child; }
  __device__ __forceinline__ int& next(int i) const { return L[i].next; }
  __device__ __forceinline__ int& prev(int i) const { return L[i].prev; }
  __device__ __forceinline__ void clear(int i) const {
    N[i] = {0.0, 0.0, 0.0, 0.0};
    L[i].parent = 0;
  }
};

// a snapshot node's key in the search beyond NH_SET: the bit pattern of its stored metric value (monotone for
// non-negative doubles), a NaN above all
__device__ __forceinline__ long long nh_key(double d) {
  return d == d ? (long long)__double_as_longlong(d) : LLONG_MAX;
}
struct NhKey {
  const double* D;
  __device__ __forceinline__ long long operator()(int i) const { return nh_key(D[i]); }
};

// round(v, digits = 3): Base's _round_digits with RoundNearest
__device__ __forceinline__ double nh_round3(double v) { return __builtin_rint(v * 1000.0) / 1000.0; }

// MyMetrics (types.jl:9-23) of the poses a and b
__device__ __forceinline__ double nh_metric(double ax, double ay, double ap, double bx, double by, double bp) {
  const double ex = bx - ax, ey = by - ay;
  const double r = mpj_sqrt(ex * ex + ey * ey) + 0.1;
  const double fx = ax - bx;
  const double rho = mpj_fabs(fx) <= 0.01 ? NH_PI / 2.0 : mpj_atan((ay - by) / fx);
  const double d = bp - ap;
  const double e1 = ap - rho, e2 = bp - rho;
  const double w = r * mpj_sin(((ap + bp) / 2.0 - rho) * 2.0);
  return (40.0 * (2.0 * (e1 * e1) + 2.0 * (e2 * e2)) + 10.0 * (d * d)) + w * w;
}

// ProjectionStates (:208-238) of the pose (bx, by, bp) seen from (ax, ay, ap); (ac, as) = (cos ap, sin ap)
struct NhProj {
  double p1, p2, p3;
};
__device__ __forceinline__ NhProj nh_proj(double ax, double ay, double ap, double ac, double as, double bx, double by,
                                          double bp) {
  const double dx = bx - ax, dy = by - ay;
  const double nrm = mpj_sqrt(dx * dx + dy * dy);
  double rho = 0.0, dpsi = 0.0;
  if (nrm >= 0.001) {
    rho = nrm;
    const double ux = dx / nrm, uy = dy / nrm;
    const double sg = ac * uy - as * ux;
    const double den = mpj_sqrt(ux * ux + uy * uy) * mpj_sqrt(ac * ac + as * as);
    dpsi = mpj_acos(rc_round2(mpj_fma(uy, as, ux * ac) / den)) * rc_sign(sg);
  }
  double sn, cs;  // mpj_sincos: the bits of mpj_sin and mpj_cos over one argument reduction
  mpj_sincos(dpsi, &sn, &cs);
  return {rc_round2(rho * cs), rc_round2(rho * sn), nh_round3(bp - ap)};
}

// neural_cost (:106-112)
__device__ __forceinline__ double nh_ncost(const NhProj& P) {
  const double dist = mpj_sqrt(P.p1 * P.p1 + P.p2 * P.p2);
  return 5.0 * dist + (P.p3 * P.p3) / dist;
}

// get_max_yawangle (:120-145): the lower and the upper bound of the yaw difference
__device__ __forceinline__ double nh_cubic(double p00, double p10, double p01, double p20, double p11, double p02,
                                           double p30, double p21, double p12, double p03, double x, double y) {
  return (((((((((p00 + p10 * x) + p01 * y) + p20 * (x * x)) + p11 * x * y) + p02 * (y * y)) + p30 * (x * x * x)) +
            p21 * (x * x) * y) + p12 * x * (y * y)) + p03 * (y * y * y));
}
__device__ __forceinline__ void nh_yaw_bounds(double x, double y, double& lo, double& hi) {
  lo = nh_cubic(-0.03911, 0.05831, 0.1148, -0.04344, 0.4135, -0.05552, 0.005515, -0.05701, 0.1892, -0.1725, x, y);
  hi = nh_cubic(0.03911, -0.05831, 0.1148, 0.04344, 0.4135, 0.05552, -0.005515, -0.05701, -0.1892, -0.1725, x, y);
}

// InitialCheck (:240-258) && FeasibilityClassifier (:154-175, its test on theta one-sided as written there)
__device__ __forceinline__ bool nh_feasible(const NhProj& P) {
  if (P.p1 < 1.0 || P.p1 > 3.0) return false;
  if (P.p2 < -1.0 || P.p2 > 1.0) return false;
  if (P.p3 < -0.35 || P.p3 > 0.35) return false;
  const double dist = mpj_sqrt(P.p1 * P.p1 + P.p2 * P.p2);
  const double theta = mpj_atan(P.p2 / P.p1);
  if (theta > mpj_fabs((NH_MAX_ANG / dist) * dist)) return false;
  double lo, hi;
  nh_yaw_bounds(dist, theta, lo, hi);
  if (P.p3 < lo || P.p3 > hi) return false;
  return true;
}

// FromProj2Real (:261-277): h1 = (c, s), l1 = cross([0, 0, 1], h1) = (0*0 - 1*s, 1*c - 0*0)
__device__ __forceinline__ void nh_real(double ax, double ay, double ap, double c, double s, double q1, double q2,
                                        double q3, double& x, double& y, double& p) {
  const double l1x = 0.0 - s, l1y = c - 0.0;
  x = (ax + c * q1) + l1x * q2;
  y = (ay + s * q1) + l1y * q2;
  p = ap + q3;
}

__global__ __launch_bounds__(RC_T) void rrtnh_plan_kernel(NhArgs A) {
  __shared__ RcLds<NH_NEAR, NH_SET> S;
  __shared__ int s_ctr[8];  // the counters, kept by thread 0

  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int cap = A.n_iter + 1;
  const size_t base = (size_t)b * cap;
  NhNode* N = A.node + base;
  NhLink* L = A.link + base;
  double* D = A.met + base;
  unsigned long long* Q = A.queue + base;
  const NhTree T{N, L};
  const double b0 = A.bound[4 * b], b1 = A.bound[4 * b + 1], b2 = A.bound[4 * b + 2], b3 = A.bound[4 * b + 3];
  const double gx = A.goal[2 * b], gy = A.goal[2 * b + 1];
  const double* __restrict__ obs = A.obs + (size_t)b * A.n_obs * 3;
  const int no = A.obs_count ? A.obs_count[b] : A.n_obs;
  const double* __restrict__ U = A.uni + (size_t)b * A.n_iter * 6;
  const double gamma = 6.0 * (b1 - b0) * (b3 - b2) * 5.0;  // nearDisk (:371)
  const double inf = __builtin_inf();

  if (tid < 8) s_ctr[tid] = 0;
  if (tid == 0) {  // defineRRT (setup.jl:13-37): node 1 is the start pose
    N[0] = {A.start[3 * b], A.start[3 * b + 1], A.start[3 * b + 2], 0.0};
    L[0] = {-1, -1, -1, -1};
  }
  __syncthreads();

  int n = 1, n_tree = 1, buf = 0;  // sample_idx, the BallTree snapshot's size, buffer_idx
  double u0 = U[0], u1 = U[1], u2 = U[2], u3 = U[3], u4 = U[4], u5 = U[5];
  for (int it = 0; it < A.n_iter; it++) {
    // sampleRRT (:18-44)
    const double sx = u0 < A.bias_rate ? gx : u1 * (b1 - b0) + b0;
    const double sy = u0 < A.bias_rate ? gy : u2 * (b3 - b2) + b2;
    const double sp = (u3 - 0.5) * 2.0 * NH_PI;
    const double u_ratio = u4, u_yaw = u5;
    if (it + 1 < A.n_iter) {  // the next iteration's uniforms, ahead of their use
      const double* Un = U + 6 * (size_t)(it + 1);
      u0 = Un[0];
      u1 = Un[1];
      u2 = Un[2];
      u3 = Un[3];
      u4 = Un[4];
      u5 = Un[5];
    }
    // knn(balltree, pose, 1) (:536) over the snapshot, under MyMetrics
    double bd = inf;
    int bi = INT_MAX;
    for (int i = tid; i < n_tree; i += RC_T) {
      const double d = nh_metric(N[i].x, N[i].y, N[i].psi, sx, sy, sp);
      if (d < bd) {
        bd = d;
        bi = i;
      }
    }
    rc_block_argmin(bd, bi, S.rd, S.ri);
    if (bi == INT_MAX) bi = 0;  // no value compares (NaN): node 1
    const double px = N[bi].x, py = N[bi].y, pp = N[bi].psi, pc = N[bi].cost;
    double pcs, psn;
    mpj_sincos(pp, &psn, &pcs);

    // steer (:292-365)
    double nx = sx, ny = sy, np = sp;
    NhProj P = nh_proj(px, py, pp, pcs, psn, nx, ny, np);
    const double dist = mpj_sqrt(P.p1 * P.p1 + P.p2 * P.p2);
    double sd = dist;  // the step: dist in range, adjustdist = grow_max (:331) otherwise
    if (dist <= A.grow_max && dist >= A.grow_min) {
      if (tid == 0) s_ctr[5]++;
    } else {
      sd = A.grow_max;
      if (dist > 0.001) {
        const double k = sd / dist;
        nh_real(px, py, pp, pcs, psn, P.p1 * k, P.p2 * k, P.p3, nx, ny, np);
      }
      P = nh_proj(px, py, pp, pcs, psn, nx, ny, np);
    }
    {
      const double mar = NH_MAX_ANG / sd;  // get_max_ang_ratio
      const double q1 = mpj_fabs(P.p1) <= 0.01 ? 0.01 : P.p1;
      const double dpsi = mpj_atan(P.p2 / q1);
      double ang_ratio;
      if (mpj_fabs(dpsi) / sd > mar) {
        ang_ratio = (2.0 * u_ratio - 1.0) * mar;
        if (tid == 0) s_ctr[6]++;
      } else {
        ang_ratio = dpsi / sd;
      }
      // decide_proj (:282-290) with DistToDeltaXY (:147-152)
      const double ang = ang_ratio * sd;
      double lo, hi;
      nh_yaw_bounds(sd, ang_ratio * sd, lo, hi);
      double asn, acs;
      mpj_sincos(ang, &asn, &acs);
      nh_real(px, py, pp, pcs, psn, sd * acs, sd * asn, u_yaw * (hi - lo) + lo, nx, ny, np);
    }
    P = nh_proj(px, py, pp, pcs, psn, nx, ny, np);
    const double nc = pc + nh_ncost(P);

    // collision (:458-498): the bound test, the kinematics of the edge (its projection is P), the circles; every
    // wavefront tests all circles, so the result needs no exchange
    if (rc_oob(nx, ny, b0, b1, b2, b3)) {
      if (tid == 0) s_ctr[0]++;
      continue;
    }
    if (!nh_feasible(P)) {
      if (tid == 0) s_ctr[1]++;
      continue;
    }
    {
      bool h = false;
      for (int k = lane; k < no; k += 64) h |= rc_hit(obs + 3 * k, px, py, nx, ny);
      if (__any(h)) {
        if (tid == 0) s_ctr[2]++;
        continue;
      }
    }

    // registerNode (:513-522)
    const int me = n;
    if (tid == 0) {
      N[me] = {nx, ny, np, nc};
      const int f = L[bi].child;
      L[me] = {bi + 1, -1, f, -1};
      if (f >= 0) L[f].prev = me;
      L[bi].child = me;
    }
    n++;
    buf++;

    if (A.rrt_star) {
      // nearDisk (:370-373); minimum([a, 24]) propagates a NaN
      const double a = gamma * (mpj_log((double)n) / (double)n);
      const double r = (a < NH_RADIUS || a != a) ? a : NH_RADIUS;
      if (tid == 0) s_ctr[7] += r < NH_RADIUS;
      double ncs, nsn;
      mpj_sincos(np, &nsn, &ncs);
      if (tid == 0) S.cnt = S.sel = S.rw = 0;
      __syncthreads();
      // inrange(balltree, new, r) (:546) over the snapshot (the new node is not in it); every value is kept
      for (int i = tid; i < n_tree; i += RC_T) {
        const double ds = nh_metric(N[i].x, N[i].y, N[i].psi, nx, ny, np);
        D[i] = ds;
        if (ds <= r) {
          const int p = atomicAdd(&S.cnt, 1);
          if (p < NH_SET) {
            S.nd[p] = ds;
            S.ni[p] = i;
          }
        }
      }
      __syncthreads();
      const int M = S.cnt;
      // fewer than 30: the near set; else knn(balltree, new, 30) (:548): the 30 smallest lie in the disk; beyond
      // NH_SET the search ranks the stored values, and each thread reads the values it stored
      if (tid == 0 && M >= NH_NEAR) s_ctr[4]++;
      const int nn = rc_near_set<false>(S, M, n_tree, r, NhKey{D});

      // rewire (:392-414), root_idx = min_idx: one near node per lane; the tests read only costs that this loop
      // does not change, and collision(new, near) reads only poses, which never change
      if (tid < nn) {
        const int j = S.near[tid];
        if (j != bi) {
          const double jx = N[j].x, jy = N[j].y, jp = N[j].psi;
          double jcs, jsn;
          mpj_sincos(jp, &jsn, &jcs);
          const NhProj Pj = nh_proj(jx, jy, jp, jcs, jsn, nx, ny, np);
          const double change = (nc + nh_ncost(Pj)) - N[j].cost;
          if (change < 0.0 && L[j].parent >= 1) {
            bool hit = rc_oob(jx, jy, b0, b1, b2, b3);
            if (!hit) hit = !nh_feasible(nh_proj(nx, ny, np, ncs, nsn, jx, jy, jp));
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
      if (tid == 0) s_ctr[3] += R;
      rc_rewire_apply(T, S, Q, me, R, cap, A.err);  // re-linking, costPropogation (:416-431)
    }

    if (buf == A.buffer_size) {  // BallTree rebuild (:558-561)
      // thread 0 registered the nodes that enter the snapshot here and every thread reads them from the next
      // scan on; without rrt_star nothing else orders those stores before these loads
      __syncthreads();
      n_tree = n;
      buf = 0;
    }
  }
  __syncthreads();

  rc_finish<8>(A, T, S, n, s_ctr);  // findBestIdx (:585-593), getBestIdxs (:604-612), outputs
}

}  // namespace

extern "C" {

int mp_rrtnh_plan(mp_ctx* ctx, const mp_rrt_params_t* p, int32_t B, const double* bound, const double* start,
                  const double* goal, int32_t n_obs, const int32_t* obs_count, const double* obstacles,
                  const double* uniforms, int32_t* n_nodes, int32_t* status, int32_t* best_idx, double* best_cost,
                  double* state, double* cost, int32_t* parent, int32_t* path_idx, int32_t* path_n,
                  int32_t* counters) {
  const RcCall C{p,        B,       bound,  start,    goal,      n_obs,    obs_count, obstacles,
                 uniforms, n_nodes, status, best_idx, best_cost, path_idx, path_n,    counters};
  if (int st = rc_validate(ctx, C, 3)) return st;
  const size_t nB = (size_t)B, cap = (size_t)p->n_iter + 1;
  NhArgs A{};
  std::vector<double> in;
  char* tree;
  // tree: the nodes, the metric values, the queue, the links
  if (int st = rc_stage(ctx, C, 3, 6, 8, sizeof(NhNode) + sizeof(NhLink) + 2 * 8, &in, &A, &tree)) return st;
  A.node = (NhNode*)tree;
  A.met = (double*)(A.node + nB * cap);
  A.queue = (unsigned long long*)(A.met + nB * cap);
  A.link = (NhLink*)(A.queue + nB * cap);
  mp_time_begin(ctx);
  hipLaunchKernelGGL(rrtnh_plan_kernel, dim3((unsigned)B), dim3(RC_T), 0, ctx->stream, A);
  MP_HIP(ctx, hipGetLastError());
  mp_time_end(ctx);

  int err = 0, st;
  if ((st = rc_fetch(ctx, C, 8, A, &err))) return st;
  std::vector<double> nodes;
  std::vector<int32_t> links;
  if (state || cost) {
    nodes.resize(4 * nB * cap);
    if ((st = mp_download(ctx, nodes.data(), (const double*)A.node, 4 * nB * cap))) return st;
  }
  if (parent) {
    links.resize(4 * nB * cap);
    if ((st = mp_download(ctx, links.data(), (const int32_t*)A.link, 4 * nB * cap))) return st;
  }
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < nB * cap; i++) {
    if (state) {
      state[3 * i] = nodes[4 * i];
      state[3 * i + 1] = nodes[4 * i + 1];
      state[3 * i + 2] = nodes[4 * i + 2];
    }
    if (cost) cost[i] = nodes[4 * i + 3];
    if (parent) parent[i] = links[4 * i];
  }
  if (err) return mp_fail(ctx, MP_ERR_NUMERIC, "RRT*: the child links of a tree hold a cycle");
  return MP_OK;
}

}  // extern "C"