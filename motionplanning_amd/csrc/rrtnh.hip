// rrtnh.hip — the car-like sampling planner for gfx950 (PathPlanning/RRTNonholonomic/src/{rrt_utils,setup,
// types}.jl: planRRT!, RRT and RRT* over poses [x, y, psi]) + C-ABI: mp_rrtnh_plan (B independent trees in one
// launch).
//
// rrtnh_plan_kernel  the whole planRRT! loop (rrt_utils.jl:528-583) of one scene per workgroup, laid out as
//                    rrt.hip's rrt_plan_kernel: the tree lives in the context workspace, one record (x, y, psi,
//                    cost) and one of links (parent, first child, siblings) per node, plus the propagation
//                    queue; LDS holds the reductions, the in-disk candidates, the near set, the rewire list
//                    and the counters.  Every value that steers the control
//                    flow (sample, nearest node, steer, collision, counts) is computed or read identically by all
//                    lanes, so the loop needs no broadcasts; the lanes split the snapshot scans (one MyMetrics
//                    value per node and scan), the near set and the cost propagation.  The near-set scan keeps
//                    every node's metric value in a per-scene array, so the search for the 30 smallest among
//                    more candidates than LDS holds ranks stored values instead of recomputing atan and sin.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#define MPJ_LANE_SAFE 1
#include "../../include/mp_jlmath.h"
#include "runtime.hpp"

namespace {

constexpr int NH_T = 512;            // threads per workgroup (8 wavefronts)
constexpr int NH_W = NH_T / 64;
constexpr int NH_NEAR = 30;          // planRRT!'s cap on the near set (:547-549)
constexpr int NH_WAYS = 7;           // thresholds per counting scan of the search beyond NH_SET
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

struct NhArgs {
  int n_iter, buffer_size, rrt_star, n_obs;
  double bias_rate, grow_min, grow_max, tol;
  const double *bound, *start, *goal, *obs, *uni;  // [B][4], [B][3], [B][2], [B][n_obs][3], [B][n_iter][6]
  const int* obs_count;                            // [B] or null
  // tree state, [B][n_iter + 1] each
  NhNode* node;
  NhLink* link;
  double* met;                // MyMetrics of every snapshot node to the newest node
  unsigned long long* queue;  // cost propagation: (rewire slot << 32) | node slot
  int *n_nodes, *status, *best_idx, *path_n, *counters, *path_idx, *err;
  double* best_cost;
};

// round(v, digits = 2 | 3): Base's _round_digits with RoundNearest
__device__ __forceinline__ double nh_round2(double v) { return __builtin_rint(v * 100.0) / 100.0; }
__device__ __forceinline__ double nh_round3(double v) { return __builtin_rint(v * 1000.0) / 1000.0; }
// Base.sign: +-1, and x itself (+-0, NaN) otherwise
__device__ __forceinline__ double nh_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : x); }

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
    dpsi = mpj_acos(nh_round2(mpj_fma(uy, as, ux * ac) / den)) * nh_sign(sg);
  }
  double sn, cs;  // mpj_sincos: the bits of mpj_sin and mpj_cos over one argument reduction
  mpj_sincos(dpsi, &sn, &cs);
  return {nh_round2(rho * cs), nh_round2(rho * sn), nh_round3(bp - ap)};
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

__device__ __forceinline__ bool nh_oob(double x, double y, double b0, double b1, double b2, double b3) {
  return x < b0 || x > b1 || y < b2 || y > b3;  // CheckWithinBoundary (:450-456)
}
// both end points of the segment against circle o (:489-495)
__device__ __forceinline__ bool nh_hit(const double* __restrict__ o, double x1, double y1, double x2, double y2) {
  const double ox = o[0], oy = o[1], rr = o[2] * o[2];
  const double e1 = x1 - ox, f1 = y1 - oy, e2 = x2 - ox, f2 = y2 - oy;
  return (e1 * e1 + f1 * f1 <= rr) || (e2 * e2 + f2 * f2 <= rr);
}

__device__ __forceinline__ bool nh_less(double d, int i, double od, int oi) { return d < od || (d == od && i < oi); }

// (d, i) -> the block's minimum by (d, then i), in every thread
__device__ __forceinline__ void nh_block_argmin(double& d, int& i, double* sd, int* si) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const double od = __shfl_xor(d, off);
    const int oi = __shfl_xor(i, off);
    if (nh_less(od, oi, d, i)) {
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
  for (int w = 1; w < NH_W; w++)
    if (nh_less(sd[w], si[w], d, i)) {
      d = sd[w];
      i = si[w];
    }
}

// the key of a stored metric value: its bit pattern (monotone for non-negative doubles), a NaN above all
__device__ __forceinline__ long long nh_key(double d) {
  return d == d ? (long long)__double_as_longlong(d) : LLONG_MAX;
}

// cn[j] = the number of snapshot nodes whose key (nh_key of the stored metric, index) is at most (tk[j], ti[j]),
// in every thread
__device__ __forceinline__ void nh_count_le(const double* D, int n_tree, const long long* tk, const int* ti, int* cn,
                                            int (*s_cw)[NH_WAYS]) {
#pragma unroll
  for (int j = 0; j < NH_WAYS; j++) cn[j] = 0;
  for (int i = threadIdx.x; i < n_tree; i += NH_T) {
    const long long kb = nh_key(D[i]);
#pragma unroll
    for (int j = 0; j < NH_WAYS; j++) cn[j] += (kb < tk[j]) || (kb == tk[j] && i <= ti[j]);
  }
#pragma unroll
  for (int j = 0; j < NH_WAYS; j++)
    for (int off = 32; off; off >>= 1) cn[j] += __shfl_xor(cn[j], off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NH_WAYS; j++) s_cw[threadIdx.x >> 6][j] = cn[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NH_WAYS; j++) {
    int t = 0;
    for (int w = 0; w < NH_W; w++) t += s_cw[w][j];
    cn[j] = t;
  }
}

__global__ __launch_bounds__(NH_T) void rrtnh_plan_kernel(NhArgs A) {
  __shared__ double s_rd[NH_W];
  __shared__ int s_ri[NH_W];
  __shared__ double s_nd[NH_SET];   // in-disk candidates: metric, node slot
  __shared__ int s_ni[NH_SET];
  __shared__ int s_near[NH_NEAR];   // the near set
  __shared__ int s_rwi[NH_NEAR];    // rewired nodes and their cost changes
  __shared__ double s_rwd[NH_NEAR];
  __shared__ int s_cw[NH_W][NH_WAYS];  // per-wave counts of the search beyond NH_SET
  __shared__ int s_cnt, s_sel, s_rw, s_tail;
  __shared__ int s_ctr[8];  // the counters, kept by thread 0

  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int cap = A.n_iter + 1;
  const size_t base = (size_t)b * cap;
  NhNode* N = A.node + base;
  NhLink* L = A.link + base;
  double* D = A.met + base;
  unsigned long long* Q = A.queue + base;
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
    for (int i = tid; i < n_tree; i += NH_T) {
      const double d = nh_metric(N[i].x, N[i].y, N[i].psi, sx, sy, sp);
      if (d < bd) {
        bd = d;
        bi = i;
      }
    }
    nh_block_argmin(bd, bi, s_rd, s_ri);
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
    if (nh_oob(nx, ny, b0, b1, b2, b3)) {
      if (tid == 0) s_ctr[0]++;
      continue;
    }
    if (!nh_feasible(P)) {
      if (tid == 0) s_ctr[1]++;
      continue;
    }
    {
      bool h = false;
      for (int k = lane; k < no; k += 64) h |= nh_hit(obs + 3 * k, px, py, nx, ny);
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
      if (tid == 0) s_cnt = s_sel = s_rw = 0;
      __syncthreads();
      // inrange(balltree, new, r) (:546) over the snapshot (the new node is not in it); every value is kept
      for (int i = tid; i < n_tree; i += NH_T) {
        const double ds = nh_metric(N[i].x, N[i].y, N[i].psi, nx, ny, np);
        D[i] = ds;
        if (ds <= r) {
          const int p = atomicAdd(&s_cnt, 1);
          if (p < NH_SET) {
            s_nd[p] = ds;
            s_ni[p] = i;
          }
        }
      }
      __syncthreads();
      const int M = s_cnt;
      int nn = M;
      if (M < NH_NEAR) {
        if (tid < M) s_near[tid] = s_ni[tid];
      } else if (M <= NH_SET) {
        // knn(balltree, new, 30) (:548): the 30 smallest lie in the disk; rank by (metric, index)
        if (tid == 0) s_ctr[4]++;
        nn = NH_NEAR;
        for (int e = tid; e < M; e += NH_T) {
          const double de = s_nd[e];
          const int ie = s_ni[e];
          int rank = 0;
          for (int j = 0; j < M; j++) rank += nh_less(s_nd[j], s_ni[j], de, ie);
          if (rank < NH_NEAR) {
            const int p = atomicAdd(&s_sel, 1);
            if (p < NH_NEAR) s_near[p] = ie;
          }
        }
      } else {
        // more candidates than LDS holds: the 30th smallest (metric, index) by search over the stored values,
        // first on the value's bit pattern, then on the index among its ties; every counting scan tests seven
        // thresholds, so the interval shrinks eightfold per scan.  Each thread reads the values it stored
        if (tid == 0) s_ctr[4]++;
        nn = NH_NEAR;
        long long klo = -1, khi = r > 0.0 ? (long long)__double_as_longlong(r) : 0;
        int ilo = -1, ihi = n_tree - 1;
        long long tk[NH_WAYS];
        int ti[NH_WAYS], cn[NH_WAYS];
        for (int phase = 0; phase < 2; phase++) {
          while (phase == 0 ? khi - klo > 1 : ihi - ilo > 1) {
#pragma unroll
            for (int j = 0; j < NH_WAYS; j++) {
              if (phase == 0) {
                const long long w = khi - klo;
                tk[j] = klo + (w >> 3) * (j + 1) + (((w & 7) * (j + 1)) >> 3);
                ti[j] = INT_MAX;
              } else {
                tk[j] = khi;
                ti[j] = ilo + (int)(((long long)(ihi - ilo) * (j + 1)) >> 3);
              }
            }
            nh_count_le(D, n_tree, tk, ti, cn, s_cw);
            bool done = false;  // the first threshold that 30 keys reach is the new upper end
#pragma unroll
            for (int j = 0; j < NH_WAYS; j++) {
              if (done) continue;
              if (cn[j] >= NH_NEAR) {
                if (phase == 0) khi = tk[j]; else ihi = ti[j];
                done = true;
              } else {
                if (phase == 0) klo = tk[j]; else ilo = ti[j];
              }
            }
          }
        }
        for (int i = tid; i < n_tree; i += NH_T) {
          const long long kb = nh_key(D[i]);
          if ((kb < khi) || (kb == khi && i <= ihi)) {
            const int p = atomicAdd(&s_sel, 1);
            if (p < NH_NEAR) s_near[p] = i;
          }
        }
      }
      __syncthreads();
      if (M >= NH_NEAR) nn = min(s_sel, NH_NEAR);

      // rewire (:392-414), root_idx = min_idx: one near node per lane; the tests read only costs that this loop
      // does not change, and collision(new, near) reads only poses, which never change
      if (tid < nn) {
        const int j = s_near[tid];
        if (j != bi) {
          const double jx = N[j].x, jy = N[j].y, jp = N[j].psi;
          double jcs, jsn;
          mpj_sincos(jp, &jsn, &jcs);
          const NhProj Pj = nh_proj(jx, jy, jp, jcs, jsn, nx, ny, np);
          const double change = (nc + nh_ncost(Pj)) - N[j].cost;
          if (change < 0.0 && L[j].parent >= 1) {
            bool hit = nh_oob(jx, jy, b0, b1, b2, b3);
            if (!hit) hit = !nh_feasible(nh_proj(nx, ny, np, ncs, nsn, jx, jy, jp));
            for (int k = 0; k < no && !hit; k++) hit = nh_hit(obs + 3 * k, nx, ny, jx, jy);
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
      if (tid == 0) s_ctr[3] += R;
      if (R > 0) {
        if (tid == 0) {  // move every rewired node under the new one
          for (int k = 0; k < R; k++) {
            const int j = s_rwi[k], op = L[j].parent - 1;
            const int pj = L[j].prev, nj = L[j].next;
            if (pj >= 0) L[pj].next = nj; else L[op].child = nj;
            if (nj >= 0) L[nj].prev = pj;
            const int f = L[me].child;
            L[j].next = f;
            L[j].prev = -1;
            if (f >= 0) L[f].prev = j;
            L[me].child = j;
            L[j].parent = me + 1;
            Q[k] = ((unsigned long long)k << 32) | (unsigned)j;
          }
          s_tail = R;
        }
        __syncthreads();
        // costPropogation (:416-431): the rewired subtrees are disjoint and every node in them receives one
        // cost += costchange, so the order is free: breadth first, the lanes split each level
        int head = 0, tail = R;
        while (head < tail) {
          for (int q = head + tid; q < tail; q += NH_T) {
            const unsigned long long e = Q[q];
            const int v = (int)(unsigned)e, slot = (int)(e >> 32);
            N[v].cost = N[v].cost + s_rwd[slot];
            for (int c = L[v].child; c >= 0; c = L[c].next) {
              const int p = atomicAdd(&s_tail, 1);
              if (p < cap) Q[p] = ((unsigned long long)slot << 32) | (unsigned)c;
            }
          }
          __syncthreads();
          head = tail;
          tail = s_tail;
          __syncthreads();
          if (tail > cap) {  // more entries than nodes: the links hold a cycle (never in a tree)
            if (tid == 0) *A.err = 1;
            break;
          }
        }
      }
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

  // findBestIdx (:585-593) over all nodes
  const double tol2 = A.tol * A.tol;
  double bc = inf;
  int bi = INT_MAX;
  for (int i = tid; i < n; i += NH_T) {
    const double ex = N[i].x - gx, ey = N[i].y - gy;
    if (ex * ex + ey * ey <= tol2) {
      const double c = N[i].cost;
      if (bi == INT_MAX || c < bc) {
        bc = c;
        bi = i;
      }
    }
  }
  nh_block_argmin(bc, bi, s_rd, s_ri);
  const int solved = bi != INT_MAX;
  // getBestIdxs (:604-612): goal side first, ending in node 1
  int* path = A.path_idx + base;
  if (tid == 0) {
    int cnt = 0;
    if (solved) {
      int k = bi;
      path[cnt++] = k + 1;
      while (k != 0 && cnt < n) {
        k = L[k].parent - 1;
        path[cnt++] = k + 1;
      }
    }
    s_cnt = cnt;
    A.n_nodes[b] = n;
    A.status[b] = solved;
    A.best_idx[b] = solved ? bi + 1 : 0;
    A.best_cost[b] = solved ? bc : 0.0;
    A.path_n[b] = cnt;
    for (int k = 0; k < 8; k++) A.counters[8 * b + k] = s_ctr[k];
  }
  __syncthreads();
  // slots past the last node read as zero
  for (int i = s_cnt + tid; i < cap; i += NH_T) path[i] = 0;
  for (int i = n + tid; i < cap; i += NH_T) {
    N[i] = {0.0, 0.0, 0.0, 0.0};
    L[i].parent = 0;
  }
}

bool nh_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace

extern "C" {

int mp_rrtnh_plan(mp_ctx* ctx, const mp_rrt_params_t* p, int32_t B, const double* bound, const double* start,
                  const double* goal, int32_t n_obs, const int32_t* obs_count, const double* obstacles,
                  const double* uniforms, int32_t* n_nodes, int32_t* status, int32_t* best_idx, double* best_cost,
                  double* state, double* cost, int32_t* parent, int32_t* path_idx, int32_t* path_n,
                  int32_t* counters) {
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
  MP_CHECK(ctx, nh_finite(bound, 4 * nB) && nh_finite(start, 3 * nB) && nh_finite(goal, 2 * nB) &&
                    std::isfinite(p->bias_rate) && std::isfinite(p->grow_min) && std::isfinite(p->grow_max) &&
                    std::isfinite(p->goal_tolerance),
           "bounds, start, goal and settings must be finite");
  MP_HIP(ctx, hipSetDevice(ctx->device));

  // inputs: [bound 4B | start 3B | goal 2B | obstacles 3 n_obs B] doubles, the counts, the uniforms; the
  // workspace slots are mp_rrt_plan's (calls on one context run one after the other)
  std::vector<double> in(nB * (9 + 3 * no));
  std::copy(bound, bound + 4 * nB, in.begin());
  std::copy(start, start + 3 * nB, in.begin() + 4 * nB);
  std::copy(goal, goal + 2 * nB, in.begin() + 7 * nB);
  if (n_obs) std::copy(obstacles, obstacles + 3 * no * nB, in.begin() + 9 * nB);
  int st = MP_OK;
  const double* din = mp_upload(ctx, WS_RRT_IN, in.data(), in.size(), &st);
  const int* dcnt = obs_count ? mp_upload(ctx, WS_RRT_CNT, (const int*)obs_count, nB, &st) : nullptr;
  const double* duni = mp_upload(ctx, WS_RRT_UNI, uniforms, 6 * (size_t)p->n_iter * nB, &st);
  // tree: the nodes, the metric values, the queue, the links; then the path and the scalars
  char* tree = (char*)mp_ws(ctx, WS_RRT_TREE, nB * cap * (sizeof(NhNode) + sizeof(NhLink) + 2 * 8));
  char* out = (char*)mp_ws(ctx, WS_RRT_OUT, nB * cap * 4 + nB * (8 + 12 * 4) + 8);
  if (st || !din || (obs_count && !dcnt) || !duni || !tree || !out) return st ? st : MP_ERR_NOMEM;

  NhArgs A{};
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
  A.goal = din + 7 * nB;
  A.obs = din + 9 * nB;
  A.uni = duni;
  A.obs_count = dcnt;
  A.node = (NhNode*)tree;
  A.met = (double*)(A.node + nB * cap);
  A.queue = (unsigned long long*)(A.met + nB * cap);
  A.link = (NhLink*)(A.queue + nB * cap);
  A.best_cost = (double*)out;
  A.n_nodes = (int*)(A.best_cost + nB);
  A.status = A.n_nodes + nB;
  A.best_idx = A.status + nB;
  A.path_n = A.best_idx + nB;
  A.counters = A.path_n + nB;
  A.err = A.counters + 8 * nB;
  A.path_idx = A.err + 2;
  MP_HIP(ctx, hipMemsetAsync(A.err, 0, sizeof(int), ctx->stream));
  mp_time_begin(ctx);
  hipLaunchKernelGGL(rrtnh_plan_kernel, dim3((unsigned)B), dim3(NH_T), 0, ctx->stream, A);
  MP_HIP(ctx, hipGetLastError());
  mp_time_end(ctx);

  int err = 0;
  if ((st = mp_download(ctx, n_nodes, (const int32_t*)A.n_nodes, nB))) return st;
  if ((st = mp_download(ctx, status, (const int32_t*)A.status, nB))) return st;
  if ((st = mp_download(ctx, best_idx, (const int32_t*)A.best_idx, nB))) return st;
  if ((st = mp_download(ctx, best_cost, (const double*)A.best_cost, nB))) return st;
  if ((st = mp_download(ctx, path_n, (const int32_t*)A.path_n, nB))) return st;
  if ((st = mp_download(ctx, counters, (const int32_t*)A.counters, 8 * nB))) return st;
  if ((st = mp_download(ctx, path_idx, (const int32_t*)A.path_idx, nB * cap))) return st;
  if ((st = mp_download(ctx, &err, (const int*)A.err, 1))) return st;
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
