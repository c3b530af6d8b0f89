// ilqr_plan.hpp — the plain C++ of mp_ilqr_solve's host side (ilqr.hip): the search plan, the map of the
// workspace and the loop's state.  No HIP type, so the plan and the map run on their own under host
// sanitizers (tools/ilqr_plan_check.cpp).
#pragma once
#include <cstddef>

struct IlqrPlan {
  int G;      // trials per search round: g_wide (kSearchG) on lane quads, else 4 or 1 single-lane trials
  size_t T2;  // slots per instance of the rest pass and the one-pass search: trials 0..ls_cap (0: neither)
  bool rest;  // the rest slots are wanted (ilqr_ws_acquire drops them when they cannot be had)
};

// Trial slots are 32 B of X and 16 B of U per (trial, instance, knot).  g_wide trials per round while the
// slots stay within 1 GiB of HBM and the context's workspace cap (ws_limit, 0 = none), else 4, else 1 (the
// sequential loop).  Rest slots (g_wide only, and only if the search can go past round 0) within 8 GiB; they
// hold trials 0..ls_cap, so that the same buffers serve the one-pass search.
inline IlqrPlan ilqr_plan(size_t B, size_t N, int ls_cap, size_t ws_limit, int g_wide) {
  auto fits = [&](size_t g) {
    return g * B * N * 48 <= ((size_t)1 << 30) && (!ws_limit || g * B * N * 32 <= ws_limit);
  };
  IlqrPlan P;
  P.G = fits((size_t)g_wide) ? g_wide : fits(4) ? 4 : 1;
  P.T2 = P.G == g_wide && ls_cap + 1 > P.G ? (size_t)(ls_cap + 1) : 0;
  P.rest = P.T2 > 0 && P.T2 * B * N * 48 <= ((size_t)8 << 30);
  return P;
}

// bytes of each workspace buffer of the solve (the rest buffers: what a plan with rest slots asks for)
struct IlqrWsBytes {
  size_t k, K, Xn, Un, J, ints, Xs, Us, Jt, pw;
};
inline IlqrWsBytes ilqr_ws_bytes(size_t B, size_t N, const IlqrPlan& P) {
  const size_t d = sizeof(double);
  return {d * 2 * (N - 1) * B,       d * 8 * (N - 1) * B,  d * 4 * N * B * P.G,  d * 2 * N * B * P.G, d * B,
          sizeof(int) * (5 * B + 4), d * 4 * N * B * P.T2, d * 2 * N * B * P.T2, d * B * P.T2,        sizeof(int) * 8 * B};
}

// every device pointer of the solve, named once
struct IlqrWs {
  double *X, *U;                // the trajectories, solved in place
  double *k, *K;                // gains of the backward pass
  double *Xn, *Un;              // G trial slots per instance (the search rounds)
  double* J;                    // current cost per instance
  int *active, *iters, *flags;  // [B] each
  // Two list buffers, each [pending count, active count, compact list of B]: iteration q's backward pass
  // reads list[(q + 1) & 1], its search writes list[q & 1] (search_accept).
  int* list[2];
  double *Xs, *Us, *Jt;  // T2 rest slots per instance and their trial costs (nullptr without rest slots)
  // Pipelined search, by launch parity: the instances its round 0 left pending, their winning-trial word and
  // their fixpoint m*.  The one-pass search has its own winm / mstar, so it never reads a slot the pipelined
  // launches left set.
  int *pend[2], *winm[2], *mstar[2];
  int *winm1, *mstar1;
};

// ints: 5 B + 4 words = active, iters, flags, list[0], list[1].  pw: 8 B words (nullptr: no rest slots) =
// pend[2], winm[2], mstar[2], winm1, mstar1; pend and winm are each contiguous over both parities.
inline void ilqr_ws_map(IlqrWs* W, size_t B, int* ints, int* pw) {
  W->active = ints;
  W->iters = ints + B;
  W->flags = ints + 2 * B;
  W->list[0] = ints + 3 * B;
  W->list[1] = W->list[0] + (2 + B);
  for (int q = 0; q < 2; q++) {
    W->pend[q] = pw ? pw + q * B : nullptr;
    W->winm[q] = pw ? pw + (2 + q) * B : nullptr;
    W->mstar[q] = pw ? pw + (4 + q) * B : nullptr;
  }
  W->winm1 = pw ? pw + 6 * B : nullptr;
  W->mstar1 = pw ? pw + 7 * B : nullptr;
}

// What the solve loop carries from one iteration to the next.
struct IlqrLoop {
  // The counts of the list buffer this iteration's search writes are zero: at the start (IlqrSolve::begin), and
  // after a one-pass or pipelined search, whose finish kernel zeroes the counts of the list it did not write.
  // The rounds-to-the-end search has no finish kernel: after it the loop zeroes them with a memset.
  bool counts_zero = true;
  // The one-pass search is armed: its winm is set (once, by a memset; then its finish kernels reset it).  It
  // arms when at most kOnePassMax instances are active (the host's last report) and the switch is terminal,
  // whatever later reports say.  Instances the last pipelined launch left pending keep their active flag and
  // their gains (they sat the backward pass out), so the one-pass search reruns them from trial 0: trials 0..15
  // give the bits round 0 gave, so they end exactly where their rest pass would.
  bool onepass = false;
  // Pipelined launches so far: launch q marks pend[q & 1] and runs the rest pass of pend[(q - 1) & 1], so each
  // rest pass overlaps the next iteration's round 0 (pend[1] starts empty).  pend[q & 1] is 0 and winm[q & 1]
  // 0x7f7f7f7f when launch q starts: reset by the finish kernel that last used them.
  int q2 = 0;
};
