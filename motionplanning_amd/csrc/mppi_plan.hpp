// mppi_plan.hpp — the launch shape of mppi_plan_kernel (mppi.hip) as a function of the call's integers: lanes per
// rollout, block size, blocks per scene, the lean instance, and the map of the dynamic LDS.  No HIP type, so the
// shape runs on its own under host sanitizers (tools/mppi_plan_check.cpp).
#pragma once
#include <cstddef>

// Dynamic LDS budgets per block (160 KiB per CU on gfx950).  The plan kernel's static LDS is at most
// 13,096 B (BT 512, LPR 2: sh_q 8 KiB, sh_e 2 KiB, the atan rows and bounds 2,704 B, the rest < 200 B), so one block
// fits beside 146 KiB, and at most 7,976 B at BT 256, so two blocks fit beside 70 KiB each.
constexpr size_t kMaxLds = 146 * 1024;
constexpr size_t kCoLds = 70 * 1024;    // budget that keeps two blocks co-resident per CU
// The occupancy grid's LDS image (staged 16 bytes per lane) starts at the first 16-byte line of its region plus
// the scene's offset within a line of the caller's buffer: up to 15 + 15 bytes into the region.
constexpr int kGridPad = 32;

struct MppiShapeIn {
  int S, K, H, n_obs, gnx, gny;
  int in_flight;      // calls on other contexts sharing the SIMDs with this one (>= 1, this call included)
  bool device_noise;  // Philox draws in the kernel (else the caller's noise)
  bool ctrl_cost;
  bool grid;          // a grid pointer is present
  bool collect;       // both coll_traj and coll_ctrl are present
  int force_lpr;      // (test hook) 1 / 2 forces the layout, anything else leaves the choice to the shape
  bool allow_lean;    // (test hook) false forces the generic instance and its LDS choice
};

struct MppiShape {
  int LPR, BT, RPB;  // lanes per rollout, threads per block, rollouts per block
  int nb, pstride;   // blocks per scene, doubles per block partial
  bool lean;         // the lean instance (mppi_plan_kernel<.., LEAN>)
  // offsets in doubles into the dynamic LDS, as PlanArgs carries them; -1: that region stays in HBM
  int lds_unom, lds_cq, lds_obs, lds_grid, lds_ctrl, lds_part;
  size_t lds_words;  // dynamic LDS in doubles; the call is refused when it exceeds kMaxLds bytes
};

inline MppiShape mppi_plan_shape(const MppiShapeIn& in) {
  const int S = in.S, K = in.K, H = in.H;
  MppiShape P;
  // 8-wave blocks once the launch fills every CU with one (the dispatcher then places
  // exactly two waves per SIMD; with 4-wave blocks, two per CU, it can stack 3 + 1 and
  // the slowest SIMD sets the end time), else 4-wave blocks for more CUs at small S.
  // One rollout per lane once that gives every SIMD two waves (S*K >= 2 x 256 CUs x 4 SIMDs x
  // 64 lanes).  Measured (cfg2, K=8192, H=50): 16 scenes, LPR 1 (2 waves/SIMD, the tire chains
  // interleaved in a lane, costs evaluated once) 0.536 ms vs LPR 2 (4 waves/SIMD) 0.703 ms;
  // 8 scenes, LPR 1 (1 wave/SIMD) 0.384 ms vs LPR 2 (2 waves/SIMD) 0.375 ms: a lone wave
  // cannot cover the fp64 dependency latency.
  // With n calls in flight on n contexts (calls_in_flight), the other calls' waves fill the SIMDs too, so the
  // rollouts of all of them count: 8 scenes, two calls alternating over two contexts, LPR 1 1.17-1.19e10
  // rollout-steps/s against LPR 2 1.08-1.10e10; three calls 1.31e10 (r06y, bench driver arguments).
  // A forced layout gives the same bits either way (tests/test_gpu_mppi_lane.py), only the launch shape changes.
  P.LPR = in.force_lpr == 1 || in.force_lpr == 2 ? in.force_lpr : ((size_t)S * K * in.in_flight >= 131072 ? 1 : 2);
  // Single scene (64 blocks): BT 128 (2 waves per CU on 128 CUs) 0.278 ms vs BT 256 (4 waves, one per
  // SIMD, on 64 CUs) 0.242 ms -- a CU's four SIMDs each holding one wave beat half-filled CUs.
  P.BT = P.LPR == 1 ? ((size_t)S * ((K + 511) / 512) >= 256 ? 512 : 256)
                    : ((size_t)S * ((K + 255) / 256) >= 256 ? 512 : 256);
  P.RPB = P.BT / P.LPR;
  P.nb = (K + P.RPB - 1) / P.RPB;
  P.pstride = 4 + 2 * H;
  // dynamic LDS: [phase-2: 2H + nb] [unom: 2H] [cq: 2H] [obs: 3 n_obs] [grid bytes] [control lists | staged partials]
  size_t off = 2 * (size_t)H + P.nb;
  P.lds_unom = (int)off;
  off += 2 * (size_t)H;
  P.lds_cq = (int)off;
  off += 2 * (size_t)H;
  P.lds_obs = (int)off;
  off += 3 * (size_t)in.n_obs;
  const size_t gbytes = (size_t)in.gnx * in.gny;
  P.lds_grid = -1;
  if (in.gnx > 0 && off * 8 + gbytes + kGridPad <= 48 * 1024) {
    P.lds_grid = (int)off;
    off += (gbytes + kGridPad + 7) / 8;
  }
  // Control lists / staged partials in LDS only while two blocks still fit per CU
  // (multi-scene launches need every block co-resident); otherwise the HBM path.
  const size_t ctrl_words = (size_t)P.RPB * (2 * (size_t)H + 1), part_words = (size_t)P.nb * P.pstride;
  P.lds_ctrl = P.lds_part = -1;
  const bool many = (size_t)S * P.nb > 256;  // more blocks than CUs: keep two per CU resident
  const size_t budget = many ? kCoLds : kMaxLds;
  // The lean instance for the common collecting call: one rollout per lane, device noise, no circle obstacles,
  // the grid in LDS, the control cost on, both collection outputs, and K < 2^27 (32-bit lane offsets of 16 K
  // bytes).  Such a call keeps no control lists in LDS: they go to coll_ctrl anyway, and the block partial sums
  // them from there over the same rollouts in the same order (the LDS path only adds the inactive lanes' 0.0 * u).
  P.lean = in.allow_lean && P.LPR == 1 && (P.BT == 256 || P.BT == 512) && in.device_noise && in.n_obs == 0 &&
           in.grid && P.lds_grid >= 0 && in.ctrl_cost && in.collect && K < (1 << 27);
  const size_t both_words = ctrl_words > part_words ? ctrl_words : part_words;
  if (P.lean) {
    if ((off + part_words) * 8 <= budget) {
      P.lds_part = (int)off;
      off += part_words;
    }
  } else if ((off + both_words) * 8 <= budget) {
    P.lds_ctrl = P.lds_part = (int)off;
    off += both_words;
  } else if ((off + part_words) * 8 <= budget) {
    P.lds_part = (int)off;
    off += part_words;
  }
  P.lds_words = off;
  return P;
}
