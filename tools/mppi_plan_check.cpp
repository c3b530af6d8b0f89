// Stand-alone check of the MPPI plan kernel's launch shape (motionplanning_amd/csrc/mppi_plan.hpp):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mppi_plan_check.cpp -o plan_check
// For every input of the sweep: each field of the shape equals the expressions plan_launch used before the shape
// was a function (restated here in their former int arithmetic); the LDS regions tile [0, total) in order without
// gap or overlap; then a buffer of exactly `total` doubles is allocated and every region is written end to end
// with a tag of its own (so the sanitizer sees any step outside the buffer) and read back (so an overlap shows as
// a wrong tag).  The sweep and two inputs between its values must reach every kind of shape (kinds_expected
// below), and the two bench shapes are printed and asserted.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "../motionplanning_amd/csrc/mppi_plan.hpp"

static int fails = 0;
static MppiShapeIn cur;
#define CHECK(c)                                                                                              \
  do {                                                                                                        \
    if (!(c)) {                                                                                               \
      std::printf("FAIL line %d: %s (S %d K %d H %d n_obs %d grid %dx%d in_flight %d noise %d cc %d coll %d " \
                  "lpr %d lean %d)\n", __LINE__, #c, cur.S, cur.K, cur.H, cur.n_obs, cur.gnx, cur.gny,        \
                  cur.in_flight, cur.device_noise, cur.ctrl_cost, cur.collect, cur.force_lpr, cur.allow_lean);\
      fails++;                                                                                                \
    }                                                                                                         \
  } while (0)

enum Placement { BOTH, PART, NONE };  // control lists + partials in LDS, partials only, neither
// (LPR, BT, grid in LDS, lean, placement, more blocks than CUs, total <= kMaxLds)
using Kind = std::tuple<int, int, bool, bool, int, bool, bool>;

// The kinds the policy can produce.  The last region is placed only within its budget (<= kMaxLds), and the grid
// goes to LDS only while it ends within 48 KiB, so a shape beyond kMaxLds has neither; lean needs LPR 1 and the
// grid in LDS and never holds the control lists.  Everything else combines freely: 2 x 2 x 2 x (2 x 3 + 1) generic
// kinds and 2 x 2 x 2 lean ones, 64 in all.
static std::set<Kind> kinds_expected() {
  std::set<Kind> E;
  for (int lpr : {1, 2})
    for (int bt : {256, 512})
      for (bool many : {false, true}) {
        for (int pl : {BOTH, PART, NONE}) {
          E.insert({lpr, bt, false, false, pl, many, true});
          E.insert({lpr, bt, true, false, pl, many, true});
        }
        E.insert({lpr, bt, false, false, NONE, many, false});
        if (lpr == 1)
          for (int pl : {PART, NONE}) E.insert({lpr, bt, true, true, pl, many, true});
      }
  return E;
}

static std::set<Kind> seen;

static void check(const MppiShapeIn& in, const void* grid, const void* coll_traj, const void* coll_ctrl) {
  cur = in;
  const MppiShape P = mppi_plan_shape(in);
  // ---- the former expressions of plan_launch, restated (D = the device parameters, A = PlanArgs)
  const int S = in.S, K = in.K, H = in.H, D_n_obs = in.n_obs, D_gnx = in.gnx, D_gny = in.gny;
  const int lpr_env = in.force_lpr;
  const int LPR = lpr_env == 1 || lpr_env == 2 ? lpr_env : ((size_t)S * K * in.in_flight >= 131072 ? 1 : 2);
  const int BT = LPR == 1 ? ((size_t)S * ((K + 511) / 512) >= 256 ? 512 : 256)
                          : ((size_t)S * ((K + 255) / 256) >= 256 ? 512 : 256);
  const int RPBh = BT / LPR;
  const int nb = (K + RPBh - 1) / RPBh;
  const int pstride = 4 + 2 * H;
  const void* A_grid = D_gnx > 0 ? grid : nullptr;
  const bool A_inline_noise = in.device_noise;
  int off = 2 * H + nb;
  const int lds_unom = off;
  off += 2 * H;
  const int lds_cq = off;
  off += 2 * H;
  const int lds_obs = off;
  off += 3 * D_n_obs;
  const size_t gbytes = (size_t)D_gnx * D_gny;
  int lds_grid = -1;
  if (D_gnx > 0 && (size_t)off * 8 + gbytes + 32 <= 48 * 1024) {
    lds_grid = off;
    off += (int)((gbytes + 32 + 7) / 8);
  }
  const int ctrl_words = RPBh * (2 * H + 1), part_words = nb * pstride;
  int lds_ctrl = -1, lds_part = -1;
  const bool many = (size_t)S * nb > 256;
  const size_t budget = many ? (size_t)70 * 1024 : (size_t)146 * 1024;
  const bool lean = in.allow_lean && LPR == 1 && (BT == 256 || BT == 512) && A_inline_noise && D_n_obs == 0 && A_grid &&
                    lds_grid >= 0 && in.ctrl_cost && coll_traj && coll_ctrl && K < (1 << 27);
  if (lean) {
    if ((size_t)(off + part_words) * 8 <= budget) {
      lds_part = off;
      off += part_words;
    }
  } else if ((size_t)(off + (ctrl_words > part_words ? ctrl_words : part_words)) * 8 <= budget) {
    lds_ctrl = lds_part = off;
    off += ctrl_words > part_words ? ctrl_words : part_words;
  } else if ((size_t)(off + part_words) * 8 <= budget) {
    lds_part = off;
    off += part_words;
  }
  // ---- 1. field for field
  CHECK(P.LPR == LPR && P.BT == BT && P.RPB == RPBh && P.nb == nb && P.pstride == pstride && P.lean == lean);
  CHECK(P.lds_unom == lds_unom && P.lds_cq == lds_cq && P.lds_obs == lds_obs && P.lds_grid == lds_grid);
  CHECK(P.lds_ctrl == lds_ctrl && P.lds_part == lds_part && P.lds_words == (size_t)off);
  // ---- 2. the regions, in order, tile [0, total)
  struct Region { long long at; size_t n; };
  std::vector<Region> R = {{0, (size_t)(2 * H + P.nb)}, {P.lds_unom, (size_t)2 * H}, {P.lds_cq, (size_t)2 * H},
                           {P.lds_obs, (size_t)3 * in.n_obs}};
  if (P.lds_grid >= 0) R.push_back({P.lds_grid, (gbytes + kGridPad + 7) / 8});
  const size_t cw = (size_t)P.RPB * (2 * H + 1), pw = (size_t)P.nb * P.pstride;
  if (P.lds_ctrl >= 0) {
    CHECK(P.lds_ctrl == P.lds_part && !P.lean);  // one region serves both, first the lists, then the partials
    R.push_back({P.lds_ctrl, cw > pw ? cw : pw});
  } else if (P.lds_part >= 0) {
    R.push_back({P.lds_part, pw});
  }
  size_t end = 0;
  for (const Region& r : R) {
    CHECK(r.at >= 0 && (size_t)r.at == end);
    end += r.n;
  }
  CHECK(end == P.lds_words);
  // ---- 3. written end to end into a buffer of exactly `total` doubles, and read back
  double* buf = (double*)std::malloc(sizeof(double) * (P.lds_words ? P.lds_words : 1));
  for (size_t r = 0; r < R.size(); r++)
    for (size_t i = 0; i < R[r].n; i++) buf[R[r].at + (long long)i] = (double)(r + 1);
  for (size_t r = 0; r < R.size(); r++)
    for (size_t i = 0; i < R[r].n; i++) CHECK(buf[R[r].at + (long long)i] == (double)(r + 1));
  std::free(buf);
  const int pl = P.lds_ctrl >= 0 ? BOTH : P.lds_part >= 0 ? PART : NONE;
  seen.insert({P.LPR, P.BT, P.lds_grid >= 0, P.lean, pl, (size_t)S * P.nb > 256, P.lds_words * 8 <= kMaxLds});
}

// a shape bench.py's headline runs: K 8192, H 50, a 100 x 100 grid, device noise, the full collection
static void bench_shape(int S, int in_flight, int BT, int nb, size_t bytes) {
  const MppiShapeIn in = {S, 8192, 50, 0, 100, 100, in_flight, true, true, true, true, 0, true};
  cur = in;
  const MppiShape P = mppi_plan_shape(in);
  std::printf("S %d, in_flight %d: LPR %d, BT %d, nb %d, %s, partials %s, %zu B\n", S, in_flight, P.LPR, P.BT, P.nb,
              P.lean ? "lean" : "generic", P.lds_part >= 0 ? "in LDS" : "in HBM", P.lds_words * 8);
  CHECK(P.LPR == 1 && P.BT == BT && P.nb == nb && P.lean && P.lds_part >= 0 && P.lds_ctrl < 0 && P.lds_grid >= 0);
  CHECK(P.lds_words * 8 == bytes);
}

int main() {
  static const char dummy = 0;  // stands for a pointer that is present
  long long n = 0;
  for (int S : {1, 2, 8, 16, 64, 300})
    for (int K : {1, 64, 320, 1500, 8192, 40000, 200000})
      for (int H : {1, 6, 20, 50, 200, 1000, 4096})
        for (int n_obs : {0, 3, 2000})
          for (int side : {0, 11, 100, 300})
            for (int in_flight : {1, 2, 3})
              for (bool noise : {true, false})
                for (bool cc : {true, false})
                  for (bool coll : {true, false})
                    for (int lpr : {0, 1, 2})
                      for (bool lean : {true, false}) {
                        const MppiShapeIn in = {S, K, H, n_obs, side, side, in_flight, noise, cc, side > 0, coll, lpr, lean};
                        check(in, side > 0 ? &dummy : nullptr, coll ? &dummy : nullptr, coll ? &dummy : nullptr);
                        n++;
                      }
  const size_t in_sweep = seen.size();
  // Two kinds lie between the sweep's values: lane pairs in 256-thread blocks (S * ceil(K / 256) < 256), more
  // blocks than CUs (S * ceil(K / 128) > 256) and the control lists too large for the co-residency budget while
  // the partials fit.  K = 1500 needs 22 <= S <= 42 for that, K = 320 has no such S.
  for (int side : {0, 11}) {
    const MppiShapeIn in = {32, 1500, 50, 0, side, side, 1, true, true, side > 0, false, 0, true};
    check(in, side > 0 ? &dummy : nullptr, nullptr, nullptr);
  }
  const std::set<Kind> E = kinds_expected();
  int missing = 0, extra = 0;
  static const char* pls[] = {"ctrl+part", "part", "none"};
  auto show = [&](const char* what, const Kind& k) {
    std::printf("%s: LPR %d BT %d grid-in-LDS %d lean %d %s many %d fits %d\n", what, std::get<0>(k), std::get<1>(k),
                std::get<2>(k), std::get<3>(k), pls[std::get<4>(k)], std::get<5>(k), std::get<6>(k));
  };
  for (const Kind& k : E)
    if (!seen.count(k)) missing++, show("not reached", k);
  for (const Kind& k : seen)
    if (!E.count(k)) extra++, show("unexpected", k);
  bench_shape(64, 1, 512, 16, 25872);
  bench_shape(8, 2, 256, 32, 39312);
  std::printf("%lld inputs in the sweep: %zu kinds of shape; with the 2 inputs between its values %zu of %zu expected "
              "(%d not reached, %d unexpected); %d failures\n", n, in_sweep, seen.size(), E.size(), missing, extra, fails);
  return fails || missing || extra || in_sweep != 62;
}
