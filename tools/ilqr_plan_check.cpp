// Stand-alone check of mp_ilqr_solve's search plan and workspace map (motionplanning_amd/csrc/ilqr_plan.hpp):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ilqr_plan_check.cpp -o plan_check
// For every shape and workspace cap: the plan equals the expressions ilqr_solve used before the plan was a
// function, the byte sizes likewise; then the two integer buffers are allocated at exactly those sizes, mapped,
// and every named region is written end to end with a tag of its own (so the sanitizer sees any step outside a
// buffer) and read back (so an overlap shows as a wrong tag).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../motionplanning_amd/csrc/ilqr_plan.hpp"

static int fails = 0;
#define CHECK(c)                                                                            \
  do {                                                                                      \
    if (!(c)) { std::printf("FAIL line %d: %s (B %zu N %zu cap %zu)\n", __LINE__, #c, B, N, cap); fails++; } \
  } while (0)

static void check(size_t B, size_t N, int ls_cap, size_t cap) {
  const int kG = 16;
  const IlqrPlan P = ilqr_plan(B, N, ls_cap, cap, kG);
  // the former expressions, restated
  auto fits = [&](size_t g) { return g * B * N * 48 <= ((size_t)1 << 30) && (!cap || g * B * N * 32 <= cap); };
  const int G = fits(16) ? 16 : fits(4) ? 4 : 1;
  const size_t T2 = G == 16 && ls_cap + 1 > G ? (size_t)(ls_cap + 1) : 0;
  CHECK(P.G == G && P.T2 == T2 && P.rest == (T2 > 0 && T2 * B * N * 48 <= ((size_t)8 << 30)));
  const IlqrWsBytes z = ilqr_ws_bytes(B, N, P);
  CHECK(z.k == sizeof(double) * 2 * (N - 1) * B && z.K == sizeof(double) * 8 * (N - 1) * B);
  CHECK(z.Xn == sizeof(double) * 4 * N * B * G && z.Un == sizeof(double) * 2 * N * B * G && z.J == sizeof(double) * B);
  CHECK(z.ints == sizeof(int) * (5 * B + 4) && z.pw == sizeof(int) * 8 * B);
  CHECK(z.Xs == sizeof(double) * 4 * N * B * T2 && z.Us == sizeof(double) * 2 * N * B * T2 && z.Jt == sizeof(double) * B * T2);
  for (int with_pw = 0; with_pw < 2; with_pw++) {
    int* ints = (int*)std::malloc(z.ints);
    int* pw = with_pw ? (int*)std::malloc(z.pw) : nullptr;
    IlqrWs W;
    ilqr_ws_map(&W, B, ints, pw);
    struct Region { int* p; size_t n; };
    std::vector<Region> R = {{W.active, B}, {W.iters, B}, {W.flags, B}, {W.list[0], 2 + B}, {W.list[1], 2 + B}};
    if (pw) {
      for (int q = 0; q < 2; q++) R.push_back({W.pend[q], B}), R.push_back({W.winm[q], B}), R.push_back({W.mstar[q], B});
      R.push_back({W.winm1, B}), R.push_back({W.mstar1, B});
      CHECK(W.pend[1] == W.pend[0] + B && W.winm[1] == W.winm[0] + B);  // IlqrSolve::begin sets each pair with one memset
    } else {
      CHECK(!W.pend[0] && !W.pend[1] && !W.winm[0] && !W.winm[1] && !W.mstar[0] && !W.mstar[1] && !W.winm1 && !W.mstar1);
    }
    for (size_t r = 0; r < R.size(); r++)
      for (size_t i = 0; i < R[r].n; i++) R[r].p[i] = (int)r + 1;
    size_t words = 0;
    for (size_t r = 0; r < R.size(); r++) {
      words += R[r].n;
      for (size_t i = 0; i < R[r].n; i++) CHECK(R[r].p[i] == (int)r + 1);
    }
    CHECK(words * sizeof(int) == z.ints + (pw ? z.pw : 0));  // the regions tile both buffers: no gap, no overlap
    std::free(ints);
    std::free(pw);
  }
}

int main() {
  const size_t Bs[] = {1, 24, 600, 2048, 4096, 100000, 300000}, Ns[] = {2, 20, 23, 100, 1000};
  const size_t caps[] = {0, (size_t)1 << 20, (size_t)230 << 10, 1024};
  int seen[17] = {0};
  for (size_t B : Bs)
    for (size_t N : Ns)
      for (size_t cap : caps)
        for (int ls_cap : {0, 15, 16, 27, 199}) {
          check(B, N, ls_cap, cap);
          seen[ilqr_plan(B, N, ls_cap, cap, 16).G]++;
        }
  std::printf("plans with G = 16: %d, G = 4: %d, G = 1: %d; %d failures\n", seen[16], seen[4], seen[1], fails);
  return fails || !seen[16] || !seen[4] || !seen[1];
}
