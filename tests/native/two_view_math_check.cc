// Stand-alone host check of include/morb/two_view_math.h and, through tv_sample8, of ransac_math.h's random_int (its own main;
// tests/test_two_view_cpu.py builds it with -fsanitize=address,undefined and runs it): tv_sample8 against the reference's vector form
// (:83-94, with DUtils::Random::RandomInt's double expression) over many sizes and rand() values, tv_min_good, tv_parallax_deg, and the
// two enums, which it prints by name for the test to compare with the Python front's tuples.  (random_int alone against that
// expression, over these sizes and rand() values too: test_random_int_matches_dutils of tests/test_sim3_solver_cpu.py.)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "morb/two_view_math.h"

using namespace morbtv;

int main() {
  int bad = 0;
  unsigned long long s = 88172645463325252ull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (int)(s >> 33); };   // 31 bits, like rand()
  for (int N = 8; N <= 2000; N = N < 40 ? N + 1 : N * 3 / 2) {
    for (int rep = 0; rep < 200; ++rep) {
      int r[TV_SET], idx[TV_SET];
      for (int& v : r) v = rep == 0 ? 0 : (rep == 1 ? 2147483647 : next());
      tv_sample8(r, N, idx);
      std::vector<size_t> avail;
      for (int i = 0; i < N; ++i) avail.push_back(i);
      for (int j = 0; j < TV_SET; ++j) {
        const int d = (int)avail.size();
        const int randi = int(((double)r[j] / ((double)2147483647 + 1.0)) * d);
        if ((int)avail[randi] != idx[j]) { if (bad++ < 5) printf("sample N %d rep %d j %d: %d != %d\n", N, rep, j, idx[j], (int)avail[randi]); }
        avail[randi] = avail.back();
        avail.pop_back();
      }
    }
  }
  for (int n = 0; n < 3000; ++n) {
    const int want = std::max(static_cast<int>(0.9 * n), 50);
    if (tv_min_good(n, TV_MIN_TRIANGULATED) != want) { if (bad++ < 5) printf("min_good(%d)\n", n); }
  }
  for (int k = 0; k <= 1000; ++k) {
    const float c = 1.f - k * 1e-5f;
    float parallax = acosf(c) * 180 / 3.1415926535897932384626433832795;   // the reference's expression (:875) with CV_PI's digits
    if (parallax != tv_parallax_deg(acosf(c))) { if (bad++ < 5) printf("parallax(%a)\n", c); }
  }
#define P(n) printf("stat %s %d\n", #n, (int)TV_S_##n);
  MORB_TV_STATS(P)
#undef P
#define P(n) printf("fstat %s %d\n", #n, (int)TV_F_##n);
  MORB_TV_FSTATS(P)
#undef P
  printf("len %d %d\n", (int)TV_STATS_LEN, (int)TV_FSTATS_LEN);
  printf("fail %d %d %d %d %d %d\n", TV_FAIL_NONE, TV_FAIL_FEW_MATCHES, TV_FAIL_ZERO_SCORE, TV_FAIL_DEGENERATE_H, TV_FAIL_AMBIGUOUS, TV_FAIL_PARALLAX);
  printf("mismatches %d\n", bad);
  return bad != 0;
}
