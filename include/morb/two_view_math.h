// Scalar pieces of TwoViewReconstruction (reference src/TwoViewReconstruction.cc) shared by the kernel (csrc/two_view.hip), the C++
// adapter (include/morb/TwoViewReconstruction.h), the CPU oracle and the native checks: plain C++ that compiles for the host and for
// the device.
//   * TwoViewStat / TwoViewFStat: the rows morb_two_view_reconstruction_batch writes to d_stats / d_fstats, index by index;
//   * TwoViewFail: why a problem returned false (d_stats[TV_S_FAIL]);
//   * tv_sample8: one iteration's minimal set (:82-95), swap-with-back sampling without the vector (RandomInt is ransac_math.h's);
//   * tv_min_good: nMinGood of ReconstructF (:510);  tv_parallax_deg: acos(c) * 180 / CV_PI as the reference's types evaluate it (:875).
#pragma once
#include <cstdint>

#include "ransac_math.h"

#if defined(__HIPCC__)
#define MORB_TV_FN __host__ __device__ __forceinline__
#define MORB_TV_UNROLL _Pragma("unroll")
#else
#define MORB_TV_FN inline
#define MORB_TV_UNROLL
#endif

// X(name): one list for the enum, for the Python front's tuple (optimizer.TWO_VIEW_STATS) and for the program that prints both
#define MORB_TV_STATS(X)                                                                                                    \
  X(N)          /* mvMatches12.size() */                                                                                    \
  X(MODEL)      /* 0 none (N < 8, or SH + SF == 0), 1 ReconstructH, 2 ReconstructF */                                       \
  X(BEST_IT_H)  /* the iteration FindHomography kept, -1 when no score exceeded 0 */                                        \
  X(BEST_IT_F)  /* ... FindFundamental */                                                                                   \
  X(NINLIERS)   /* set bits of the chosen model's best mask (N of ReconstructH / ReconstructF) */                           \
  X(NHYP)       /* motion hypotheses checked: 0, 4 (F) or 8 (H) */                                                          \
  X(CHOSEN)     /* the hypothesis returned, -1 when none */                                                                 \
  X(FAIL)       /* TwoViewFail */                                                                                           \
  X(NGOOD0) X(NGOOD1) X(NGOOD2) X(NGOOD3) X(NGOOD4) X(NGOOD5) X(NGOOD6) X(NGOOD7)   /* CheckRT's return, per hypothesis */

#define MORB_TV_FSTATS(X)                                                                  \
  X(SH) X(SF) X(RH)                                                                        \
  X(H21_0) X(H21_1) X(H21_2) X(H21_3) X(H21_4) X(H21_5) X(H21_6) X(H21_7) X(H21_8)   /* the best H21, row-major */ \
  X(F21_0) X(F21_1) X(F21_2) X(F21_3) X(F21_4) X(F21_5) X(F21_6) X(F21_7) X(F21_8)   /* the best F21, row-major */ \
  X(PARALLAX0) X(PARALLAX1) X(PARALLAX2) X(PARALLAX3) X(PARALLAX4) X(PARALLAX5) X(PARALLAX6) X(PARALLAX7)

namespace morbtv {

#define MORB_TV_X(n) TV_S_##n,
enum TwoViewStat { MORB_TV_STATS(MORB_TV_X) TV_STATS_LEN };
#undef MORB_TV_X
#define MORB_TV_X(n) TV_F_##n,
enum TwoViewFStat { MORB_TV_FSTATS(MORB_TV_X) TV_FSTATS_LEN };
#undef MORB_TV_X

enum TwoViewFail {
  TV_FAIL_NONE = 0,
  TV_FAIL_FEW_MATCHES = 1,    // fewer than 8 matches: no iteration (undefined in the reference)
  TV_FAIL_ZERO_SCORE = 2,     // SH + SF == 0 (:112)
  TV_FAIL_DEGENERATE_H = 3,   // d1 / d2 < 1.00001 || d2 / d3 < 1.00001 (:590)
  TV_FAIL_AMBIGUOUS = 4,      // maxGood < nMinGood || nsimilar > 1 (:520); the count conditions of :712-713
  TV_FAIL_PARALLAX = 5,       // the winner's parallax below minParallax (:526-556; :712 with the count conditions met)
};

constexpr int TV_SET = 8;                 // points per minimal set
constexpr int TV_MIN_TRIANGULATED = 50;   // Reconstruct's last argument to ReconstructH / ReconstructF (:123, :128)
constexpr float TV_MIN_PARALLAX = 1.0f;   // (:115)
constexpr int TV_PARALLAX_RANK = 50;      // vCosParallax[min(50, size - 1)] of the sorted list (:874)

// vAvailableIndices = 0 .. N-1; eight times: randi = RandomInt(0, size - 1), take [randi], move the back there, pop (:83-94).
// Without the vector: the value at a position is the latest one moved there, or the position itself.  N >= 8.
MORB_TV_FN void tv_sample8(const int* r, int N, int* idx) {
  int pos[TV_SET], val[TV_SET];
  MORB_TV_UNROLL
  for (int i = 0; i < TV_SET; ++i) {
    const int size = N - i;
    const int randi = morbransac::random_int(r[i], size);
    int v = randi, bv = size - 1;
    MORB_TV_UNROLL
    for (int k = 0; k < TV_SET; ++k) {
      if (k < i) {
        if (pos[k] == randi) v = val[k];
        if (pos[k] == size - 1) bv = val[k];
      }
    }
    idx[i] = v;
    pos[i] = randi;
    val[i] = bv;
  }
}

// int nMinGood = max(static_cast<int>(0.9 * N), minTriangulated): a double product, truncated
MORB_TV_FN int tv_min_good(int nInliers, int minTriangulated) {
  const int a = (int)(0.9 * (double)nInliers);
  return a > minTriangulated ? a : minTriangulated;
}

// parallax = acos(c) * 180 / CV_PI with c a float: acosf, a float product, a double quotient rounded to float
MORB_TV_FN float tv_parallax_deg(float acosOfCos) { return (float)((double)(acosOfCos * 180.f) / 3.1415926535897932384626433832795); }

}  // namespace morbtv
