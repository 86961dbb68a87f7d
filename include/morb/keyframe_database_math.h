// Scalar pieces of KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc:579-814)
// and of DBoW2's L1 score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), shared by the kernels of csrc/keyframe_database.hip, the
// C++ adapter and the CPU oracle: plain C++ that compiles for the host and for the device.
//   * l1_term: what one common word adds to the score's sum;
//   * l1_score: the sum's value as the float the database stores;
//   * min_common_words: the count a keyframe must EXCEED to be scored (:623, :743);
//   * retained: the relocalisation test against 0.75 of the best accumulated score (:795-803);
//   * acc_sort_key / first_word_key: the two orderings as unsigned keys (ascending key = list order).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MORB_KFDB_FN __host__ __device__ __forceinline__
#else
#define MORB_KFDB_FN inline
#endif

namespace morbkfdb {

// flag bits of d_flags
enum { KFDB_BAD = 1, KFDB_MAP_BAD = 2 };

// score += fabs(vi - wi) - fabs(vi) - fabs(wi)  (ScoringObject.cpp:41); no product, so nothing here can contract
MORB_KFDB_FN double l1_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }

// score = -score / 2.0 (:65), narrowed by `float si = mpVoc->score(..)` (KeyFrameDatabase.cc:637, :757)
MORB_KFDB_FN float l1_score(double sum) { return (float)(-sum / 2.0); }

// int minCommonWords = maxCommonWords * 0.8f: the int is converted to float, the product is a float, the conversion truncates
MORB_KFDB_FN int min_common_words(int maxCommonWords) { return (int)((float)maxCommonWords * 0.8f); }

// si > 0.75f * bestAccScore
MORB_KFDB_FN bool retained(float accScore, float bestAccScore) { return accScore > 0.75f * bestAccScore; }

// list::sort(compFirst), a stable sort by accScore descending, as an ascending sort of unique keys: the high word falls as the
// float rises (the usual order-preserving map of the bit pattern, -0 read as +0 because compFirst sees them equal), the low word is
// the entry's position before the sort.  A NaN accScore has no place in the reference's order either.
MORB_KFDB_FN uint64_t acc_sort_key(float accScore, uint32_t position) {
  if (accScore == 0.0f) accScore = 0.0f;
  uint32_t u;
  memcpy(&u, &accScore, 4);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // rises with the float
  return ((uint64_t)(~u) << 32) | position;
}

// lKFsSharingWords' order: (rank in the query of the first common word, add rank)
MORB_KFDB_FN uint64_t first_word_key(int firstRank, int dbRank) { return ((uint64_t)(uint32_t)firstRank << 32) | (uint32_t)dbRank; }

}  // namespace morbkfdb
