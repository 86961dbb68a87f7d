// Host build of include/morb/keyframe_database_math.h (the scalar pieces the KeyFrameDatabase kernels share with the adapter and
// the CPU oracle) for tests/test_keyframe_database_cpu.py, a program of its own so that it can run under sanitizers: the word
// threshold against the reference's expression over every count to 2^20 and at the ends of int, the L1 term and score, the 0.75
// test, and the two sort keys against the comparisons they stand for.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "morb/keyframe_database_math.h"

int main() {
  using namespace morbkfdb;
  long bad = 0;
  for (int m = 0; m <= (1 << 20); ++m) {
    const int want = m * 0.8f;   // int minCommonWords = maxCommonWords * 0.8f
    bad += min_common_words(m) != want;
    bad += min_common_words(m) >= m && m > 0;   // the keyframe with the most common words is always scored
  }
  const int big[] = {16777217, 100000001, 2147483647};
  for (int m : big) { const int want = m * 0.8f; bad += min_common_words(m) != want; }
  bad += min_common_words(10) != 8 || min_common_words(5) != 4 || min_common_words(1) != 0;
  bad += l1_term(0.25, 0.75) != 0.5 - 0.25 - 0.75 || l1_term(0.5, 0.5) != -1.0 || l1_term(-0.5, 0.5) != 0.0;
  bad += l1_score(-2.0) != 1.0f || l1_score(0.0) != 0.0f || l1_score(-0.2) != (float)(0.2 / 2.0);
  bad += retained(0.75f, 1.0f) || !retained(0.7500001f, 1.0f) || retained(0.0f, 0.0f) || !retained(1e-30f, 0.0f);
  // acc_sort_key: key order = (accScore descending, position ascending); -0 and +0 tie
  std::srand(1);
  std::vector<float> v = {0.0f, -0.0f, 1.0f, -1.0f, 1e-38f, -1e-38f, 3.4e38f, -3.4e38f, 0.5f, 0.5f, 1.0000001f, INFINITY, -INFINITY};
  for (int k = 0; k < 200; ++k) v.push_back((float)(std::rand() % 2001 - 1000) / (float)(1 + std::rand() % 50));
  for (size_t i = 0; i < v.size(); ++i)
    for (size_t j = 0; j < v.size(); ++j) {
      const bool before = v[i] > v[j] || (v[i] == v[j] && i < j);
      bad += (acc_sort_key(v[i], (uint32_t)i) < acc_sort_key(v[j], (uint32_t)j)) != before;
    }
  // first_word_key: (first-word rank, add rank) lexicographic
  const int r[] = {0, 1, 2, 63, 64, 1199, 100000, 2147483647};
  for (int a : r) for (int b : r) for (int c : r) for (int d : r) {
    const bool before = a < c || (a == c && b < d);
    bad += (first_word_key(a, b) < first_word_key(c, d)) != before;
  }
  bad += KFDB_BAD != 1 || KFDB_MAP_BAD != 2;
  std::printf("mismatches %ld\n", bad);
  return bad != 0;
}
