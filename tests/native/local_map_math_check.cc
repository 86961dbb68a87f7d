// Stand-alone check of include/morb/local_map_math.h, meant to be built with -fsanitize=address,undefined: the two walks on random
// keyframe graphs (bad rows, rows out of range, stamped probes, long first stages, missing tables) against a plain restatement with
// std::set and std::vector, the bound LM_WALK_MAX on every entry a walk reads or adds, and the sequence key's order and words.
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "morb/local_map_math.h"

using namespace morblm;

struct Graph {
  std::vector<int> stamp, list;
  std::vector<uint8_t> flags;
  int maxRead = -1;
  bool stamped(int kf) const { return stamp.at(kf) != 0; }
  bool bad(int kf) const { return (flags.at(kf) & LM_BAD) != 0; }
  int first(int i) { if (i > maxRead) maxRead = i; return list.at(i); }
  void add(int kf) { stamp.at(kf) = 1; list.push_back(kf); }
};

int main() {
  std::mt19937 rng(12345);
  long mismatches = 0, walks = 0, longest = 0;
  for (int trial = 0; trial < 4000; ++trial) {
    const int nkf = 1 + (int)(rng() % 140), ncovis = (int)(rng() % 6);
    auto pick = [&](int lo) { return lo + (int)(rng() % (unsigned)(nkf + 2 - lo)); };   // [lo, nkf + 1]: one value past the table
    std::vector<int> covis((size_t)nkf * ncovis), parent(nkf), prev(nkf), childStart(nkf + 1, 0), child;
    std::vector<uint8_t> flags(nkf);
    for (auto& c : covis) c = pick(-1);
    for (int k = 0; k < nkf; ++k) {
      parent[k] = rng() % 3 ? -1 : pick(-1);
      prev[k] = rng() % 8 ? k - 1 : pick(-1);
      flags[k] = rng() % 7 == 0;
      const int nc = (int)(rng() % 3);
      for (int j = 0; j < nc; ++j) child.push_back(pick(-1));
      childStart[k + 1] = (int)child.size();
    }
    const bool withChildren = rng() % 5 != 0, withParent = rng() % 5 != 0, withPrev = rng() % 5 != 0;
    const int inertial = (int)(rng() % 2), lastKf = pick(-1);
    const unsigned density = 1 + rng() % 4;
    Graph g;
    g.stamp.assign(nkf, 0);
    g.flags = flags;
    for (int k = 0; k < nkf; ++k)
      if (rng() % density == 0 && !flags[k]) g.add(k);
    const std::vector<int> first = g.list;
    const int n1 = (int)first.size();
    // the restatement
    std::vector<int> want = first;
    std::set<int> st(first.begin(), first.end());
    auto ok = [&](int k) { return k >= 0 && k < nkf; };
    for (int i = 0; i < n1; ++i) {
      if (want.size() > 80) break;
      const int kf = first[i];
      for (int j = 0; j < ncovis; ++j) {
        const int nb = covis[(size_t)kf * ncovis + j];
        if (ok(nb) && !flags[nb] && !st.count(nb)) { want.push_back(nb); st.insert(nb); break; }
      }
      if (withChildren)
        for (int j = childStart[kf]; j < childStart[kf + 1]; ++j) {
          const int c = child[j];
          if (ok(c) && !flags[c] && !st.count(c)) { want.push_back(c); st.insert(c); break; }
        }
      const int p = withParent ? parent[kf] : -1;
      if (ok(p) && !st.count(p)) { want.push_back(p); st.insert(p); break; }
    }
    const size_t afterSecond = want.size();
    if (inertial && want.size() < 80) {
      int kf = lastKf;
      for (int i = 0; i < 20; ++i) {
        if (!ok(kf)) break;
        if (!st.count(kf)) { want.push_back(kf); st.insert(kf); kf = withPrev ? prev[kf] : -1; }
      }
    }
    const int n2 = second_stage(g, n1, nkf, covis.data(), ncovis, withChildren ? childStart.data() : nullptr, child.data(),
                                withParent ? parent.data() : nullptr);
    if (n2 != (int)afterSecond || n2 != (int)g.list.size()) ++mismatches;
    const int n3 = temporal_tail(g, n2, inertial, lastKf, nkf, withPrev ? prev.data() : nullptr);
    if (n3 != (int)g.list.size() || g.list != want) ++mismatches;
    if (g.maxRead > LM_SIZE_LIMIT) ++mismatches;                               // first(i) only below the limit
    if (n3 > n1 && n3 > LM_WALK_MAX) ++mismatches;                             // a list the walks touched
    if (n3 > n1 && n3 > longest) longest = n3;
    ++walks;
  }
  // the sequence key orders (reverse position, feature index) lexicographically and never looks like a listed word
  for (int kfCap : {1, 7, 1200, 65536}) {
    uint32_t last = 0;
    bool firstKey = true;
    for (int rp = 0; rp < 40; ++rp)
      for (int idx : {0, 1, kfCap / 2, kfCap - 1}) {
        if (idx < 0 || idx >= kfCap) continue;
        const uint32_t k = sequence_key(rp, kfCap, idx);
        if (!firstKey && k < last) ++mismatches;
        if ((k & LM_LISTED) || listed_position(k) != -1) ++mismatches;
        last = k; firstKey = false;
      }
  }
  if (sequence_key(32767, 65536, 65535) != 0x7fffffffu) ++mismatches;         // the largest key the entry admits
  for (int pos : {0, 1, 255, 256, 1 << 20, 0x7ffffffe})
    if (listed_position(listed_word(pos)) != pos || listed_word(pos) == LM_KEY_NONE) ++mismatches;
  if (listed_position(LM_KEY_NONE) != -1) ++mismatches;
  std::printf("walks %ld, longest touched list %ld (LM_WALK_MAX %d), mismatches %ld\n", walks, longest, (int)LM_WALK_MAX, mismatches);
  return mismatches ? 1 : 0;
}
