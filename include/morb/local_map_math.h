// The order-defining integer logic of Tracking::UpdateLocalMap (reference src/Tracking.cc:3184-3358), shared by the kernels of
// csrc/local_map.hip, the CPU oracle's cross-check and a stand-alone sanitizer program: plain C++ that compiles for the host and for
// the device.  Nothing here is floating point.
//   * second_stage: the neighbour / child / parent walk over the first-stage keyframes (:3289-3335);
//   * temporal_tail: the inertial walk along mPrevKF (:3338-3352);
//   * sequence_key / its two parts: where UpdateLocalPoints (:3193-3218) meets a point, as one unsigned number (ascending key =
//     list order), and the word a listed point's key is replaced with.
// Both walks see the map through a caller's object `g` with
//   bool stamped(int kf)    mnTrackReferenceForFrame == mCurrentFrame.mnId
//   bool bad(int kf)        isBad()
//   void add(int kf)        push_back + stamp (the caller counts: the walks keep the size themselves)
//   int  first(int i)       entry i of the first stage's list
// and plain tables of rows (-1 = NULL); a row outside [0, nkf) is skipped like a NULL.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MORB_LM_FN __host__ __device__ __forceinline__
#else
#define MORB_LM_FN inline
#endif

namespace morblm {

enum { LM_BAD = 1 };                 // bit 0 of d_kfFlags / d_mpFlags: isBad()
enum { LM_OVERFLOW_KF = 1, LM_OVERFLOW_MP = 2 };   // bits of d_overflow
enum {
  LM_SIZE_LIMIT = 80,    // `mvpLocalKeyFrames.size() > 80` (:3293) and `< 80` (:3340)
  LM_TAIL_STEPS = 20,    // Nd (:3343)
  // The longest list either walk can touch: the second stage runs only below the limit and adds at most three per entry, the tail
  // only below it and adds at most LM_TAIL_STEPS.
  LM_WALK_MAX = LM_SIZE_LIMIT + 3 + LM_TAIL_STEPS,
  // The kernels take the keyframes (in d_kfOrder order, then in reverse list order) LM_WINDOW positions at a time, one per thread of
  // the query's workgroup; more keyframes than that take another trip of the same loop.  Host and device share it: the tests cross it.
  LM_WINDOW = 256,
};

MORB_LM_FN bool row_ok(int kf, int nkf) { return kf >= 0 && kf < nkf; }

// :3289-3335.  n1 = the first stage's length; returns the list's size behind the loop.
template <class G>
MORB_LM_FN int second_stage(G& g, int n1, int nkf, const int* covis, int ncovis, const int* childStart, const int* child,
                            const int* parent) {
  int size = n1;
  for (int i = 0; i < n1; ++i) {
    if (size > LM_SIZE_LIMIT) break;   // additions count (:3293)
    const int kf = g.first(i);
    for (int j = 0; j < ncovis; ++j) {   // vNeighs, in its order
      const int nb = covis[(int64_t)kf * ncovis + j];
      if (!row_ok(nb, nkf)) continue;
      if (!g.bad(nb) && !g.stamped(nb)) { g.add(nb); ++size; break; }
    }
    if (childStart) {
      for (int j = childStart[kf]; j < childStart[kf + 1]; ++j) {   // spChilds, in the set's order
        const int c = child[j];
        if (!row_ok(c, nkf)) continue;
        if (!g.bad(c) && !g.stamped(c)) { g.add(c); ++size; break; }
      }
    }
    const int p = parent ? parent[kf] : -1;
    if (row_ok(p, nkf) && !g.stamped(p)) {   // no isBad() test, and the break leaves the KEYFRAME loop (:3332)
      g.add(p); ++size;
      break;
    }
  }
  return size;
}

// :3338-3352.  `size` = the list's size on entry; returns it behind the walk.  A stamped keyframe is not advanced from (:3346-3350), so the
// remaining steps add nothing; there is no size test inside.
template <class G>
MORB_LM_FN int temporal_tail(G& g, int size, int inertial, int lastKf, int nkf, const int* prevKf) {
  if (!inertial || size >= LM_SIZE_LIMIT) return size;
  int kf = lastKf;
  for (int i = 0; i < LM_TAIL_STEPS; ++i) {
    if (!row_ok(kf, nkf)) break;
    if (g.stamped(kf)) break;   // every later step would meet the same stamped keyframe
    g.add(kf); ++size;
    kf = prevKf ? prevKf[kf] : -1;
  }
  return size;
}

// UpdateLocalPoints meets a point first at (keyframe at `reversePos` from the list's END, feature `idx`): the least key wins.  The
// callers keep nkf * kfCap below 2^31, so a key never has LM_LISTED set.
MORB_LM_FN uint32_t sequence_key(int reversePos, int kfCap, int idx) { return (uint32_t)reversePos * (uint32_t)kfCap + (uint32_t)idx; }

// the word of a point nobody met, and of a point that went into the list at `position`
enum : uint32_t { LM_KEY_NONE = 0xffffffffu, LM_LISTED = 0x80000000u };
MORB_LM_FN uint32_t listed_word(int position) { return LM_LISTED | (uint32_t)position; }
MORB_LM_FN int listed_position(uint32_t word) { return (word != LM_KEY_NONE && (word & LM_LISTED)) ? (int)(word & ~LM_LISTED) : -1; }

}  // namespace morblm
