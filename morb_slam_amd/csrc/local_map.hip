// Tracking::UpdateLocalMap (reference src/Tracking.cc:3184-3358): UpdateLocalKeyFrames (:3220-3358) and UpdateLocalPoints (:3193-3218)
// batched over query frames on device-resident map tables, and the gather that fills the per-frame tables of isInFrustum and
// SearchByProjection(F, MapPoints) from the map-wide point arrays.  Integers only: two calls give the same bytes.
// Four launches per morb_update_local_map_batch on the caller's stream, no host synchronisation:
//   k_lm_init       grid-wide: zeroes the per-query keyframe words, sets the per-query point keys to "nobody met it".
//   k_lm_keyframes  one workgroup per query: bad frame points are cleared and the others vote (integer atomic adds, one word per
//                   keyframe ROW); the first stage takes the keyframes LM_WINDOW at a time in d_kfOrder order (a window's rows are
//                   found by a scan of d_kfOrder into LDS, so no inverse permutation is stored), compacts the voted, non-bad ones in
//                   that order and replaces each one's votes with its list position + 1: the stamp.  Thread 0 then runs
//                   local_map_math.h's two serial walks (at most LM_SIZE_LIMIT entries with ncovis + children probes each) on the
//                   same words.
//   k_lm_point_keys one wave per (query, keyframe row): a listed keyframe's features take atomicMin(key[point], sequence_key(reverse
//                   position, feature index)): the first meeting of UpdateLocalPoints wins, whatever the scheduling.
//   k_lm_points     one workgroup per query: the listed keyframes in reverse list order, LM_WINDOW at a time (found by a scan of the
//                   words), their rows in feature order; a feature whose key is its point's is kept, by ordered compaction; the
//                   point's key becomes its list position, which d_frameLocal then reads.
// Workspace (morb_matcher::localMap): nq * (nkf + nmp) ints, the words and the keys.
// Decisions taken here ("Local map"):
//   * a row outside its table (a point >= nmp, a keyframe >= nkf) is read as NULL everywhere, a count beyond its capacity as the capacity;
//   * the stamps a query starts from are clear: mnTrackReferenceForFrame of an earlier frame never equals this frame's id;
//   * with d_overflow's bit 1 set, a frame point listed at or beyond mpCap has d_frameLocal -1: the value indexes a table of mpCap rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "common.h"
#include "handles.h"
#include "morb_hip.h"
#include "morb/local_map_math.h"
#include "ransac_block.h"

namespace {

using namespace morblm;
using namespace morbransac;

constexpr int LM_NT = LM_WINDOW, LM_NW = LM_NT / 64;
static_assert(LM_NT % 64 == 0, "whole waves");
static_assert(LM_WALK_MAX <= LM_WINDOW, "the walks' list lives in one window of LDS");

struct MapArgs {
  int nkf, kfCap, ncovis, nmp;
  const int* kfMp;
  const int* kfCount;
  const uint8_t* kfFlags;
  const int* kfOrder;   // null: row order
  const int* covis;
  const int* childStart;
  const int* child;
  const int* parent;
  const int* prevKf;
  const int* mpObsStart;
  const int* mpObsKf;
  const uint8_t* mpFlags;
};

struct QueryArgs {
  int cap, inertial, kfOut, mpCap;
  int* frameMp;
  const int* count;
  const int* lastKf;
  int* localKf;
  int* nLocalKf;
  int* refKf;
  int* localMp;
  int* nLocalMp;
  int* frameLocal;   // may be null
  int* votes;        // may be null
  int* overflow;
};

__global__ __launch_bounds__(256) void k_lm_init(int* word, size_t nWord, uint32_t* key, size_t nKey) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nWord; i += stride) word[i] = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nKey; i += stride) key[i] = LM_KEY_NONE;
}

// what the walks see: the query's keyframe words (0 = unstamped, else list position + 1) and the head of its list in LDS
struct WalkGraph {
  int* word;
  const uint8_t* flags;
  int* head;       // LDS, LM_WINDOW entries: every entry the walks read or add lies below LM_WALK_MAX
  int* out;
  int kfOut, size;
  __device__ bool stamped(int kf) const { return word[kf] != 0; }
  __device__ bool bad(int kf) const { return (flags[kf] & LM_BAD) != 0; }
  __device__ int first(int i) const { return head[i]; }
  __device__ void add(int kf) {
    word[kf] = size + 1;
    if (size < LM_WINDOW) head[size] = kf;
    if (size < kfOut) out[size] = kf;
    ++size;
  }
};

// The rows of window [w, w + LM_WINDOW) of an order into sRow (-1 where none): sel(i) gives row i's position in the order, or -1.
// Starts and ends in a barrier.
template <class Sel>
__device__ __forceinline__ void window_rows(int* sRow, int w, int nkf, Sel sel) {
  __syncthreads();   // the window before is read
  sRow[threadIdx.x] = -1;
  __syncthreads();
  for (int i = threadIdx.x; i < nkf; i += LM_NT) {
    const int p = sel(i);
    if (p >= w && p < w + LM_WINDOW) sRow[p - w] = i;
  }
  __syncthreads();
}

__global__ __launch_bounds__(LM_NT) void k_lm_keyframes(MapArgs a, QueryArgs qa, int* words) {
  __shared__ int sRow[LM_WINDOW], sHead[LM_WINDOW], wcount[LM_NW], running, sMax, sRefOrder, sRef;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = blockIdx.x, nkf = a.nkf;
  int* word = words + (size_t)q * nkf;
  int* frameMp = qa.frameMp + (size_t)q * qa.cap;
  int* out = qa.localKf + (size_t)q * qa.kfOut;
  if (t == 0) { running = 0; sMax = 0; sRefOrder = INT_MAX; sRef = -1; }
  // the vote (:3223-3261)
  const int n = min(max(qa.count[q], 0), qa.cap);
  for (int i = t; i < n; i += LM_NT) {
    const int mp = frameMp[i];
    if (mp < 0 || mp >= a.nmp) continue;
    if (a.mpFlags[mp] & LM_BAD) { frameMp[i] = -1; continue; }   // :3237 / :3257
    for (int j = a.mpObsStart[mp]; j < a.mpObsStart[mp + 1]; ++j) {
      const int kf = a.mpObsKf[j];
      if (row_ok(kf, nkf)) atomicAdd(&word[kf], 1);
    }
  }
  __syncthreads();
  // max: the greatest count among the keyframes that are not bad (:3276-3281)
  int m = 0;
  for (int i = t; i < nkf; i += LM_NT) {
    const int v = __hip_atomic_load(&word[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the adds went to L2
    if (qa.votes) qa.votes[(size_t)q * nkf + i] = v;
    if (!(a.kfFlags[i] & LM_BAD)) m = max(m, v);
  }
  if (m > 0) atomicMax(&sMax, m);
  __syncthreads();
  const int vmax = sMax;
  // first stage (:3271-3285), in d_kfOrder order
  for (int w = 0; w < nkf; w += LM_WINDOW) {
    int row = w + t < nkf ? w + t : -1;
    if (a.kfOrder) {
      window_rows(sRow, w, nkf, [&](int i) { return a.kfOrder[i]; });
      row = sRow[t];
    }
    int v = 0;
    if (row >= 0) v = __hip_atomic_load(&word[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool listed = row >= 0 && v > 0 && !(a.kfFlags[row] & LM_BAD);
    const int c = ordered_slot(listed, lane, wv, wcount, &running);
    if (row >= 0) word[row] = listed ? c + 1 : 0;   // votes -> stamp
    if (listed) {
      if (c < LM_WINDOW) sHead[c] = row;
      if (c < qa.kfOut) out[c] = row;
      if (v == vmax) atomicMin(&sRefOrder, w + t);   // the first with the strictly greatest count
    }
    ordered_commit<LM_NW>(wcount, &running);
    if (listed && v == vmax && sRefOrder == w + t) sRef = row;
    __syncthreads();
  }
  // second stage and the tail: serial by nature, one lane
  if (t == 0) {
    WalkGraph g{word, a.kfFlags, sHead, out, qa.kfOut, running};
    second_stage(g, running, nkf, a.covis, a.ncovis, a.childStart, a.child, a.parent);
    temporal_tail(g, g.size, qa.inertial, qa.lastKf ? qa.lastKf[q] : -1, nkf, a.prevKf);
    qa.nLocalKf[q] = g.size;
    qa.refKf[q] = sRef;
    qa.overflow[q] = g.size > qa.kfOut ? LM_OVERFLOW_KF : 0;
  }
}

__global__ __launch_bounds__(LM_NT) void k_lm_point_keys(MapArgs a, const int* nLocalKf, const int* words, uint32_t* keys) {
  const int lane = threadIdx.x & 63, q = blockIdx.y;
  const int kf = blockIdx.x * LM_NW + (threadIdx.x >> 6);
  if (kf >= a.nkf) return;   // wave-uniform
  const int w = words[(size_t)q * a.nkf + kf];
  if (w == 0) return;
  const int rp = nLocalKf[q] - w;   // position from the list's end
  uint32_t* key = keys + (size_t)q * a.nmp;
  const int* row = a.kfMp + (size_t)kf * a.kfCap;
  const int n = min(max(a.kfCount[kf], 0), a.kfCap);
  for (int idx = lane; idx < n; idx += 64) {
    const int mp = row[idx];
    if (mp < 0 || mp >= a.nmp || (a.mpFlags[mp] & LM_BAD)) continue;
    atomicMin(&key[mp], sequence_key(rp, a.kfCap, idx));
  }
}

__global__ __launch_bounds__(LM_NT) void k_lm_points(MapArgs a, QueryArgs qa, const int* words, uint32_t* keys) {
  __shared__ int sRow[LM_WINDOW], wcount[LM_NW], running;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = blockIdx.x, nkf = a.nkf;
  const int* word = words + (size_t)q * nkf;
  uint32_t* key = keys + (size_t)q * a.nmp;
  int* out = qa.localMp + (size_t)q * qa.mpCap;
  const int nLocal = qa.nLocalKf[q];
  if (t == 0) running = 0;
  __syncthreads();
  for (int w = 0; w < nLocal; w += LM_WINDOW) {
    window_rows(sRow, w, nkf, [&](int i) { const int s = word[i]; return s ? nLocal - s : -1; });
    const int nw = min(LM_WINDOW, nLocal - w);
    for (int k = 0; k < nw; ++k) {
      const int kf = sRow[k];   // workgroup-uniform
      if (kf < 0) continue;
      const int* row = a.kfMp + (size_t)kf * a.kfCap;
      const int n = min(max(a.kfCount[kf], 0), a.kfCap);
      for (int base = 0; base < n; base += LM_NT) {
        const int idx = base + t;
        int mp = -1;
        if (idx < n) mp = row[idx];
        // A listed point's word has LM_LISTED set and equals no sequence key, so a second meeting (in this pass or a later one) fails
        // the test whether it reads the key or the word.
        const bool won = mp >= 0 && mp < a.nmp && key[mp] == sequence_key(w + k, a.kfCap, idx);
        const int c = ordered_slot(won, lane, wv, wcount, &running);
        if (won) {
          if (c < qa.mpCap) out[c] = mp;
          key[mp] = listed_word(c);
        }
        ordered_commit<LM_NW>(wcount, &running);
      }
    }
  }
  if (t == 0) {
    qa.nLocalMp[q] = running;
    if (running > qa.mpCap) qa.overflow[q] |= LM_OVERFLOW_MP;
  }
  if (qa.frameLocal) {
    const int* frameMp = qa.frameMp + (size_t)q * qa.cap;
    const int n = min(max(qa.count[q], 0), qa.cap);
    for (int i = t; i < qa.cap; i += LM_NT) {
      int pos = -1;
      if (i < n) {
        const int mp = frameMp[i];
        if (mp >= 0 && mp < a.nmp) pos = listed_position(key[mp]);
        if (pos >= qa.mpCap) pos = -1;
      }
      qa.frameLocal[(size_t)q * qa.cap + i] = pos;
    }
  }
}

struct GatherArgs {
  int nmp, mpCap;
  const int* localMp;
  const int* nLocalMp;
  const float *Pw, *normal, *maxDist, *minDist;
  const uint8_t *desc, *isBad, *hasObs;
  float *oPw, *oNormal, *oMaxDist, *oMinDist;
  uint8_t *oDesc, *oIsBad, *oHasObs;
};

// one thread per (query, list entry, descriptor byte): 32 consecutive threads copy one point
__global__ __launch_bounds__(256) void k_lm_gather(GatherArgs g) {
  const int q = blockIdx.y;
  const int n = min(max(g.nLocalMp[q], 0), g.mpCap);
  const int j = blockIdx.x * 256 + threadIdx.x, c = j >> 5, b = j & 31;
  if (c >= n) return;
  const int mp = g.localMp[(size_t)q * g.mpCap + c];
  if (mp < 0 || mp >= g.nmp) return;
  const size_t o = (size_t)q * g.mpCap + c;
  g.oDesc[o * 32 + b] = g.desc[(size_t)mp * 32 + b];
  if (b < 3) g.oPw[o * 3 + b] = g.Pw[(size_t)mp * 3 + b];
  else if (b < 6) g.oNormal[o * 3 + (b - 3)] = g.normal[(size_t)mp * 3 + (b - 3)];
  else if (b == 6) g.oMaxDist[o] = g.maxDist[mp];
  else if (b == 7) g.oMinDist[o] = g.minDist[mp];
  else if (b == 8) g.oIsBad[o] = g.isBad[mp];
  else if (b == 9) g.oHasObs[o] = g.hasObs[mp];
}

}  // namespace

extern "C" {

int morb_update_local_map_batch(morb_matcher* m, int nq, int nkf, int kfCap, const int* d_kfMp, const int* d_kfCount,
                                const uint8_t* d_kfFlags, const int* d_kfOrder, const int* d_covis, int ncovis, const int* d_childStart,
                                const int* d_child, const int* d_parent, const int* d_prevKf, int nmp, const int* d_mpObsStart,
                                const int* d_mpObsKf, const uint8_t* d_mpFlags, int cap, int* d_frameMp, const int* d_count,
                                const int* d_lastKf, int inertial, int kfOut, int* d_localKf, int* d_nLocalKf, int* d_refKf, int mpCap,
                                int* d_localMp, int* d_nLocalMp, int* d_frameLocal, int* d_votes, int* d_overflow, void* stream) {
  MORB_REQUIRE(m, MORB_ERR_INVALID, "NULL handle");
  MORB_REQUIRE(nq >= 0 && nkf >= 0 && nmp >= 0 && ncovis >= 0 && cap >= 1 && kfCap >= 1 && kfOut >= 1 && mpCap >= 1, MORB_ERR_INVALID,
               "bad sizes");
  if (nq == 0) return MORB_OK;
  MORB_REQUIRE(d_frameMp && d_count && d_localKf && d_nLocalKf && d_refKf && d_localMp && d_nLocalMp && d_overflow, MORB_ERR_INVALID,
               "NULL argument");
  MORB_REQUIRE(nkf == 0 || (d_kfMp && d_kfCount && d_kfFlags && (d_covis || ncovis == 0)), MORB_ERR_INVALID, "NULL keyframe table");
  MORB_REQUIRE(nmp == 0 || (d_mpObsStart && d_mpObsKf && d_mpFlags), MORB_ERR_INVALID, "NULL map point table");
  MORB_REQUIRE(nq <= 65535 && (size_t)nkf * (size_t)kfCap <= (size_t)INT_MAX && (size_t)nq * ((size_t)nkf + (size_t)nmp) <= (size_t)INT_MAX,
               MORB_ERR_CAPACITY, "more than 65535 queries, or nkf * kfCap or nq * (nkf + nmp) beyond 2^31");
  MORB_ENTER(st, m, stream);
  const size_t nWord = (size_t)nq * nkf, nKey = (size_t)nq * nmp;
  int* ws = nullptr;
  const int rc = morb::grow(m->localMap, nWord + nKey + 1, &ws);
  if (rc != MORB_OK) return rc;
  int* words = ws;
  uint32_t* keys = reinterpret_cast<uint32_t*>(ws + nWord);
  MapArgs a{nkf, kfCap, ncovis, nmp, d_kfMp, d_kfCount, d_kfFlags, d_kfOrder, d_covis, d_childStart, d_child, d_parent, d_prevKf,
            d_mpObsStart, d_mpObsKf, d_mpFlags};
  QueryArgs qa{cap, inertial ? 1 : 0, kfOut, mpCap, d_frameMp, d_count, d_lastKf, d_localKf, d_nLocalKf, d_refKf, d_localMp, d_nLocalMp,
               d_frameLocal, d_votes, d_overflow};
  if (nWord + nKey > 0) {
    const int blocks = (int)std::min<size_t>((nWord + nKey + 255) / 256, 4096);
    hipLaunchKernelGGL(k_lm_init, dim3(blocks), dim3(256), 0, st, words, nWord, keys, nKey);
    MORB_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_lm_keyframes, dim3(nq), dim3(LM_NT), 0, st, a, qa, words);
  MORB_HIP_CHECK(hipGetLastError());
  if (nkf > 0 && nmp > 0) {
    hipLaunchKernelGGL(k_lm_point_keys, dim3(morb::div_up(nkf, LM_NW), nq), dim3(LM_NT), 0, st, a, d_nLocalKf, words, keys);
    MORB_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_lm_points, dim3(nq), dim3(LM_NT), 0, st, a, qa, words, keys);
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}

int morb_gather_local_map_points_batch(morb_matcher* m, int nq, int nmp, const float* d_mpPw, const float* d_mpNormal,
                                       const float* d_mpMaxDist, const float* d_mpMinDist, const uint8_t* d_mpDescriptor,
                                       const uint8_t* d_mpIsBad, const uint8_t* d_mpObserved, int mpCap, const int* d_localMp,
                                       const int* d_nLocalMp, float* d_Pw, float* d_normal, float* d_maxDist, float* d_minDist,
                                       uint8_t* d_mpDesc, uint8_t* d_isBad, uint8_t* d_mpHasObs, void* stream) {
  MORB_REQUIRE(m, MORB_ERR_INVALID, "NULL handle");
  MORB_REQUIRE(nq >= 0 && nmp >= 0 && mpCap >= 1, MORB_ERR_INVALID, "bad sizes");
  if (nq == 0 || nmp == 0) return MORB_OK;
  MORB_REQUIRE(d_mpPw && d_mpNormal && d_mpMaxDist && d_mpMinDist && d_mpDescriptor && d_mpIsBad && d_mpObserved && d_localMp && d_nLocalMp &&
                   d_Pw && d_normal && d_maxDist && d_minDist && d_mpDesc && d_isBad && d_mpHasObs, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nq <= 65535 && (size_t)mpCap * 32 <= (size_t)INT_MAX, MORB_ERR_CAPACITY, "more than 65535 queries, or mpCap beyond 2^26");
  MORB_ENTER(st, m, stream);
  GatherArgs g{nmp, mpCap, d_localMp, d_nLocalMp, d_mpPw, d_mpNormal, d_mpMaxDist, d_mpMinDist, d_mpDescriptor, d_mpIsBad, d_mpObserved,
               d_Pw, d_normal, d_maxDist, d_minDist, d_mpDesc, d_isBad, d_mpHasObs};
  hipLaunchKernelGGL(k_lm_gather, dim3(morb::div_up(mpCap * 32, 256), nq), dim3(256), 0, st, g);
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}

}  // extern "C"
