// KeyFrameDatabase::DetectNBestCandidates (reference src/KeyFrameDatabase.cc:579-705) and DetectRelocalizationCandidates (:707-814)
// with DBoW2's L1 score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), batched over queries, on the BowVector pool that
// morb_bow_vector_batch leaves on the device.  Two kernels on the caller's stream, no host synchronisation:
//   k_kfdb_intersect  one WAVE per (query, keyframe): the lanes take the keyframe's words 64 at a time and binary-search them in
//                     the query's row; the ballots give the common-word count and the query rank of the first common word; the
//                     L1 terms are added lane after lane in ascending word order, one FP64 chain, so the double is the reference's
//                     sum bit for bit.  A keyframe that is outside the database, shares no word or (N best) is connected to the
//                     query is "not stamped": words = -1.
//   k_kfdb_select     one workgroup per query: max count, the threshold, the scored keyframes in lKFsSharingWords' order, the
//                     covisibility accumulation (one lane per entry, float adds in neighbour order), then either the stable
//                     descending order by accScore and the two candidate lists, or the 0.75 test and the relocalisation list.
// No inverted file is kept: `add` appends a keyframe to all its words at once and `erase` / `clearMap` keep relative order, so a
// word's list is always "the database keyframes holding that word, in add order", and lKFsSharingWords is the sharing keyframes
// sorted by (rank in the query of their first common word, add rank).  Both orderings are bitonic sorts of UNIQUE 64-bit keys
// (keyframe_database_math.h), which makes them deterministic and the second one stable; the lists live in LDS up to KFDB_LDS_N
// keyframes in the pool and in the handle's kfdbList workspace beyond that.
// Decisions taken here ("KeyFrameDatabase"):
//   * a query id never equals a stamp an earlier query left or the initial 0, so "stamped by this query" is a function of this
//     query alone; the stored score of a stamped keyframe that is not scored is d_prevScore's (0 where that is NULL);
//   * only the L1 score is built (ORBvoc.txt's, the only one the reference runs);
//   * pool rows out of range in d_qImg, d_conn or d_covis are ignored (an out-of-range query shares no word with anything).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "common.h"
#include "handles.h"
#include "morb_hip.h"
#include "morb/keyframe_database_math.h"
#include "ransac_block.h"
#include "wave.h"

#ifndef MORB_KFDB_LDS_N
#define MORB_KFDB_LDS_N 4096   // list entries (12 bytes each) a query keeps in LDS; a power of two
#endif

namespace {

using namespace morbkfdb;
using namespace morbransac;

constexpr int KFDB_NT = 256, KFDB_NW = KFDB_NT / 64;
constexpr int KFDB_LDS_N = MORB_KFDB_LDS_N;
constexpr int KFDB_LIST_WORDS = 3;   // a 64-bit key and an int per list entry
static_assert((KFDB_LDS_N & (KFDB_LDS_N - 1)) == 0, "the bitonic sort pads to a power of two");

struct PoolArgs {
  int nimg, cap;
  const int* qImg;
  const int* bowWord;
  const double* bowValue;
  const int* bowCount;
  const int* dbRank;
  const int* connStart;   // null: no connected set (relocalisation)
  const int* conn;
};

__global__ __launch_bounds__(KFDB_NT) void k_kfdb_intersect(PoolArgs a, int* words, int* first, float* si) {
  const int lane = threadIdx.x & 63, q = blockIdx.y;
  const int kf = blockIdx.x * KFDB_NW + (threadIdx.x >> 6);
  if (kf >= a.nimg) return;   // wave-uniform
  const size_t o = (size_t)q * a.nimg + kf;
  const int qi = a.qImg[q];
  int count = 0, firstRank = -1;
  double s = 0.0;
  if (qi >= 0 && qi < a.nimg && a.dbRank[kf] >= 0) {
    const int nQ = min(max(a.bowCount[qi], 0), a.cap), nK = min(max(a.bowCount[kf], 0), a.cap);
    const int* qW = a.bowWord + (size_t)qi * a.cap;
    const double* qV = a.bowValue + (size_t)qi * a.cap;
    const int* kW = a.bowWord + (size_t)kf * a.cap;
    const double* kV = a.bowValue + (size_t)kf * a.cap;
    for (int base = 0; base < nK && nQ > 0; base += 64) {
      const int i = base + lane;
      bool found = false;
      int pos = 0;
      double term = 0.0;
      if (i < nK) {
        const int w = kW[i];
        int lo = 0, hi = nQ;   // first query word >= w
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (qW[mid] < w) lo = mid + 1; else hi = mid;
        }
        pos = lo;
        found = pos < nQ && qW[pos] == w;
        if (found) term = l1_term(qV[pos], kV[i]);
      }
      unsigned long long bal = __ballot(found);
      if (bal == 0ull) continue;
      if (firstRank < 0) firstRank = __shfl(pos, __ffsll((long long)bal) - 1);
      count += __popcll(bal);
      while (bal) {   // the reference's sum: one add per common word, ascending
        const int src = __ffsll((long long)bal) - 1;
        s += morbwave::readlane_f64(term, src);
        bal &= bal - 1ull;
      }
    }
    if (count > 0 && a.connStart) {   // spConnectedKF.count(pKFi): never stamped, never listed (:603)
      const int c0 = a.connStart[q], c1 = a.connStart[q + 1];
      bool hit = false;
      for (int j = c0 + lane; j < c1; j += 64) hit |= a.conn[j] == kf;
      if (__ballot(hit) != 0ull) count = 0;
    }
  }
  if (lane == 0) {
    words[o] = count > 0 ? count : -1;
    first[o] = firstRank;
    si[o] = l1_score(s);
  }
}

struct SelectArgs {
  int nimg, ncovis, nNumCandidates;
  const int* qImg;    // N best: the query's map is mapId[qImg[q]]
  const int* qMap;    // relocalisation: the query's map
  const int* dbRank;
  const int* covis;
  const int* mapId;
  const uint8_t* flags;
  const float* prev;  // null: zeros
  const int* words;   // k_kfdb_intersect's
  int* first;         // k_kfdb_intersect's first-word ranks; reused as the first position of each pBestKF
  const float* si;
  int *candA, *nA, *candB, *nB;   // N best: loop / merge lists; relocalisation: the candidate list in A
  float* score;       // may be null
};

// ascending bitonic sort of (key, val) over n = a power of two entries, by the whole workgroup; ends in a barrier
__device__ __forceinline__ void block_sort(uint64_t* key, int* val, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = threadIdx.x; idx < (n >> 1); idx += KFDB_NT) {
        const int i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), l = i | j;
        const uint64_t ki = key[i], kl = key[l];
        if ((ki > kl) == ((i & k) == 0)) {
          key[i] = kl; key[l] = ki;
          const int vi = val[i]; val[i] = val[l]; val[l] = vi;
        }
      }
      __syncthreads();
    }
  }
}

template <bool RELOC, bool LDS>
__global__ __launch_bounds__(KFDB_NT) void k_kfdb_select(SelectArgs a, char* ws, size_t pitch, int wsN) {
  __shared__ uint64_t sKey[LDS ? KFDB_LDS_N : 1];
  __shared__ int sVal[LDS ? KFDB_LDS_N : 1];
  __shared__ int wcount[KFDB_NW], running, sMax, sBestBits;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = blockIdx.x, nimg = a.nimg;
  uint64_t* key = LDS ? sKey : reinterpret_cast<uint64_t*>(ws + (size_t)q * pitch);
  int* val = LDS ? sVal : reinterpret_cast<int*>(ws + (size_t)q * pitch + (size_t)wsN * 8);
  const int* words = a.words + (size_t)q * nimg;
  int* first = a.first + (size_t)q * nimg;
  const float* si = a.si + (size_t)q * nimg;
  const int outN = RELOC ? nimg : a.nNumCandidates;
  for (int i = t; i < outN; i += KFDB_NT) {
    a.candA[(size_t)q * outN + i] = -1;
    if (!RELOC) a.candB[(size_t)q * outN + i] = -1;
  }
  if (t == 0) { running = 0; sMax = 0; sBestBits = 0; }
  __syncthreads();
  // maxCommonWords over lKFsSharingWords (:615-621)
  int m = 0;
  for (int i = t; i < nimg; i += KFDB_NT) m = max(m, words[i]);
  if (m > 0) atomicMax(&sMax, m);
  __syncthreads();
  const int minCommon = min_common_words(sMax);
  // lScoreAndMatch's members (:630-641), and the stored score every keyframe is left with
  for (int base = 0; base < nimg; base += KFDB_NT) {
    const int i = base + t;
    const bool scored = i < nimg && words[i] > minCommon;
    if (i < nimg && a.score) a.score[(size_t)q * nimg + i] = scored ? si[i] : (a.prev ? a.prev[i] : 0.f);
    const int c = ordered_slot(scored, lane, wv, wcount, &running);
    if (scored) { key[c] = first_word_key(first[i], a.dbRank[i]); val[c] = i; }
    ordered_commit<KFDB_NW>(wcount, &running);
  }
  const int ns = running;
  int npad = 1;
  while (npad < ns) npad <<= 1;
  for (int i = ns + t; i < npad; i += KFDB_NT) { key[i] = ~0ull; val[i] = -1; }
  __syncthreads();
  if (ns == 0) {   // :612 / :643 and :732 / :763
    if (t == 0) { a.nA[q] = 0; if (!RELOC) a.nB[q] = 0; }
    return;
  }
  block_sort(key, val, npad);   // lKFsSharingWords' order
  // accumulate by covisibility (:649-672), one lane per entry
  for (int i = t; i < ns; i += KFDB_NT) {
    const int kf = val[i];
    float bestScore = si[kf], accScore = bestScore;
    int pBest = kf;
    for (int j = 0; j < a.ncovis; ++j) {
      const int nb = a.covis[(size_t)kf * a.ncovis + j];
      if (nb < 0 || nb >= nimg) continue;
      const int w = words[nb];
      if (w < 0) continue;   // not stamped by this query
      const float sc = w > minCommon ? si[nb] : (a.prev ? a.prev[nb] : 0.f);
      accScore += sc;
      if (sc > bestScore) { pBest = nb; bestScore = sc; }
    }
    if (RELOC) {
      if (accScore > 0.f) atomicMax(&sBestBits, __float_as_int(accScore));   // positive floats order as their bit patterns
      key[i] = (uint64_t)(uint32_t)__float_as_int(accScore);
    } else {
      key[i] = acc_sort_key(accScore, (uint32_t)i);
    }
    val[i] = pBest;
  }
  __syncthreads();
  if (!RELOC) block_sort(key, val, npad);   // lAccScoreAndMatch.sort(compFirst); the padding keys stay last
  const float bestAcc = __int_as_float(sBestBits);
  const int qmap = RELOC ? a.qMap[q] : a.mapId[min(max(a.qImg[q], 0), nimg - 1)];
  // spAlreadyAddedKF: the first position of each pBestKF among the entries that reach the duplicate test
  for (int i = t; i < nimg; i += KFDB_NT) first[i] = INT_MAX;
  __syncthreads();
  for (int p = t; p < ns; p += KFDB_NT) {
    const int pb = val[p];
    const bool reach = RELOC ? (retained(__int_as_float((int)(uint32_t)key[p]), bestAcc) && a.mapId[pb] == qmap) : !(a.flags[pb] & KFDB_BAD);
    if (reach) atomicMin(&first[pb], p);
  }
  __syncthreads();
  for (int pass = 0; pass < (RELOC ? 1 : 2); ++pass) {
    if (t == 0) running = 0;
    __syncthreads();
    int* out = (pass == 0 ? a.candA : a.candB) + (size_t)q * outN;
    for (int base = 0; base < ns; base += KFDB_NT) {
      const int p = base + t;
      bool valid = false;
      int pb = -1;
      if (p < ns) {
        pb = val[p];
        valid = first[pb] == p;
        if (!RELOC && valid) {
          const bool same = a.mapId[pb] == qmap;
          valid = pass == 0 ? same : (!same && !(a.flags[pb] & KFDB_MAP_BAD));
        }
      }
      const int c = ordered_slot(valid, lane, wv, wcount, &running);
      if (valid && c < outN) out[c] = pb;
      ordered_commit<KFDB_NW>(wcount, &running);
    }
    if (t == 0) (pass == 0 ? a.nA : a.nB)[q] = min(running, outN);
    __syncthreads();
  }
}

int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// both entries: the pair workspace, the intersection, the selection
template <bool RELOC>
int detect(morb_matcher* m, int nq, const PoolArgs& pa, SelectArgs sa, int* d_words, hipStream_t st) {
  const size_t pairs = (size_t)nq * pa.nimg;
  int* pairWs = nullptr;   // first ranks, scores and (unless the caller takes them) counts of every (query, keyframe)
  int rc = morb::grow(m->kfdbPair, pairs * (d_words ? 2 : 3), &pairWs);
  if (rc != MORB_OK) return rc;
  int* first = pairWs;
  float* si = reinterpret_cast<float*>(pairWs + pairs);
  int* words = d_words ? d_words : pairWs + 2 * pairs;
  char* ws = nullptr;
  size_t pitch = 0;
  const int wsN = pow2_at_least(pa.nimg);
  rc = morb::grow_beyond_lds(m->kfdbList, nq, wsN, KFDB_LDS_N, KFDB_LIST_WORDS, &ws, &pitch);
  if (rc != MORB_OK) return rc;
  hipLaunchKernelGGL(k_kfdb_intersect, dim3(morb::div_up(pa.nimg, KFDB_NW), nq), dim3(KFDB_NT), 0, st, pa, words, first, si);
  MORB_HIP_CHECK(hipGetLastError());
  sa.words = words; sa.first = first; sa.si = si;
  if (ws) hipLaunchKernelGGL((k_kfdb_select<RELOC, false>), dim3(nq), dim3(KFDB_NT), 0, st, sa, ws, pitch, wsN);
  else hipLaunchKernelGGL((k_kfdb_select<RELOC, true>), dim3(nq), dim3(KFDB_NT), 0, st, sa, ws, pitch, wsN);
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}

}  // namespace

extern "C" {

int morb_detect_n_best_candidates_batch(morb_matcher* m, int nq, const int* d_qImg, int nimg, int cap, const int* d_bowWord,
                                        const double* d_bowValue, const int* d_bowCount, const int* d_dbRank, const int* d_connStart,
                                        const int* d_conn, const int* d_covis, int ncovis, const int* d_mapId, const uint8_t* d_flags,
                                        const float* d_prevScore, int nNumCandidates, int* d_loopCand, int* d_nLoop, int* d_mergeCand,
                                        int* d_nMerge, int* d_words, float* d_score, void* stream) {
  MORB_REQUIRE(m, MORB_ERR_INVALID, "NULL handle");
  MORB_REQUIRE(nq >= 0 && nimg >= 0 && cap >= 1 && ncovis >= 0 && nNumCandidates >= 1, MORB_ERR_INVALID, "bad sizes");
  if (nq == 0 || nimg == 0) return MORB_OK;
  MORB_REQUIRE(d_qImg && d_bowWord && d_bowValue && d_bowCount && d_dbRank && d_connStart && d_mapId && d_flags && d_loopCand && d_nLoop &&
                   d_mergeCand && d_nMerge && (d_covis || ncovis == 0), MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nq <= 65535 && (size_t)nq * (size_t)nimg <= (size_t)INT_MAX, MORB_ERR_CAPACITY, "more than 65535 queries, or nq * nimg beyond 2^31");
  MORB_ENTER(st, m, stream);
  PoolArgs pa{nimg, cap, d_qImg, d_bowWord, d_bowValue, d_bowCount, d_dbRank, d_connStart, d_conn};
  SelectArgs sa{};
  sa.nimg = nimg; sa.ncovis = ncovis; sa.nNumCandidates = nNumCandidates;
  sa.qImg = d_qImg; sa.dbRank = d_dbRank; sa.covis = d_covis; sa.mapId = d_mapId; sa.flags = d_flags; sa.prev = d_prevScore;
  sa.candA = d_loopCand; sa.nA = d_nLoop; sa.candB = d_mergeCand; sa.nB = d_nMerge; sa.score = d_score;
  return detect<false>(m, nq, pa, sa, d_words, st);
}

int morb_detect_relocalization_candidates_batch(morb_matcher* m, int nq, const int* d_qImg, const int* d_qMap, int nimg, int cap,
                                                const int* d_bowWord, const double* d_bowValue, const int* d_bowCount,
                                                const int* d_dbRank, const int* d_covis, int ncovis, const int* d_mapId,
                                                const float* d_prevScore, int* d_cand, int* d_nCand, int* d_words, float* d_score,
                                                void* stream) {
  MORB_REQUIRE(m, MORB_ERR_INVALID, "NULL handle");
  MORB_REQUIRE(nq >= 0 && nimg >= 0 && cap >= 1 && ncovis >= 0, MORB_ERR_INVALID, "bad sizes");
  if (nq == 0 || nimg == 0) return MORB_OK;
  MORB_REQUIRE(d_qImg && d_qMap && d_bowWord && d_bowValue && d_bowCount && d_dbRank && d_mapId && d_cand && d_nCand &&
                   (d_covis || ncovis == 0), MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nq <= 65535 && (size_t)nq * (size_t)nimg <= (size_t)INT_MAX, MORB_ERR_CAPACITY, "more than 65535 queries, or nq * nimg beyond 2^31");
  MORB_ENTER(st, m, stream);
  PoolArgs pa{nimg, cap, d_qImg, d_bowWord, d_bowValue, d_bowCount, d_dbRank, nullptr, nullptr};
  SelectArgs sa{};
  sa.nimg = nimg; sa.ncovis = ncovis; sa.nNumCandidates = 1;
  sa.qMap = d_qMap; sa.dbRank = d_dbRank; sa.covis = d_covis; sa.mapId = d_mapId; sa.prev = d_prevScore;
  sa.candA = d_cand; sa.nA = d_nCand; sa.score = d_score;
  return detect<true>(m, nq, pa, sa, d_words, st);
}

}  // extern "C"
