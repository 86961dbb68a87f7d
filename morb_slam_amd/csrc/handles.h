// The matcher and optimizer handles of libmorb_hip.so, shared by every translation unit that works on them, and the entry helper
// of their calls.  Nothing here allocates: the members own their HIP resources through hip_owned.h.
#pragma once
#include <cstdint>
#include <vector>

#include "ba_host.h"
#include "common.h"
#include "hip_owned.h"

// Sharing, as the code has it today: a workspace is reused from call to call and across the entry points named at its member, and
// the STREAM orders that reuse: a call's kernels run behind those of the previous call on the same stream.  One handle per stream
// is the convention the front end follows (frontend.py:64, a second ORBmatcher for the BoW stream: "one workspace set per stream");
// calls on one handle from several streams or threads at once would share these buffers unordered.
struct morb_matcher {
  int device = 0;
  morb::Stream stream;
  // grow-only workspaces (hip_owned.h: kernels queued on a caller's stream may still read an outgrown block, so it lives as long as the handle)
  morb::DeviceGrow sortA;        // k_bow_sort's sorted (node, feature) keys
  morb::DeviceGrow bin;          // k_bow_match / k_rot_filter: rotation histogram bins
  morb::DeviceGrow sad;          // k_stereo_match / k_stereo_median
  morb::DeviceGrow stereoRec;    // k_stereo_prep's per-frame records
  // projection.hip's searches; a helper (window_search, kfproj_candidates, best_per_query) takes the members its body names
  morb::DeviceGrow candKeys;     // candidate keys per query (k_candidates, k_search).  Also: fisheye stereo's knn indices
  morb::DeviceGrow candCount;    // candidates per query.  Also: fisheye stereo's knn distances
  morb::DeviceGrow evictJ;       // k_resolve's eviction chain, features.  Also: rotation bins of SearchForTriangulation (k_rot_filter12)
  morb::DeviceGrow evictB;       // k_resolve's eviction chain, displaced queries
  morb::DeviceGrow pairTables;   // SearchForTriangulation's per-pair tables (F12 and epipoles, or the rig's cameras and transforms)
  morb::DeviceGrow newPointPairs;  // CreateNewMapPoints' per-pair poses and descriptor-order flags (new_map_points.hip); its own buffer: the search before it on the stream reads pairTables
  morb::DeviceGrow queries;      // the Query records of a search.  Also: fisheye stereo's per-frame counts and offsets
  morb::DeviceGrow queryCount;   // queries per frame / pair
  morb::DeviceGrow kfdbPair;     // k_kfdb_intersect's per-(query, keyframe) first-word ranks, scores and common-word counts (keyframe_database.hip)
  morb::DeviceGrow kfdbList;     // k_kfdb_select's sort lists of queries on a pool of more keyframes than fit the LDS
  morb::DeviceGrow localMap;     // UpdateLocalMap's per-query keyframe words (votes, then stamps) and map point sequence keys: nq * (nkf + nmp) ints (local_map.hip)
  morb::DeviceGrow scratch;      // per call: the unused projXR plane of isInFrustum (KB8), SearchForInitialization's gathered query descriptors, SearchByBoW's matched2
  // small constant tables (PredictScale thresholds, camera parameters): device copy + the host bytes it was made from, so that a
  // call with the same table neither uploads nor waits (matcher.hip: morb_matcher_const)
  // Four most-recently-used copies per slot (a KB8 rig alternates the left and the right camera's table on one slot); a live copy is never
  // rewritten — a kernel of an earlier call, queued on another caller's stream, may still be reading it: a replaced copy is retired, and
  // freed with the handle.
  struct ConstCopy { morb::DeviceArray<> d; std::vector<uint8_t> host; unsigned long long used = 0; };
  struct ConstSlot { ConstCopy way[4]; unsigned long long clock = 0; };
  enum ConstTable {
    kThresholdsPinhole = 0,   // the 16 level thresholds (isInFrustum and the keyframe projections share the table)
    kThresholdsKB8 = 1,       // ... followed by a KB8 camera's 8 parameters
    kRigLastFrame = 2,        // KB8 camera + Trl of SearchByProjection(CurrentFrame, LastFrame) on a fisheye rig
  };
  ConstSlot consts[4];         // indexed by ConstTable
  std::vector<morb::DeviceArray<>> retired;
};

// Sharing: as morb_matcher's.  Optimizer.h is entered from three threads; each of them is meant to hold a handle of its own.  One
// handle shared by calls on different streams has them share `spill` unordered: a known open item.
struct morb_optimizer {
  int device = 0;
  morb::Stream stream;
  // grid-mode LocalBA runs pairs of independent small phases side by side (per-point / per-keyframe builds, Schur
  // complement / reduced right-hand side): fork-join on a side stream
  morb::Stream side;
  morb::Event evFork, evJoin;
  // grow-only buffers (hip_owned.h: growth neither waits nor frees — Optimizer.h:46-139 is all-static and entered from three threads, and a
  // tracking-thread call must not wait for the LocalBundleAdjustment another thread has running on this device)
  morb::DeviceGrow work;       // device workspace of the one-shot entry points (morb_local_inertial_ba, the one-shot LocalBundleAdjustment): carved anew at every call by ba_host.h's ArenaCarver
  morb::DeviceGrow spill;      // device buffer of the BATCH entry points: edge lists (k_pose_inertial) and correspondences (OptimizeSim3, Sim3Solver) that do not fit the LDS
  morb::DeviceGrow mlpnpCorr;  // MLPnPsolver's correspondences of problems that do not fit the LDS (k_mlpnp_solver); its own buffer, so that no other entry point's launch shares it
  morb::DeviceGrow twoViewCorr;  // TwoViewReconstruction's matches of problems that do not fit the LDS (k_two_view); its own buffer, as mlpnpCorr is
  morb::DeviceGrow inertialOpt;  // InertialOptimization's per-link information matrices and scratch records, and the chain records of problems that do not fit the LDS (k_inertial_optimization)
  morb::DeviceGrow initialMap;   // CreateInitialMapMonocular's per-point records of problems that do not fit the LDS (k_initial_map); its own buffer, as mlpnpCorr is
  morb::DeviceGrow essentialGraph;  // OptimizeEssentialGraph's graph lists, per-edge Jacobians and the block envelope of H and of its LDL^T factor (essential_graph.hip), carved anew at every call by ArenaCarver; its own buffer: a map-sized block that `work`'s local windows never need
  morb::DeviceGrow globalBA;        // BundleAdjustment's flattened map, per-edge Jacobians, Schur contribution lists and the 6 x 6 block envelope of the reduced system and of its LDL^T factor (global_ba.hip), carved anew at every call by ArenaCarver; its own buffer, as essentialGraph is
  morb::DeviceGrow fullInertialBA;  // FullInertialBA's flattened map, per-edge and per-link records, Schur contribution lists and the 3 x 3 block envelope of the reduced system and of its LDL^T factor (full_inertial_ba.hip), carved anew at every call by ArenaCarver; its own buffer, as globalBA is
  morb::PinnedGrow stage;      // pinned host buffer: the one-shot entry points gather their inputs here for a single upload (ba_host.h: the mirror of `work`'s upload region)
  morb::PinnedArray<int> lmWords;   // 16 pinned, device-mapped ints: LM state mirror of the one-shot entry points (optimizer.hip: morb_optimizer_lm_words)
  int exactOrder = 1;             // PoseOptimization: 1 (default) = edge-order sums, the LM path of g2o decision for decision; 0 = tree sums
  int mfmaChain = 0;              // ... carried by the FP64 matrix core (this device passed k_mfma_order_selftest) instead of dependent v_add_f64
  int mfmaSelftest = -1;          // what k_mfma_order_selftest said on this device: 1 passed, 0 rejected, -1 not run (MORB_PO2_CHAIN forced the choice) or failed to run
};

namespace morb {

// n elements of T in a grow-only buffer (device or pinned host)
template <class Block, typename T>
int grow(GrowOnly<Block>& b, size_t n, T** out) {
  void* p = nullptr;
  const int rc = b.ensure(sizeof(T) * n, &p);
  *out = static_cast<T*>(p);
  return rc;
}

// The per-problem workspace of a batched RANSAC solver, whose entries (`words` 4-byte words each) live in LDS up to ldsN per problem:
// only a batch whose cap exceeds ldsN gets one, *pitch bytes (a multiple of 256) per problem at *ws; else *ws = null, *pitch = 0.
inline int grow_beyond_lds(DeviceGrow& b, int nprob, int cap, int ldsN, int words, char** ws, size_t* pitch) {
  *ws = nullptr;
  *pitch = 0;
  if (cap <= ldsN) return MORB_OK;
  *pitch = ((size_t)cap * words * 4 + 255) / 256 * 256;
  return grow(b, *pitch * (size_t)nprob, ws);
}

// the stream a call runs on: the caller's, or the handle's own when the caller passes none
template <class Handle>
inline hipStream_t stream_or_own(const Handle* h, void* stream) { return stream ? (hipStream_t)stream : (hipStream_t)h->stream; }

// The host's two steps around ba_host.h's lm_slot_queue, which is compiled without HIP and therefore cannot hold them.
// Before a solve's first launch: the mapped LM words are cleared — `stop`, the word the caller's stop flag is forwarded to (null: the
// optimiser has none), and the mirror hostw[0 .. words): [0] decided trials, [1] done (last, with release), then what the unit keeps there.
inline void reset_lm_words(int* hostw, int words, int* stop) {
  if (stop) __atomic_store_n(stop, 0, __ATOMIC_RELAXED);
  for (int k = 0; k < words; ++k)
    if (k != 1) __atomic_store_n(hostw + k, 0, __ATOMIC_RELAXED);
  __atomic_store_n(hostw + 1, 0, __ATOMIC_RELEASE);
}
// The queue's look(): is everything queued on st done?  A failed stream leaves its error, under the optimiser's name `who`.
inline StreamLook stream_look(hipStream_t st, const char* who) {
  const hipError_t e = hipStreamQuery(st);
  if (e != hipSuccess && e != hipErrorNotReady) set_error("%s: %s while waiting for the LM decision", who, hipGetErrorString(e));
  return e == hipSuccess ? StreamLook::Idle : e == hipErrorNotReady ? StreamLook::Busy : StreamLook::Failed;
}

}  // namespace morb

// Entry of a call on a handle, behind its argument checks: select the handle's device and declare `st`, the stream the call runs on.
#define MORB_ENTER(st, h, stream)              \
  MORB_HIP_CHECK(hipSetDevice((h)->device));   \
  hipStream_t st = ::morb::stream_or_own(h, stream)
