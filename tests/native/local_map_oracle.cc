// CPU oracle of Tracking::UpdateLocalMap, written from reading the reference's src/Tracking.cc:3184-3358: objects with pointers, a real
// std::map<KeyFrame*, int> for the votes, std::set<KeyFrame*> for the children, one stamp per object, the reserve and the iterators
// of the second loop.  The keyframe objects live in ONE array and keyframe `row` sits at slot d_kfOrder[row], so that the order of
// the pointers IS the prescribed order.  lm_oracle_walk runs include/morb/local_map_math.h's walks (what the kernels compile) on the
// same tables behind a first stage of its own, for the tests to compare the two.
#include <chrono>
#include <cstdint>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "morb/local_map_math.h"

namespace {

struct KeyFrame;

struct MapPoint {
  int row = -1;
  bool bad = false;
  long mnTrackReferenceForFrame = 0;
  std::map<KeyFrame*, std::tuple<int, int>> mObservations;
  bool isBad() const { return bad; }
  std::map<KeyFrame*, std::tuple<int, int>> GetObservations() const { return mObservations; }
};

struct KeyFrame {
  int row = -1;
  bool bad = false;
  long mnTrackReferenceForFrame = 0;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<KeyFrame*> covis;
  std::set<KeyFrame*> mspChildrens;
  KeyFrame* mpParent = nullptr;
  KeyFrame* mPrevKF = nullptr;
  bool isBad() const { return bad; }
  std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(int) const { return covis; }
  std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
  KeyFrame* GetParent() const { return mpParent; }
};

struct Frame {
  long mnId = 0;
  int N = 0;
  std::vector<MapPoint*> mvpMapPoints;
  KeyFrame* mpLastKeyFrame = nullptr;
  KeyFrame* mpReferenceKF = nullptr;
};

struct Tracker {
  Frame mCurrentFrame;
  std::vector<KeyFrame*> mvpLocalKeyFrames;
  std::vector<MapPoint*> mvpLocalMapPoints;
  KeyFrame* mpReferenceKF = nullptr;
  bool inertial = false;
  std::map<KeyFrame*, int> lastCounter;

  void UpdateLocalKeyFrames() {
    std::map<KeyFrame*, int> keyframeCounter;
    for (int i = 0; i < mCurrentFrame.N; i++) {
      MapPoint* pMP = mCurrentFrame.mvpMapPoints[i];
      if (!pMP) continue;
      if (pMP->isBad()) {
        mCurrentFrame.mvpMapPoints[i] = nullptr;
        continue;
      }
      const std::map<KeyFrame*, std::tuple<int, int>> observations = pMP->GetObservations();
      for (auto it = observations.begin(); it != observations.end(); ++it) keyframeCounter[it->first]++;
    }
    lastCounter = keyframeCounter;

    int max = 0;
    KeyFrame* pKFmax = nullptr;
    mvpLocalKeyFrames.clear();
    mvpLocalKeyFrames.reserve(3 * keyframeCounter.size());
    for (auto it = keyframeCounter.begin(); it != keyframeCounter.end(); ++it) {
      KeyFrame* pKF = it->first;
      if (pKF->isBad()) continue;
      if (it->second > max) {
        max = it->second;
        pKFmax = pKF;
      }
      mvpLocalKeyFrames.push_back(pKF);
      pKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
    }

    // The iterators are taken once: the loop runs over the first stage's entries.  The reserve keeps them valid while the list
    // grows: each entry but the last adds at most two, and the one that adds a third (the parent) leaves the loop at once.
    for (auto itKF = mvpLocalKeyFrames.begin(), itEndKF = mvpLocalKeyFrames.end(); itKF != itEndKF; ++itKF) {
      if (mvpLocalKeyFrames.size() > 80) break;
      KeyFrame* pKF = *itKF;
      const std::vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
      for (KeyFrame* pNeighKF : vNeighs) {
        if (!pNeighKF->isBad() && pNeighKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
          mvpLocalKeyFrames.push_back(pNeighKF);
          pNeighKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
          break;
        }
      }
      const std::set<KeyFrame*> spChilds = pKF->GetChilds();
      for (KeyFrame* pChildKF : spChilds) {
        if (!pChildKF->isBad() && pChildKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
          mvpLocalKeyFrames.push_back(pChildKF);
          pChildKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
          break;
        }
      }
      KeyFrame* pParent = pKF->GetParent();
      if (pParent && pParent->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
        mvpLocalKeyFrames.push_back(pParent);
        pParent->mnTrackReferenceForFrame = mCurrentFrame.mnId;
        break;   // of the keyframe loop
      }
    }

    if (inertial && mvpLocalKeyFrames.size() < 80) {
      KeyFrame* tempKeyFrame = mCurrentFrame.mpLastKeyFrame;
      const int Nd = 20;
      for (int i = 0; i < Nd; i++) {
        if (!tempKeyFrame) break;
        if (tempKeyFrame->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
          mvpLocalKeyFrames.push_back(tempKeyFrame);
          tempKeyFrame->mnTrackReferenceForFrame = mCurrentFrame.mnId;
          tempKeyFrame = tempKeyFrame->mPrevKF;
        }
      }
    }

    if (pKFmax) {
      mpReferenceKF = pKFmax;
      mCurrentFrame.mpReferenceKF = mpReferenceKF;
    }
  }

  void UpdateLocalPoints() {
    mvpLocalMapPoints.clear();
    for (auto itKF = mvpLocalKeyFrames.rbegin(); itKF != mvpLocalKeyFrames.rend(); ++itKF) {
      const std::vector<MapPoint*> vpMPs = (*itKF)->GetMapPointMatches();
      for (MapPoint* pMP : vpMPs) {
        if (!pMP) continue;
        if (pMP->mnTrackReferenceForFrame == mCurrentFrame.mnId) continue;
        if (!pMP->isBad()) {
          mvpLocalMapPoints.push_back(pMP);
          pMP->mnTrackReferenceForFrame = mCurrentFrame.mnId;
        }
      }
    }
  }
};

// the header's walks on plain arrays
struct HostGraph {
  std::vector<int> stamp, list;
  const uint8_t* flags;
  bool stamped(int kf) const { return stamp[kf] != 0; }
  bool bad(int kf) const { return (flags[kf] & morblm::LM_BAD) != 0; }
  int first(int i) const { return list[i]; }
  void add(int kf) { stamp[kf] = 1; list.push_back(kf); }
};

double g_last_ms = 0;   // the two reference functions of the last lm_oracle_update, without building the objects

}  // namespace

extern "C" {

double lm_oracle_last_ms() { return g_last_ms; }

// one query; localKf [nkf], localMp [nmp], votes [nkf] take the whole lists.  frameMp [cap] is in / out.
int lm_oracle_update(int nkf, int kfCap, const int* kfMp, const int* kfCount, const uint8_t* kfFlags, const int* kfOrder, const int* covis,
                     int ncovis, const int* childStart, const int* child, const int* parent, const int* prevKf, int nmp,
                     const int* mpObsStart, const int* mpObsKf, const uint8_t* mpFlags, int* frameMp, int count, int lastKf, int inertial,
                     int* localKf, int* nLocalKf, int* refKf, int* localMp, int* nLocalMp, int* votes) {
  std::vector<KeyFrame> kfs(nkf);   // slot = position in the order
  std::vector<MapPoint> mps(nmp);
  std::vector<KeyFrame*> at(nkf);   // row -> object
  for (int r = 0; r < nkf; ++r) {
    at[r] = &kfs[kfOrder ? kfOrder[r] : r];
    if (at[r]->row != -1) return -1;   // not a permutation
    at[r]->row = r;
  }
  auto kf = [&](int r) -> KeyFrame* { return r >= 0 && r < nkf ? at[r] : nullptr; };
  auto mp = [&](int r) -> MapPoint* { return r >= 0 && r < nmp ? &mps[r] : nullptr; };
  for (int r = 0; r < nmp; ++r) {
    mps[r].row = r;
    mps[r].bad = mpFlags[r] & 1;
    for (int j = mpObsStart[r]; j < mpObsStart[r + 1]; ++j)
      if (KeyFrame* k = kf(mpObsKf[j])) mps[r].mObservations[k] = std::make_tuple(j, -1);
  }
  for (int r = 0; r < nkf; ++r) {
    KeyFrame* k = at[r];
    k->bad = kfFlags[r] & 1;
    const int n = kfCount[r] < kfCap ? kfCount[r] : kfCap;
    for (int i = 0; i < n; ++i) k->mvpMapPoints.push_back(mp(kfMp[(long)r * kfCap + i]));
    for (int j = 0; j < ncovis; ++j)
      if (KeyFrame* c = kf(covis[(long)r * ncovis + j])) k->covis.push_back(c);
    if (childStart)
      for (int j = childStart[r]; j < childStart[r + 1]; ++j)
        if (KeyFrame* c = kf(child[j])) k->mspChildrens.insert(c);
    k->mpParent = parent ? kf(parent[r]) : nullptr;
    k->mPrevKF = prevKf ? kf(prevKf[r]) : nullptr;
  }
  Tracker T;
  T.inertial = inertial != 0;
  T.mCurrentFrame.mnId = 7;
  T.mCurrentFrame.N = count;
  for (int i = 0; i < count; ++i) T.mCurrentFrame.mvpMapPoints.push_back(mp(frameMp[i]));
  T.mCurrentFrame.mpLastKeyFrame = kf(lastKf);
  const auto t0 = std::chrono::steady_clock::now();
  T.UpdateLocalKeyFrames();
  T.UpdateLocalPoints();
  g_last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int i = 0; i < count; ++i)
    if (frameMp[i] >= 0 && frameMp[i] < nmp && !T.mCurrentFrame.mvpMapPoints[i]) frameMp[i] = -1;
  *nLocalKf = (int)T.mvpLocalKeyFrames.size();
  for (int i = 0; i < *nLocalKf; ++i) localKf[i] = T.mvpLocalKeyFrames[i]->row;
  *refKf = T.mpReferenceKF ? T.mpReferenceKF->row : -1;
  *nLocalMp = (int)T.mvpLocalMapPoints.size();
  for (int i = 0; i < *nLocalMp; ++i) localMp[i] = T.mvpLocalMapPoints[i]->row;
  for (int r = 0; r < nkf; ++r) votes[r] = 0;
  for (auto& kv : T.lastCounter) votes[kv.first->row] = kv.second;
  return 0;
}

// local_map_math.h's second_stage and temporal_tail behind a first stage computed from `votes` (lm_oracle_update's): -> the list's length
int lm_oracle_walk(int nkf, const uint8_t* kfFlags, const int* kfOrder, const int* covis, int ncovis, const int* childStart,
                   const int* child, const int* parent, const int* prevKf, const int* votes, int lastKf, int inertial, int* localKf) {
  std::vector<int> rowAt(nkf);
  for (int r = 0; r < nkf; ++r) rowAt[kfOrder ? kfOrder[r] : r] = r;
  HostGraph g;
  g.stamp.assign(nkf, 0);
  g.flags = kfFlags;
  for (int p = 0; p < nkf; ++p) {
    const int r = rowAt[p];
    if (votes[r] > 0 && !g.bad(r)) g.add(r);
  }
  const int n1 = (int)g.list.size();
  const int n2 = morblm::second_stage(g, n1, nkf, covis, ncovis, childStart, child, parent);
  const int n3 = morblm::temporal_tail(g, n2, inertial, lastKf, nkf, prevKf);
  if (n3 != (int)g.list.size()) return -1;
  for (int i = 0; i < n3; ++i) localKf[i] = g.list[i];
  return n3;
}

// the constants host and device share: 0 LM_SIZE_LIMIT, 1 LM_TAIL_STEPS, 2 LM_WALK_MAX, 3 LM_WINDOW
int lm_oracle_constant(int which) {
  const int v[4] = {morblm::LM_SIZE_LIMIT, morblm::LM_TAIL_STEPS, morblm::LM_WALK_MAX, morblm::LM_WINDOW};
  return which >= 0 && which < 4 ? v[which] : -1;
}

}  // extern "C"
