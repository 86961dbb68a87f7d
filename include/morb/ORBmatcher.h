// Drop-in adapter: ORB_SLAM3::ORBmatcher (reference include/ORBmatcher.h:36-129) over libmorb_hip.so — all 13 public methods.
//
// The reference's methods take Frame / KeyFrame / MapPoint objects; what they READ from them is a handful of arrays.  The adapter
// takes exactly those arrays as plain views (FrameView / KeyFrameView, MapPointView below, each member named after the reference
// member it mirrors), so that inside the reference tree the glue is one function per class that fills a view from the object
// (include/morb/reference_glue.h does it under the reference's locks; INTEGRATION.md shows the call sites), and outside it (this
// repository has no OpenCV / Eigen / Sophus) the header compiles as is.  Results come back as index tables with the meaning of the
// containers the reference methods fill (vpMapPointMatches[i] = map point of keyframe feature table[i], ...); the bookkeeping on live
// map state (AddObservation, Replace, ...) stays with the caller, as DESIGN.md states for the whole matcher family.
// Every method: one morb_adapter::CallStaging (device_buffer.h: hipSetDevice(device), uploads and device arrays from per-thread, per-device
// staging that only grows), one C-ABI call per reference call, synchronised on the handle's own stream (never the device: Tracking's matcher
// calls do not wait for the LocalBundleAdjustment trials the mapping thread has in flight on its optimizer handle; only a call that outgrows
// the staging pays for an allocation, which does).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../morb_hip.h"
#include "device_buffer.h"

namespace ORB_SLAM3 {

// Frame / KeyFrame members the searches read (include/Frame.h, include/KeyFrame.h).  Unused members stay NULL.
struct FrameView {
  int N = 0;                                    // N (for a fisheye rig: left + right features, left first)
  const morb_keypoint* mvKeysUn = nullptr;      // [N] (cv::KeyPoint has the same 28-byte layout)
  const uint8_t* mDescriptors = nullptr;        // [N][32]
  const float* mvuRight = nullptr;              // [N] or NULL (monocular)
  const uint8_t* hasTrackedMapPoint = nullptr;  // [N] mvpMapPoints[i] && mvpMapPoints[i]->Observations() > 0 (SearchByProjection's "already matched")
  morb_frame_params params{};
  float mRcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // row-major
  float mtcw[3] = {0, 0, 0};
  float mOw[3] = {0, 0, 0};                     // camera centre = Tcw.inverse().translation()
  float Tcw[7] = {0, 0, 0, 1, 0, 0, 0};         // GetPose() as unit quaternion xyzw + translation
  // BoW: mFeatVec inverted — the vocabulary node (at levelsup) feature i is listed under, -1 if none
  const int* featNode = nullptr;                // [N]
  int nValid = -1;                              // KeyFrame: mvKeysUn.size() where it is smaller than N (fisheye, ORBmatcher.cc:734); -1 = N
  // the map point held by feature i (mvpMapPoints[i] / GetMapPointMatches()[i]):
  const uint8_t* hasMapPoint = nullptr;         // [N] non-NULL && !isBad() (for a last frame: && !mvbOutlier[i])
  const float* mpWorldPos = nullptr;            // [N][3] GetWorldPos()
  const float* mpMaxDistance = nullptr;         // [N] mfMaxDistance (the 1.2 / 0.8 invariance factors are applied inside)
  const float* mpMinDistance = nullptr;         // [N] mfMinDistance
  const uint8_t* mpDescriptor = nullptr;        // [N][32] GetDescriptor()
  const uint8_t* mpHasObservations = nullptr;   // [N] Observations() > 0
};
struct KeyFrameView : FrameView {   // the same members read from a KeyFrame (GetMapPointMatches(), mFeatVec, GetPose(), ...)
  // KannalaBrandt8 rig keyframe (KeyFrame::NLeft != -1): the rows hold mvKeys | mvKeysRight; the loop-closing searches (no rig branch in the reference) then
  // look among the first NLeft features only and project with mpCamera (rigCam8: fx fy cx cy k0..k3) where the reference calls mpCamera->project
  int NLeft = -1;
  float rigCam8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
// MapPoint members read by isInFrustum / SearchByProjection / Fuse (include/MapPoint.h)
struct MapPointView {
  int n = 0;
  const float* worldPos = nullptr;      // [n][3]
  const float* normal = nullptr;        // [n][3] GetNormal()
  const float* maxDistance = nullptr;   // [n]
  const float* minDistance = nullptr;   // [n]
  const uint8_t* descriptor = nullptr;  // [n][32]
  const uint8_t* isBad = nullptr;       // [n]
  const uint8_t* hasObservations = nullptr;  // [n]
  // the state checks at the top of the Sim3 / Fuse loops: non-NULL && !isBad() && !IsInKeyFrame(pKF) (or && !spAlreadyFound.count(pMP))
  const uint8_t* valid = nullptr;       // [n]
};
// Sophus::Sim3f Scw as the searches use it: Tcw = SE3(Scw.rotationMatrix(), Scw.translation() / Scw.scale()), Ow = Tcw.inverse().translation()
struct Sim3View {
  float Tcw[7] = {0, 0, 0, 1, 0, 0, 0};
  float Ow[3] = {0, 0, 0};
};

class ORBmatcher {
 public:
  static const int TH_LOW = 50;      // ORBmatcher.cc:33-35
  static const int TH_HIGH = 100;
  static const int HISTO_LENGTH = 30;

  ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0) : mfNNratio(nnratio), mbCheckOrientation(checkOri), device_(device) {
    if (device < 0 || device >= morb_adapter::kMaxDevices) throw std::runtime_error("ORBmatcher: bad device");
    if (morb_matcher_create(&h_, device) != MORB_OK) throw std::runtime_error(std::string("morb_matcher_create: ") + morb_last_error());
  }
  ~ORBmatcher() { morb_matcher_destroy(h_); }
  ORBmatcher(const ORBmatcher&) = delete;
  ORBmatcher& operator=(const ORBmatcher&) = delete;

  // static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b)  (ORBmatcher.cc:1880-1894): the bit-parallel popcount of the
  // reference on two 32-byte rows.  A host helper of the class surface (callers use it on single pairs); the matchers themselves
  // compute their distances on the device.
  static int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
    int dist = 0;
    for (int i = 0; i < 8; ++i) {
      uint32_t pa, pb;
      std::memcpy(&pa, a + 4 * i, 4); std::memcpy(&pb, b + 4 * i, 4);
      dist += __builtin_popcount(pa ^ pb);
    }
    return dist;
  }

  // Tracking::SearchLocalPoints' pair (Tracking.cc:3117-3183): Frame::isInFrustum(pMP, 0.5) for every candidate — that host loop (IncreaseVisible,
  // mnLastFrameSeen, mmProjectPoints) stays in the integrated tree, see the reference-typed member below — then
  // int SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, th, bFarPoints, thFarPoints)  (ORBmatcher.h:45-47,
  // ORBmatcher.cc:42-209).  matchF[i] = index of the map point assigned to feature i, or -1 (in/out: earlier assignments are kept
  // if the vector already has N entries).  Returns the reference's return value.
  int SearchByProjection(const FrameView& F, const MapPointView& mps, std::vector<int>& matchF, float th = 3.f, bool bFarPoints = false,
                         float thFarPoints = 50.f, float viewingCosLimit = 0.5f) {
    const int N = F.N, M = mps.n;
    if (N <= 0 || M <= 0) { matchF.assign(N > 0 ? N : 0, -1); return 0; }
    Call c(device_, morb_matcher_stream(h_));
    const int img = 0;
    const int *d_fImg = c.in(&img, 1), *d_count = c.in(&N, 1);
    const morb_keypoint* d_kps = c.in(F.mvKeysUn, N);
    const uint8_t* d_desc = c.in(F.mDescriptors, (size_t)N * 32);
    const float* d_uRight = F.mvuRight ? c.in(F.mvuRight, N) : nullptr;
    const uint8_t* d_blocked = F.hasTrackedMapPoint ? c.in(F.hasTrackedMapPoint, N) : c.out_filled<uint8_t>(N, 0);
    const float *d_Rcw = c.in(F.mRcw, 9), *d_tcw = c.in(F.mtcw, 3), *d_Ow = c.in(F.mOw, 3);
    const int* d_nMP = c.in(&M, 1);
    const float *d_Pw = c.in(mps.worldPos, (size_t)M * 3), *d_normal = c.in(mps.normal, (size_t)M * 3), *d_maxDist = c.in(mps.maxDistance, M);
    const float* d_minDist = c.in(mps.minDistance, M);
    const uint8_t *d_isBad = c.in(mps.isBad, M), *d_mpDesc = c.in(mps.descriptor, (size_t)M * 32), *d_mpHasObs = c.in(mps.hasObservations, M);
    uint8_t* d_inView = c.out<uint8_t>(M);   // what isInFrustum leaves in the map points
    float *d_projX = c.out<float>(M), *d_projY = c.out<float>(M), *d_projXR = c.out<float>(M), *d_depth = c.out<float>(M), *d_viewCos = c.out<float>(M);
    int* d_level = c.out<int>(M);
    int* d_matchF = (int)matchF.size() == N ? c.in(matchF.data(), N) : c.out_filled<int>(N, 0xFF);   // -1
    int* d_nmatches = c.out_filled<int>(1, 0);
    check(morb_is_in_frustum_batch(h_, &F.params, 1, d_Rcw, d_tcw, d_Ow, M, d_nMP, d_Pw, d_normal, d_maxDist, d_minDist, viewingCosLimit, d_inView,
                                   d_projX, d_projY, d_projXR, d_depth, d_level, d_viewCos, nullptr));
    check(morb_search_by_projection_mps_batch(h_, &F.params, 1, d_fImg, N, d_count, d_kps, d_desc, d_uRight, d_blocked, M, d_nMP, d_inView, d_isBad,
                                              d_depth, d_projX, d_projY, d_projXR, d_level, d_viewCos, d_mpDesc, d_mpHasObs, th, bFarPoints ? 1 : 0,
                                              thFarPoints, mfNNratio, d_matchF, d_nmatches, nullptr));
    c.wait();
    matchF = c.fetch(d_matchF, N);
    return c.fetch(d_nmatches, 1)[0];
  }

  // int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono)  (ORBmatcher.h:51-52,
  // ORBmatcher.cc:1521-1733; Tracking::TrackWithMotionModel).  Last.hasMapPoint[i] = LastFrame.mvpMapPoints[i] && !LastFrame.mvbOutlier[i];
  // Cur.hasTrackedMapPoint[i2] = CurrentFrame.mvpMapPoints[i2] && Observations() > 0.  matchCur[i2] = index of the LAST-frame feature
  // whose map point is assigned to current feature i2, -1 otherwise (in/out like matchF above).
  int SearchByProjection(const FrameView& Cur, const FrameView& Last, std::vector<int>& matchCur, float th, bool bMono) {
    const int N = Cur.N, NL = Last.N;
    if (N <= 0 || NL <= 0) { matchCur.assign(N > 0 ? N : 0, -1); return 0; }
    Call c(device_, morb_matcher_stream(h_));
    const Pool pool = load_pool(c, {&Cur, &Last});
    const int cap = pool.cap;
    // :1536-1539: tlc = Tlw * twc; forward / backward motion widens the octave range
    float tlc2 = Last.mtcw[2];
    for (int k = 0; k < 3; ++k) tlc2 += Last.mRcw[6 + k] * Cur.mOw[k];
    const uint8_t fwd = (tlc2 > Cur.params.mb && !bMono) ? 1 : 0, bwd = (-tlc2 > Cur.params.mb && !bMono) ? 1 : 0;
    const int cur = 0, last = 1;
    const int *d_curImg = c.in(&cur, 1), *d_lastImg = c.in(&last, 1);
    const uint8_t* d_curBlocked = c.in_rows(Cur.hasTrackedMapPoint, N, cap, 1);
    const float* d_Tcw = c.in(Cur.Tcw, 7);
    const uint8_t* d_lastValid = c.in_rows(Last.hasMapPoint, NL, cap, 1);
    const float* d_lastXw = c.in_rows(Last.mpWorldPos, NL, cap, 3);
    const uint8_t *d_lastMPdesc = c.in_rows(Last.mpDescriptor, NL, cap, 32), *d_lastMPhasObs = c.in_rows(Last.mpHasObservations, NL, cap, 1);
    const uint8_t *d_bForward = c.in(&fwd, 1), *d_bBackward = c.in(&bwd, 1);
    int *d_matchCur = in_match(c, matchCur, N, cap), *d_nmatches = c.out_filled<int>(1, 0);
    check(morb_search_by_projection_last_batch(h_, &Cur.params, 1, d_curImg, d_lastImg, cap, pool.count, pool.kps, pool.desc,
                                               Cur.mvuRight ? pool.uRight : nullptr, d_curBlocked, d_Tcw, d_lastValid, d_lastXw, d_lastMPdesc,
                                               d_lastMPhasObs, th, d_bForward, d_bBackward, mbCheckOrientation ? 1 : 0, d_matchCur, d_nmatches, nullptr));
    c.wait();
    matchCur = c.fetch(d_matchCur, cap); matchCur.resize(N);
    return c.fetch(d_nmatches, 1)[0];
  }

  // int SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, const float th, const int ORBdist)
  // (ORBmatcher.h:56-58, ORBmatcher.cc:1735-1842; relocalisation).  alreadyFound[i] != 0 <=> sAlreadyFound.count(pKF's map point i);
  // Cur.hasMapPoint[i2] = CurrentFrame.mvpMapPoints[i2] != NULL.  matchCur[i2] = keyframe feature whose map point goes to current feature i2.
  // curCam8 / curNLeft: CurrentFrame is a KannalaBrandt8 rig frame (rows hold left | right features): projection with mpCamera (the left
  // camera: fx fy cx cy k0..k3), search among the left features only — the reference has no rig branch in this member, this is what its
  // code does on such a frame (GetFeaturesInArea's bRight defaults to false; morb_search_by_projection_kf_rig_batch).
  int SearchByProjection(const FrameView& Cur, const KeyFrameView& KF, const std::vector<uint8_t>& alreadyFound, std::vector<int>& matchCur,
                         float th, int ORBdist, const float* curCam8 = nullptr, int curNLeft = -1) {
    const int N = Cur.N, NK = KF.N;
    if (N <= 0 || NK <= 0) { matchCur.assign(N > 0 ? N : 0, -1); return 0; }
    Call c(device_, morb_matcher_stream(h_));
    const Pool pool = load_pool(c, {&Cur, &KF});
    const int cap = pool.cap;
    std::vector<uint8_t> kfValid(NK);
    for (int i = 0; i < NK; ++i) kfValid[i] = (KF.hasMapPoint && KF.hasMapPoint[i] && !(i < (int)alreadyFound.size() && alreadyFound[i])) ? 1 : 0;
    const int cur = 0, kf = 1;
    const int *d_curImg = c.in(&cur, 1), *d_kfImg = c.in(&kf, 1);
    const uint8_t* d_curHasMP = c.in_rows(Cur.hasMapPoint, N, cap, 1);
    const float *d_Tcw = c.in(Cur.Tcw, 7), *d_Ow = c.in(Cur.mOw, 3);
    const uint8_t* d_kfValid = c.in_rows(kfValid.data(), NK, cap, 1);
    const float *d_Xw = c.in_rows(KF.mpWorldPos, NK, cap, 3), *d_maxDist = c.in_rows(KF.mpMaxDistance, NK, cap, 1);
    const float* d_minDist = c.in_rows(KF.mpMinDistance, NK, cap, 1);
    const uint8_t* d_mpDesc = c.in_rows(KF.mpDescriptor, NK, cap, 32);
    int *d_matchCur = in_match(c, matchCur, N, cap), *d_nmatches = c.out_filled<int>(1, 0);
    if (curCam8 && curNLeft >= 0) {
      const int* d_nLeftCur = c.in(&curNLeft, 1);
      check(morb_search_by_projection_kf_rig_batch(h_, &Cur.params, curCam8, 1, d_curImg, d_kfImg, d_nLeftCur, cap, pool.count, pool.kps, pool.desc,
                                                   d_curHasMP, d_Tcw, d_Ow, d_kfValid, d_Xw, d_maxDist, d_minDist, d_mpDesc, th, ORBdist,
                                                   mbCheckOrientation ? 1 : 0, d_matchCur, d_nmatches, nullptr));
    } else
    check(morb_search_by_projection_kf_batch(h_, &Cur.params, 1, d_curImg, d_kfImg, cap, pool.count, pool.kps, pool.desc, d_curHasMP, d_Tcw, d_Ow,
                                             d_kfValid, d_Xw, d_maxDist, d_minDist, d_mpDesc, th, ORBdist, mbCheckOrientation ? 1 : 0, d_matchCur,
                                             d_nmatches, nullptr));
    c.wait();
    matchCur = c.fetch(d_matchCur, cap); matchCur.resize(N);
    return c.fetch(d_nmatches, 1)[0];
  }

  // int SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th,
  // float ratioHamming)  (ORBmatcher.h:62-65, ORBmatcher.cc:397-494; loop detection).  vpMatched[idx] = index into vpPoints of the map point
  // matched to keyframe feature idx, -1 = none; entries >= 0 on entry are "already matched" and block their feature (the reference's
  // spAlreadyFound is folded into vpPoints.valid by the caller).  Returns the number of NEW matches, as the reference does.
  int SearchByProjection(const KeyFrameView& KF, const Sim3View& Scw, const MapPointView& vpPoints, std::vector<int>& vpMatched, int th,
                         float ratioHamming = 1.0f) {
    return sim3_projection(KF, Scw, vpPoints, vpMatched, th, ratioHamming, 0);
  }
  // ... the twin with vpPointsKFs / vpMatchedKF (ORBmatcher.h:69-74, ORBmatcher.cc:496-601; place recognition): vpMatchedKF[idx] is
  // vpPointsKFs[vpMatched[idx]] — the keyframe list is parallel to the point list, so the caller reads it through the same index.
  int SearchByProjection(const KeyFrameView& KF, const Sim3View& Scw, const MapPointView& vpPoints, std::vector<int>& vpMatched,
                         std::vector<int>& vpMatchedKF, int th, float ratioHamming = 1.0f) {
    const int n = sim3_projection(KF, Scw, vpPoints, vpMatched, th, ratioHamming, 1);
    vpMatchedKF = vpMatched;
    return n;
  }

  // int SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)  (ORBmatcher.h:79, ORBmatcher.cc:218-395; tracking the
  // reference keyframe, relocalisation).  vpMapPointMatches[j] = keyframe feature whose map point is matched to frame feature j, or -1.
  int SearchByBoW(const KeyFrameView& KF, const FrameView& F, std::vector<int>& vpMapPointMatches) {
    if (KF.N <= 0 || F.N <= 0) { vpMapPointMatches.assign(F.N > 0 ? F.N : 0, -1); return 0; }
    Call c(device_, morb_matcher_stream(h_));
    const Pool pool = load_pool(c, {&KF, &F});
    const int kf = 0, fr = 1;
    const int *d_kfImg = c.in(&kf, 1), *d_fImg = c.in(&fr, 1);
    int *d_matchF = c.out<int>(pool.cap), *d_nmatches = c.out_filled<int>(1, 0);
    check(morb_search_by_bow_batch(h_, 1, d_kfImg, d_fImg, 2, pool.kps, pool.desc, pool.node, pool.count, pool.hasMP, pool.cap, mfNNratio,
                                   mbCheckOrientation ? 1 : 0, d_matchF, d_nmatches, nullptr));
    c.wait();
    vpMapPointMatches = c.fetch(d_matchF, pool.cap); vpMapPointMatches.resize(F.N);
    return c.fetch(d_nmatches, 1)[0];
  }
  // int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)  (ORBmatcher.h:80-81, ORBmatcher.cc:702-819; loop closing).
  // vpMatches12[i1] = feature of pKF2 whose map point is matched to feature i1 of pKF1, or -1.
  int SearchByBoW(const KeyFrameView& KF1, const KeyFrameView& KF2, std::vector<int>& vpMatches12) {
    if (KF1.N <= 0 || KF2.N <= 0) { vpMatches12.assign(KF1.N > 0 ? KF1.N : 0, -1); return 0; }
    Call c(device_, morb_matcher_stream(h_));
    const Pool pool = load_pool(c, {&KF1, &KF2});
    const int a = 0, b = 1;
    const int nv[2] = {KF1.nValid >= 0 ? KF1.nValid : KF1.N, KF2.nValid >= 0 ? KF2.nValid : KF2.N};
    const int *d_kf1Img = c.in(&a, 1), *d_kf2Img = c.in(&b, 1), *d_nValid = c.in(nv, 2);
    int *d_match12 = c.out<int>(pool.cap), *d_nmatches = c.out_filled<int>(1, 0);
    check(morb_search_by_bow_kfkf_batch(h_, 1, d_kf1Img, d_kf2Img, d_nValid, 2, pool.kps, pool.desc, pool.node, pool.count, pool.hasMP, pool.cap,
                                        mfNNratio, mbCheckOrientation ? 1 : 0, d_match12, d_nmatches, nullptr));
    c.wait();
    vpMatches12 = c.fetch(d_match12, pool.cap); vpMatches12.resize(KF1.N);
    return c.fetch(d_nmatches, 1)[0];
  }

  // int SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12, int windowSize)
  // (ORBmatcher.h:84-87, ORBmatcher.cc:603-700; monocular initialisation).  vbPrevMatched = [N1][2] floats (x, y), updated like the reference.
  int SearchForInitialization(const FrameView& F1, const FrameView& F2, std::vector<float>& vbPrevMatched, std::vector<int>& vnMatches12,
                              int windowSize = 10) {
    if (F1.N <= 0 || F2.N <= 0) { vnMatches12.assign(F1.N > 0 ? F1.N : 0, -1); return 0; }
    Call c(device_, morb_matcher_stream(h_));
    const Pool pool = load_pool(c, {&F1, &F2});
    const int cap = pool.cap;
    const int a = 0, b = 1;
    const int *d_img1 = c.in(&a, 1), *d_img2 = c.in(&b, 1);
    std::vector<float> prev((size_t)cap * 2, 0.f);
    std::copy(vbPrevMatched.begin(), vbPrevMatched.begin() + std::min(vbPrevMatched.size(), (size_t)F1.N * 2), prev.begin());
    float* d_prevMatched = c.in(prev.data(), prev.size());
    int *d_matches12 = c.out<int>(cap), *d_nmatches = c.out_filled<int>(1, 0);
    check(morb_search_for_initialization_batch(h_, &F2.params, 1, d_img1, d_img2, cap, pool.count, pool.kps, pool.desc, d_prevMatched, windowSize,
                                               mfNNratio, mbCheckOrientation ? 1 : 0, d_matches12, d_nmatches, nullptr));
    c.wait();
    vnMatches12 = c.fetch(d_matches12, cap); vnMatches12.resize(F1.N);
    c.fetch(d_prevMatched, prev.data(), prev.size());
    vbPrevMatched.assign(prev.begin(), prev.begin() + (size_t)F1.N * 2);
    return c.fetch(d_nmatches, 1)[0];
  }

  // int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, vector<pair<size_t, size_t>>& vMatchedPairs, bool bOnlyStereo, bool bCoarse)
  // (ORBmatcher.h:90-93, ORBmatcher.cc:821-1042; LocalMapping::CreateNewMapPoints), pinhole keyframes.  R12 / t12 = (T1w * Tw2) as rotation
  // matrix (row-major) and translation, ep = pKF2->mpCamera->project(T2w * pKF1->GetCameraCenter()) (:829-838): Sophus expressions the glue
  // evaluates exactly as the reference does.
  int SearchForTriangulation(const KeyFrameView& KF1, const KeyFrameView& KF2, const float R12[9], const float t12[3], const float ep[2],
                             std::vector<std::pair<size_t, size_t>>& vMatchedPairs, bool bOnlyStereo, bool bCoarse = false) {
    vMatchedPairs.clear();
    if (KF1.N <= 0 || KF2.N <= 0) return 0;
    Call c(device_, morb_matcher_stream(h_));
    const Pool pool = load_pool(c, {&KF1, &KF2});
    const int a = 0, b = 1;
    const int *d_img1 = c.in(&a, 1), *d_img2 = c.in(&b, 1);
    int *d_match12 = c.out<int>(pool.cap), *d_nmatches = c.out_filled<int>(1, 0);
    check(morb_search_for_triangulation_batch(h_, &KF1.params, 1, d_img1, d_img2, 2, pool.cap, pool.count, pool.kps, pool.desc, pool.node, pool.hasMP,
                                              (KF1.mvuRight || KF2.mvuRight) ? pool.uRight : nullptr, R12, t12, ep, bOnlyStereo ? 1 : 0, bCoarse ? 1 : 0,
                                              mbCheckOrientation ? 1 : 0, d_match12, d_nmatches, nullptr));
    c.wait();
    const std::vector<int> m12 = c.fetch(d_match12, pool.cap);
    for (int i = 0; i < KF1.N; ++i)
      if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);   // :1030-1036: ascending feature of pKF1
    return c.fetch(d_nmatches, 1)[0];
  }

  // int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, const Sophus::Sim3f& S12, const float th)
  // (ORBmatcher.h:102-104, ORBmatcher.cc:1323-1519; loop closing).  S12 / S21 = S12 and S12.inverse() as 7 floats each: RxSO3 quaternion xyzw
  // whose squared norm is the scale, then the translation.  vpMatches12[i1] = feature of pKF2 (index) matched to feature i1 of pKF1 or -1;
  // entries >= 0 on entry are the reference's vbAlreadyMatched1 / vbAlreadyMatched2 (:1356-1369) and are kept.
  int SearchBySim3(const KeyFrameView& KF1, const KeyFrameView& KF2, std::vector<int>& vpMatches12, const float S12[7], const float S21[7], float th) {
    const int N1 = KF1.N, N2 = KF2.N;
    if (N1 <= 0 || N2 <= 0) return 0;
    Call c(device_, morb_matcher_stream(h_));
    const Pool pool = load_pool(c, {&KF1, &KF2});
    const int cap = pool.cap;
    if ((int)vpMatches12.size() != N1) vpMatches12.assign(N1, -1);
    std::vector<uint8_t> v1(N1), v2(N2);
    std::vector<uint8_t> already2(N2, 0);
    for (int i = 0; i < N1; ++i) if (vpMatches12[i] >= 0 && vpMatches12[i] < N2) already2[vpMatches12[i]] = 1;
    for (int i = 0; i < N1; ++i) v1[i] = (KF1.hasMapPoint && KF1.hasMapPoint[i] && vpMatches12[i] < 0) ? 1 : 0;
    for (int i = 0; i < N2; ++i) v2[i] = (KF2.hasMapPoint && KF2.hasMapPoint[i] && !already2[i]) ? 1 : 0;
    const int a = 0, b = 1;
    const int *d_kf1Img = c.in(&a, 1), *d_kf2Img = c.in(&b, 1);
    const float *d_T1w = c.in(KF1.Tcw, 7), *d_T2w = c.in(KF2.Tcw, 7), *d_S12 = c.in(S12, 7), *d_S21 = c.in(S21, 7);
    const uint8_t* d_valid1 = c.in_rows(v1.data(), N1, cap, 1);
    const float *d_Pw1 = c.in_rows(KF1.mpWorldPos, N1, cap, 3), *d_maxDist1 = c.in_rows(KF1.mpMaxDistance, N1, cap, 1);
    const float* d_minDist1 = c.in_rows(KF1.mpMinDistance, N1, cap, 1);
    const uint8_t *d_mpDesc1 = c.in_rows(KF1.mpDescriptor, N1, cap, 32), *d_valid2 = c.in_rows(v2.data(), N2, cap, 1);
    const float *d_Pw2 = c.in_rows(KF2.mpWorldPos, N2, cap, 3), *d_maxDist2 = c.in_rows(KF2.mpMaxDistance, N2, cap, 1);
    const float* d_minDist2 = c.in_rows(KF2.mpMinDistance, N2, cap, 1);
    const uint8_t* d_mpDesc2 = c.in_rows(KF2.mpDescriptor, N2, cap, 32);
    int *d_vnMatch1 = c.out<int>(cap), *d_vnMatch2 = c.out<int>(cap), *d_match12 = c.out<int>(cap), *d_nFound = c.out_filled<int>(1, 0);
    if (KF1.NLeft >= 0 || KF2.NLeft >= 0) {   // rig keyframes: the candidates are the left features (a keyframe without a right camera: all of them)
      const int nl1 = KF1.NLeft >= 0 ? KF1.NLeft : N1, nl2 = KF2.NLeft >= 0 ? KF2.NLeft : N2;
      const int *d_nLeft1 = c.in(&nl1, 1), *d_nLeft2 = c.in(&nl2, 1);
      check(morb_search_by_sim3_rig_batch(h_, &KF1.params, 1, d_kf1Img, d_kf2Img, cap, pool.count, pool.kps, pool.desc, d_T1w, d_T2w, d_S12, d_S21,
                                          d_valid1, d_Pw1, d_maxDist1, d_minDist1, d_mpDesc1, d_valid2, d_Pw2, d_maxDist2, d_minDist2, d_mpDesc2, th,
                                          d_nLeft1, d_nLeft2, d_vnMatch1, d_vnMatch2, d_match12, d_nFound, nullptr));
    } else
    check(morb_search_by_sim3_batch(h_, &KF1.params, 1, d_kf1Img, d_kf2Img, cap, pool.count, pool.kps, pool.desc, d_T1w, d_T2w, d_S12, d_S21, d_valid1,
                                    d_Pw1, d_maxDist1, d_minDist1, d_mpDesc1, d_valid2, d_Pw2, d_maxDist2, d_minDist2, d_mpDesc2, th, d_vnMatch1,
                                    d_vnMatch2, d_match12, d_nFound, nullptr));
    c.wait();
    const std::vector<int> m12 = c.fetch(d_match12, cap);
    for (int i = 0; i < N1; ++i) if (m12[i] >= 0) vpMatches12[i] = m12[i];   // :1506-1515
    return c.fetch(d_nFound, 1)[0];
  }

  // int Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th, const bool bRight)  (ORBmatcher.h:107-108,
  // ORBmatcher.cc:1044-1213; LocalMapping::SearchInNeighbors) — the search: bestIdx[i] = feature of pKF chosen for map point i
  // (bestDist <= TH_LOW) or -1.  What follows a hit (Replace / AddObservation / AddMapPoint, :1196-1208) depends on live map state and is
  // replayed by the caller over bestIdx in map-point order; the return value here is the number of hits.
  // On a KannalaBrandt8 rig (KeyFrame::NLeft != -1; KF holds mvKeys | mvKeysRight in one row) `side` names the camera searched: its pose and
  // centre (GetPose / GetCameraCenter, or GetRightPose / GetRightCameraCenter with bRight), its KB8 parameters and its feature range
  // ([0, NLeft) or [NLeft, N)); the indices returned count from the start of the row (:1050-1054, :1130-1177).
  struct RigSide { float Tcw[7]; float Ow[3]; float cam8[8]; int jLo, jHi; };
  int Fuse(const KeyFrameView& KF, const MapPointView& vpMapPoints, std::vector<int>& bestIdx, std::vector<int>& bestDist, float th = 3.0f,
           const RigSide* side = nullptr) {
    Sim3View T;
    if (side) { std::memcpy(T.Tcw, side->Tcw, sizeof T.Tcw); std::memcpy(T.Ow, side->Ow, sizeof T.Ow); }
    else { std::memcpy(T.Tcw, KF.Tcw, sizeof T.Tcw); std::memcpy(T.Ow, KF.mOw, sizeof T.Ow); }
    return fuse(KF, T, vpMapPoints, bestIdx, bestDist, th, 0, side);
  }
  // int Fuse(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints, float th, vector<MapPoint*>& vpReplacePoint)
  // (ORBmatcher.h:112-114, ORBmatcher.cc:1215-1321; loop closing): vpReplacePoint[i] = pKF->GetMapPoint(bestIdx[i]) where that is non-NULL.
  int Fuse(const KeyFrameView& KF, const Sim3View& Scw, const MapPointView& vpPoints, float th, std::vector<int>& bestIdx, std::vector<int>& bestDist) {
    if (KF.NLeft >= 0) {   // rig keyframe (no rig branch in the reference: pCamera = pKF->mpCamera, the left features)
      RigSide side;
      std::memcpy(side.Tcw, Scw.Tcw, sizeof side.Tcw); std::memcpy(side.Ow, Scw.Ow, sizeof side.Ow); std::memcpy(side.cam8, KF.rigCam8, sizeof side.cam8);
      side.jLo = 0; side.jHi = KF.NLeft;
      return fuse(KF, Scw, vpPoints, bestIdx, bestDist, th, 1, &side);
    }
    return fuse(KF, Scw, vpPoints, bestIdx, bestDist, th, 1);
  }

  morb_matcher* handle() { return h_; }   // for the batched / device-resident entry points

  // ---- the reference's own signatures (include/ORBmatcher.h:41-114) as member templates: a call site of src/Tracking.cc / src/LocalMapping.cc /
  // src/LoopClosing.cc compiles unchanged and instantiates them with the reference's Frame / KeyFrame / MapPoint / Sophus types
  // (definitions: ORBmatcher_reference.h, included below) ----
  template <class Mat, class = typename std::enable_if<!std::is_pointer<Mat>::value>::type>
  static int DescriptorDistance(const Mat& a, const Mat& b);
  template <class FrameT, class MP>
  int SearchByProjection(FrameT& F, const std::vector<MP*>& vpMapPoints, const float th = 3, const bool bFarPoints = false, const float thFarPoints = 50.0f);
  template <class FrameT>
  int SearchByProjection(FrameT& CurrentFrame, const FrameT& LastFrame, const float th, const bool bMono);
  template <class FrameT, class KF, class MP>
  int SearchByProjection(FrameT& CurrentFrame, KF* pKF, const std::set<MP*>& sAlreadyFound, const float th, const int ORBdist);
  template <class KF, class Sim3, class MP>
  int SearchByProjection(KF* pKF, Sim3& Scw, const std::vector<MP*>& vpPoints, std::vector<MP*>& vpMatched, int th, float ratioHamming = 1.0);
  template <class KF, class Sim3, class MP>
  int SearchByProjection(KF* pKF, Sim3& Scw, const std::vector<MP*>& vpPoints, const std::vector<KF*>& vpPointsKFs, std::vector<MP*>& vpMatched,
                         std::vector<KF*>& vpMatchedKF, int th, float ratioHamming = 1.0);
  template <class KF, class FrameT, class MP, class = typename std::enable_if<!std::is_pointer<FrameT>::value>::type>
  int SearchByBoW(KF* pKF, FrameT& F, std::vector<MP*>& vpMapPointMatches);
  template <class KF, class MP>
  int SearchByBoW(KF* pKF1, KF* pKF2, std::vector<MP*>& vpMatches12);
  template <class FrameT, class Pt, class = typename std::enable_if<!std::is_base_of<FrameView, FrameT>::value>::type>
  int SearchForInitialization(FrameT& F1, FrameT& F2, std::vector<Pt>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize = 10);
  template <class KF>
  int SearchForTriangulation(KF* pKF1, KF* pKF2, std::vector<std::pair<size_t, size_t>>& vMatchedPairs, const bool bOnlyStereo, const bool bCoarse = false);
  template <class KF, class MP, class Sim3>
  int SearchBySim3(KF* pKF1, KF* pKF2, std::vector<MP*>& vpMatches12, const Sim3& S12, const float th);
  template <class KF, class MP>
  int Fuse(KF* pKF, const std::vector<MP*>& vpMapPoints, const float th = 3.0, const bool bRight = false);
  template <class KF, class Sim3, class MP>
  int Fuse(KF* pKF, Sim3& Scw, const std::vector<MP*>& vpPoints, float th, std::vector<MP*>& vpReplacePoint);

 protected:
  using Call = morb_adapter::CallStaging;   // one per method call: device, the handle's stream, this thread's staging (device_buffer.h)
  template <class KF, class Sim3, class MP>
  int sim3_projection_ref(KF* pKF, Sim3& Scw, const std::vector<MP*>& vpPoints, const std::vector<KF*>* vpPointsKFs, std::vector<MP*>& vpMatched,
                          std::vector<KF*>* vpMatchedKF, int th, float ratioHamming);
  static void check(int rc) { if (rc < 0) throw std::runtime_error(morb_last_error()); }
  // a match table of cap entries: the caller's N assignments where it holds N, -1 everywhere else
  static int* in_match(Call& c, const std::vector<int>& m, int N, int cap) { return c.in_rows((int)m.size() == N ? m.data() : nullptr, N, cap, 1, -1); }
  // the pool the batched entry points index: image k = views[k], every array [nimg][cap]
  struct Pool {   // count [nimg]; node = BoW node of a feature, -1 if none; uRight -1 where a view has none
    int cap; const morb_keypoint* kps; const uint8_t *desc, *hasMP; const int *count, *node; const float* uRight;
  };
  static Pool load_pool(Call& c, std::initializer_list<const FrameView*> views) {
    int cap = 1;
    for (const FrameView* v : views) cap = std::max(cap, v->N);
    const int nimg = (int)views.size();
    std::vector<morb_keypoint> kps((size_t)nimg * cap);
    std::vector<uint8_t> desc((size_t)nimg * cap * 32, 0), has((size_t)nimg * cap, 0);
    std::vector<int> node((size_t)nimg * cap, -1), count(nimg);
    std::vector<float> ur((size_t)nimg * cap, -1.f);
    std::memset(static_cast<void*>(kps.data()), 0, kps.size() * sizeof(morb_keypoint));
    int k = 0;
    for (const FrameView* v : views) {
      count[k] = v->N;
      std::copy(v->mvKeysUn, v->mvKeysUn + v->N, kps.begin() + (size_t)k * cap);
      std::copy(v->mDescriptors, v->mDescriptors + (size_t)v->N * 32, desc.begin() + (size_t)k * cap * 32);
      if (v->featNode) std::copy(v->featNode, v->featNode + v->N, node.begin() + (size_t)k * cap);
      if (v->hasMapPoint) std::copy(v->hasMapPoint, v->hasMapPoint + v->N, has.begin() + (size_t)k * cap);
      if (v->mvuRight) std::copy(v->mvuRight, v->mvuRight + v->N, ur.begin() + (size_t)k * cap);
      ++k;
    }
    Pool p; p.cap = cap;
    p.kps = c.in(kps.data(), kps.size()); p.desc = c.in(desc.data(), desc.size()); p.hasMP = c.in(has.data(), has.size());
    p.count = c.in(count.data(), count.size()); p.node = c.in(node.data(), node.size()); p.uRight = c.in(ur.data(), ur.size());
    return p;
  }
  struct Points { const uint8_t *valid, *desc; const float *Pw, *normal, *maxDist, *minDist; };
  static Points load_points(Call& c, const MapPointView& P) {
    const size_t M = P.n;
    Points p; p.valid = c.in(P.valid, M); p.Pw = c.in(P.worldPos, M * 3); p.normal = c.in(P.normal, M * 3);
    p.maxDist = c.in(P.maxDistance, M); p.minDist = c.in(P.minDistance, M); p.desc = c.in(P.descriptor, M * 32);
    return p;
  }
  int sim3_projection(const KeyFrameView& KF, const Sim3View& Scw, const MapPointView& P, std::vector<int>& vpMatched, int th, float ratioHamming,
                      int manual) {
    const int N = KF.N, M = P.n;
    if ((int)vpMatched.size() != N) vpMatched.assign(N > 0 ? N : 0, -1);
    if (N <= 0 || M <= 0) return 0;
    Call c(device_, morb_matcher_stream(h_));
    const Pool pool = load_pool(c, {&KF});
    const Points pts = load_points(c, P);
    const int cap = pool.cap;
    std::vector<uint8_t> matched(cap, 0);
    for (int i = 0; i < N; ++i) matched[i] = vpMatched[i] >= 0 ? 1 : 0;
    const int kf = 0;
    const int* d_kfImg = c.in(&kf, 1);
    const float *d_Tcw = c.in(Scw.Tcw, 7), *d_Ow = c.in(Scw.Ow, 3);
    const int* d_nMP = c.in(&M, 1);
    const uint8_t* d_matched = c.in(matched.data(), cap);
    int *d_matchF = c.out<int>(cap), *d_nmatches = c.out_filled<int>(1, 0);
    if (KF.NLeft >= 0) {   // rig keyframe: left features, the left KB8 camera where the reference calls mpCamera->project
      const int* d_nLeft = c.in(&KF.NLeft, 1);
      check(morb_search_by_projection_sim3_rig_batch(h_, &KF.params, 1, d_kfImg, cap, pool.count, pool.kps, pool.desc, d_Tcw, d_Ow, M, d_nMP, pts.valid,
                                                     pts.Pw, pts.normal, pts.maxDist, pts.minDist, pts.desc, d_matched, th, ratioHamming, manual,
                                                     KF.rigCam8, d_nLeft, d_matchF, d_nmatches, nullptr));
    } else
    check(morb_search_by_projection_sim3_batch(h_, &KF.params, 1, d_kfImg, cap, pool.count, pool.kps, pool.desc, d_Tcw, d_Ow, M, d_nMP, pts.valid, pts.Pw,
                                               pts.normal, pts.maxDist, pts.minDist, pts.desc, d_matched, th, ratioHamming, manual, d_matchF, d_nmatches,
                                               nullptr));
    c.wait();
    const std::vector<int> mf = c.fetch(d_matchF, cap);
    for (int i = 0; i < N; ++i) if (mf[i] >= 0) vpMatched[i] = mf[i];
    return c.fetch(d_nmatches, 1)[0];
  }
  int fuse(const KeyFrameView& KF, const Sim3View& T, const MapPointView& P, std::vector<int>& bestIdx, std::vector<int>& bestDist, float th, int sim3Form,
           const RigSide* side = nullptr) {
    const int N = KF.N, M = P.n;
    bestIdx.assign(M > 0 ? M : 0, -1); bestDist.assign(M > 0 ? M : 0, 256);
    if (N <= 0 || M <= 0) return 0;
    Call c(device_, morb_matcher_stream(h_));
    const Pool pool = load_pool(c, {&KF});
    const Points pts = load_points(c, P);
    const int kf = 0;
    const int* d_kfImg = c.in(&kf, 1);
    const float *d_Tcw = c.in(T.Tcw, 7), *d_Ow = c.in(T.Ow, 3);
    const int *d_jLo = side ? c.in(&side->jLo, 1) : nullptr, *d_jHi = side ? c.in(&side->jHi, 1) : nullptr, *d_nMP = c.in(&M, 1);
    int *d_bestIdx = c.out<int>(M), *d_bestDist = c.out<int>(M);
    check(morb_fuse_batch(h_, &KF.params, 1, d_kfImg, pool.cap, pool.count, pool.kps, pool.desc, (KF.mvuRight && !side) ? pool.uRight : nullptr, d_Tcw, d_Ow,
                          side ? side->cam8 : nullptr, d_jLo, d_jHi, M, d_nMP, pts.valid, pts.Pw, pts.normal, pts.maxDist, pts.minDist, pts.desc, th,
                          sim3Form, d_bestIdx, d_bestDist, nullptr));
    c.wait();
    bestIdx = c.fetch(d_bestIdx, M); bestDist = c.fetch(d_bestDist, M);
    int hits = 0;
    for (int i = 0; i < M; ++i) hits += bestIdx[i] >= 0 ? 1 : 0;
    return hits;
  }

  float mfNNratio;
  bool mbCheckOrientation;
  int device_ = 0;
  morb_matcher* h_ = nullptr;
};

}  // namespace ORB_SLAM3

#include "ORBmatcher_reference.h"
