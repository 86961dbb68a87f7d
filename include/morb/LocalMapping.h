// LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:403-711) with the reference's member names, over the GPU entry points:
// per neighbour the pair gate, ORBmatcher::SearchForTriangulation, morb_create_new_map_points_batch for that one pair, and a host
// replay of :693-708 in ascending idx1 (new MapPoint, the two AddObservation, the two AddMapPoint, ComputeDistinctiveDescriptors,
// UpdateNormalAndDepth, the atlas, mlpRecentAddedMapPoints).  The neighbours are visited one after the other, as the reference does:
// AddMapPoint of neighbour k is what the search of neighbour k + 1 sees.
//
// A template on the caller's types, as the other adapters are: it names no OpenCV / Eigen / Sophus type.  What it touches:
//   KeyFrame  GetBestCovisibilityKeyFrames, mPrevKF, GetPose, GetPoseInverse, GetCameraCenter, mb, ComputeSceneMedianDepth, GetMap,
//             NLeft, mpCamera2, N, mvKeysUn, mvKeys, mvuRight, mvDepth, mDescriptors, mfScaleFactor, AddMapPoint and what
//             ORBmatcher::SearchForTriangulation reads;
//   MapPoint  MapPoint(Eigen::Vector3f, KeyFrame*, Map*), AddObservation, ComputeDistinctiveDescriptors, UpdateNormalAndDepth;
//   Atlas     GetCurrentMap, AddMapPoint;   Tracker  mState, RECENTLY_LOST.
// Several idx1 may share one idx2 (the search never sets vbMatched2): the replay keeps the reference's last-wins AddMapPoint on
// keyframe 2.  The device's position, normal, distances and descriptor of every created point stay in `created` beside the pointers,
// for callers that feed morb_fuse_batch or morb_ba_problem_create without asking each MapPoint again.
// Not here: KannalaBrandt8 rigs (morb_create_new_map_points_fisheye_batch has no reference-typed member yet; a rig keyframe throws).
#pragma once
#include <algorithm>
#include <functional>
#include <list>
#include <stdexcept>
#include <utility>
#include <vector>

#include "ORBmatcher.h"
#include "new_map_points_math.h"

namespace ORB_SLAM3 {

template <class KeyFrame, class MapPoint, class Atlas, class Tracker, class Vector3f>
class LocalMappingT {
 public:
  // include/LocalMapping.h
  KeyFrame* mpCurrentKeyFrame = nullptr;
  Atlas* mpAtlas = nullptr;
  Tracker* mpTracker = nullptr;
  bool mbMonocular = false, mbInertial = false, mbFarPoints = false;
  float mThFarPoints = 0.f;
  std::list<MapPoint*> mlpRecentAddedMapPoints;
  std::function<bool()> fnCheckNewKeyFrames;   // the caller's keyframe queue (mlNewKeyFrames under its mutex)
  bool CheckNewKeyFrames() { return fnCheckNewKeyFrames && fnCheckNewKeyFrames(); }

  // one created point as the device made it
  struct Created {
    MapPoint* pMP; KeyFrame* pKF2; int idx1, idx2, status;
    float Xw[3], normal[3], maxDistance, minDistance; uint8_t descriptor[32];
  };
  std::vector<Created> created;                  // of the last CreateNewMapPoints, in creation order
  int countStereo = 0, countStereoGoodProj = 0, countStereoAttempt = 0, totalStereoPts = 0;   // the reference's locals, summed

  explicit LocalMappingT(int device = 0) : device_(device), matcher_(0.6f, false, device) {}   // float th = 0.6f; ORBmatcher matcher(th, false)

  void CreateNewMapPoints() {
    created.clear();
    countStereo = countStereoGoodProj = countStereoAttempt = totalStereoPts = 0;
    // Retrieve neighbor keyframes in covisibility graph
    int nn = 10;
    if (mbMonocular) nn = 30;
    std::vector<KeyFrame*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
    if (mbInertial) {
      KeyFrame* pKF = mpCurrentKeyFrame;
      int count = 0;
      while ((static_cast<int>(vpNeighKFs.size()) <= nn) && (pKF->mPrevKF) && (count++ < nn)) {
        typename std::vector<KeyFrame*>::iterator it = std::find(vpNeighKFs.begin(), vpNeighKFs.end(), pKF->mPrevKF);
        if (it == vpNeighKFs.end()) vpNeighKFs.push_back(pKF->mPrevKF);
        pKF = pKF->mPrevKF;
      }
    }
    if (mpCurrentKeyFrame->NLeft != -1 || mpCurrentKeyFrame->mpCamera2)
      throw std::runtime_error("LocalMapping::CreateNewMapPoints: KannalaBrandt8 rig keyframes go through morb_create_new_map_points_fisheye_batch");

    float poses[4 * morbnmp::NMP_POSE];
    pose12(mpCurrentKeyFrame->GetPose(), poses);
    pose12(mpCurrentKeyFrame->GetPoseInverse(), poses + morbnmp::NMP_POSE);
    const auto Ow1v = mpCurrentKeyFrame->GetCameraCenter();
    const float Ow1[3] = {Ow1v(0), Ow1v(1), Ow1v(2)};
    const float ratioFactor = 1.5f * mpCurrentKeyFrame->mfScaleFactor;

    for (size_t i = 0; i < vpNeighKFs.size(); i++) {
      if (i > 0 && CheckNewKeyFrames()) return;
      KeyFrame* pKF2 = vpNeighKFs[i];
      // Check first that baseline is not too short
      const auto Ow2v = pKF2->GetCameraCenter();
      const float Ow2[3] = {Ow2v(0), Ow2v(1), Ow2v(2)};
      if (morbnmp::nmp_pair_gate(mbMonocular, Ow1, Ow2, pKF2->mb, mbMonocular ? pKF2->ComputeSceneMedianDepth(2) : 0.f)) continue;
      if (pKF2->NLeft != -1 || pKF2->mpCamera2) throw std::runtime_error("LocalMapping::CreateNewMapPoints: rig neighbour");

      // Search matches that fullfil epipolar constraint
      std::vector<std::pair<size_t, size_t>> vMatchedIndices;
      bool bCoarse = mbInertial && mpTracker->mState == Tracker::RECENTLY_LOST && mpCurrentKeyFrame->GetMap()->GetIniertialBA2();
      matcher_.SearchForTriangulation(mpCurrentKeyFrame, pKF2, vMatchedIndices, false, bCoarse);
      if (vMatchedIndices.empty()) continue;

      // Triangulate each match: one pair on the device
      pose12(pKF2->GetPose(), poses + 2 * morbnmp::NMP_POSE);
      pose12(pKF2->GetPoseInverse(), poses + 3 * morbnmp::NMP_POSE);
      const uint8_t kf2First = std::less<KeyFrame*>()(pKF2, mpCurrentKeyFrame) ? 1 : 0;
      KeyFrame* kf[2] = {mpCurrentKeyFrame, pKF2};
      const int cap = std::max(std::max(kf[0]->N, kf[1]->N), 1);
      std::vector<morb_keypoint> kps((size_t)2 * cap), raw((size_t)2 * cap);
      std::memset(static_cast<void*>(kps.data()), 0, kps.size() * sizeof(morb_keypoint));
      std::memset(static_cast<void*>(raw.data()), 0, raw.size() * sizeof(morb_keypoint));
      std::vector<uint8_t> desc((size_t)2 * cap * 32, 0);
      std::vector<float> ur((size_t)2 * cap, -1.f), depth((size_t)2 * cap, -1.f);
      std::vector<int> count(2), m12(cap, -1);
      bool stereo = false;
      for (int k = 0; k < 2; ++k) {
        const int N = kf[k]->N;
        count[k] = N;
        for (int j = 0; j < N; ++j) {
          keypoint(kf[k]->mvKeysUn[j], kps[(size_t)k * cap + j]);
          keypoint(kf[k]->mvKeys[j], raw[(size_t)k * cap + j]);
        }
        std::memcpy(&desc[(size_t)k * cap * 32], kf[k]->mDescriptors.template ptr<uint8_t>(0), (size_t)N * 32);
        if ((int)kf[k]->mvuRight.size() >= N && (int)kf[k]->mvDepth.size() >= N) {
          std::copy(kf[k]->mvuRight.begin(), kf[k]->mvuRight.begin() + N, ur.begin() + (size_t)k * cap);
          std::copy(kf[k]->mvDepth.begin(), kf[k]->mvDepth.begin() + N, depth.begin() + (size_t)k * cap);
          stereo = true;
        }
      }
      for (const auto& mm : vMatchedIndices) m12[mm.first] = (int)mm.second;
      morb_frame_params P;
      morb_glue::fill_params(P, *mpCurrentKeyFrame, mpCurrentKeyFrame->mfGridElementWidthInv, mpCurrentKeyFrame->mfGridElementHeightInv);

      morb_adapter::CallStaging c(device_, morb_matcher_stream(matcher_.handle()));
      const int a = 0, b = 1;
      const int *d_img1 = c.in(&a, 1), *d_img2 = c.in(&b, 1), *d_row = c.in(&a, 1);
      const int *d_count = c.in(count.data(), 2), *d_m12 = c.in(m12.data(), m12.size());
      const morb_keypoint *d_kps = c.in(kps.data(), kps.size()), *d_raw = c.in(raw.data(), raw.size());
      const uint8_t* d_desc = c.in(desc.data(), desc.size());
      const float *d_ur = stereo ? c.in(ur.data(), ur.size()) : nullptr, *d_depth = stereo ? c.in(depth.data(), depth.size()) : nullptr;
      int *d_status = c.template out<int>(cap), *d_stats = c.template out<int>(morbnmp::NMP_STATS_LEN);
      float *d_Xw = c.template out<float>((size_t)cap * 3), *d_normal = c.template out<float>((size_t)cap * 3);
      float *d_maxD = c.template out<float>(cap), *d_minD = c.template out<float>(cap);
      uint8_t *d_mpDesc = c.template out<uint8_t>((size_t)cap * 32), *d_has = c.template out_filled<uint8_t>((size_t)2 * cap, 0);
      int *d_oImg = c.template out<int>(cap), *d_oIdx = c.template out<int>(cap);
      const int rc = morb_create_new_map_points_batch(matcher_.handle(), &P, 1, d_img1, d_img2, 2, cap, d_count, d_kps, d_raw, d_desc, d_ur, d_depth,
                                                      d_m12, poses, &kf2First, ratioFactor, mbInertial ? 1 : 0, mbFarPoints ? 1 : 0, mThFarPoints,
                                                      d_status, d_stats, 1, d_row, d_Xw, d_normal, d_maxD, d_minD, d_mpDesc, d_oImg, d_oIdx, d_has,
                                                      nullptr);
      if (rc < 0) throw std::runtime_error(morb_last_error());
      c.wait();
      const std::vector<int> status = c.fetch(d_status, cap), stats = c.fetch(d_stats, morbnmp::NMP_STATS_LEN);
      const std::vector<float> Xw = c.fetch(d_Xw, (size_t)cap * 3), nrm = c.fetch(d_normal, (size_t)cap * 3);
      const std::vector<float> maxD = c.fetch(d_maxD, cap), minD = c.fetch(d_minD, cap);
      const std::vector<uint8_t> mpDesc = c.fetch(d_mpDesc, (size_t)cap * 32);
      totalStereoPts += stats[morbnmp::NMP_S_TOTAL_STEREO_PTS];
      countStereoAttempt += stats[morbnmp::NMP_S_STEREO_ATTEMPT];
      countStereoGoodProj += stats[morbnmp::NMP_S_STEREO_GOOD_PROJ];
      countStereo += stats[morbnmp::NMP_S_COUNT_STEREO];

      // Triangulation is succesfull: :693-708 for the accepted matches, in the order of vMatchedIndices (ascending idx1)
      for (const auto& mm : vMatchedIndices) {
        const int idx1 = (int)mm.first, idx2 = (int)mm.second;
        if (!morbnmp::nmp_created(status[idx1])) continue;
        MapPoint* pMP = new MapPoint(Vector3f(Xw[3 * idx1], Xw[3 * idx1 + 1], Xw[3 * idx1 + 2]), mpCurrentKeyFrame, mpAtlas->GetCurrentMap());
        pMP->AddObservation(mpCurrentKeyFrame, idx1);
        pMP->AddObservation(pKF2, idx2);
        mpCurrentKeyFrame->AddMapPoint(pMP, idx1);
        pKF2->AddMapPoint(pMP, idx2);
        pMP->ComputeDistinctiveDescriptors();
        pMP->UpdateNormalAndDepth();
        mpAtlas->AddMapPoint(pMP);
        mlpRecentAddedMapPoints.push_back(pMP);
        Created cr;
        cr.pMP = pMP; cr.pKF2 = pKF2; cr.idx1 = idx1; cr.idx2 = idx2; cr.status = status[idx1];
        for (int k = 0; k < 3; ++k) { cr.Xw[k] = Xw[3 * idx1 + k]; cr.normal[k] = nrm[3 * idx1 + k]; }
        cr.maxDistance = maxD[idx1]; cr.minDistance = minD[idx1];
        std::memcpy(cr.descriptor, &mpDesc[(size_t)idx1 * 32], 32);
        created.push_back(cr);
      }
    }
  }

 private:
  template <class SE3>
  static void pose12(const SE3& T, float* out) {   // 3 x 4 row-major [R | t]
    const auto R = T.rotationMatrix();
    const auto t = T.translation();
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) out[4 * r + c] = R(r, c); out[4 * r + 3] = t(r); }
  }
  template <class KP>
  static void keypoint(const KP& k, morb_keypoint& o) {
    o.x = k.pt.x; o.y = k.pt.y; o.size = k.size; o.angle = k.angle; o.response = k.response; o.octave = k.octave; o.class_id = k.class_id;
  }
  int device_;
  ORBmatcher matcher_;
};

}  // namespace ORB_SLAM3
