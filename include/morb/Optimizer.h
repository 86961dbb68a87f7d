// Drop-in adapter: ORB_SLAM3::Optimizer (reference include/Optimizer.h:46-139) over libmorb_hip.so — the two static methods of the
// hot path, PoseOptimization and LocalBundleAdjustment.  As in ORBmatcher.h the arguments are plain views of what the reference
// methods read from Frame / KeyFrame / MapPoint / Map and write back to them; INTEGRATION.md shows the glue inside the reference tree.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../morb_hip.h"
#include "device_buffer.h"

namespace ORB_SLAM3 {

// What Optimizer::PoseOptimization(Frame* pFrame) reads and writes (Optimizer.cc:762-1051): per feature i "mvpMapPoints[i] != NULL",
// (mvKeysUn[i].pt.x, .pt.y, mvuRight[i]), mvInvLevelSigma2[octave], the map point's world position; the camera; in / out the pose
// (Sophus::SE3f as unit quaternion xyzw + translation, :781-783) and mvbOutlier.
struct PoseOptimizationView {
  int N = 0;
  const uint8_t* hasMapPoint = nullptr;   // [N]
  const float* obs = nullptr;             // [N][3]
  const float* invSigma2 = nullptr;       // [N]
  const float* worldPos = nullptr;        // [N][3]
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  float pose[7] = {0, 0, 0, 1, 0, 0, 0};  // in / out
  std::vector<uint8_t> mvbOutlier;        // in / out [N] (empty on input = all false)
  // KannalaBrandt8 rig (pFrame->mpCamera2 != NULL, Optimizer.cc:880-946): features [0, nLeft) on the left camera, the rest on the right one;
  // rig28 = left KB8 parameters (8), right ones (8), rotation (9, row-major) + translation (3) of GetRelativePoseTrl().  NULL = pinhole.
  int nLeft = -1;
  const float* rig28 = nullptr;
};
// What PoseInertialOptimizationLastKeyFrame / LastFrame read and write (Optimizer.cc:4391-5161): the frame's visual edges as above plus
// close[i] (mTrackDepth < 10), the IMU states as 21 floats (Rwb row-major, twb, velocity, gyro bias, acc bias), the preintegrations,
// mImuCalib.mTbc, and the ConstraintPoseImu priors as 246 doubles (state in FP64, then the 15 x 15 H row-major).
struct PoseInertialView {
  int N = 0, nLeft = -1;
  const uint8_t* hasMapPoint = nullptr;
  const float* obs = nullptr;
  const float* invSigma2 = nullptr;
  const float* worldPos = nullptr;
  const uint8_t* close = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  const float* rig28 = nullptr;
  float Tbc12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  float state[21] = {0};         // in / out: the frame
  float otherState[21] = {0};    // LastKeyFrame: pFrame->mpLastKeyFrame (fixed); LastFrame: pFrame->mpPrevFrame (free)
  morb_imu_preintegrated pre{};  // LastKeyFrame: mpImuPreintegrated; LastFrame: mpImuPreintegratedFrame
  morb_imu_preintegrated preKF{};   // LastFrame only: mpImuPreintegrated (the random-walk information)
  double prevPrior[246] = {0};   // LastFrame only: pFp->mpcpi
  double prior[246] = {0};       // out: the frame's new mpcpi
  std::vector<uint8_t> mvbOutlier;
};
// The graph Optimizer::LocalInertialBA assembles (Optimizer.cc:2337-2768), flattened as morb_local_inertial_ba takes it.
struct LocalInertialBAView {
  int nKF = 0, nMP = 0, nE = 0, nI = 0;
  float* kfState = nullptr;            // [nKF][21] in / out
  const uint8_t* kfKind = nullptr;     // [nKF] 0 temporal optimizable, 1 the fixed keyframe before the window, 2 fixed observer
  float* mpPos = nullptr;              // [nMP][3] in / out
  const uint8_t* mpClose = nullptr;
  const int *eKF = nullptr, *eMP = nullptr;
  const float *eObs = nullptr, *eInvSigma2 = nullptr;
  const uint8_t* eRight = nullptr;     // rig only
  const int *iKF1 = nullptr, *iKF2 = nullptr;
  const morb_imu_preintegrated* iPre = nullptr;
  const uint8_t* iRobust = nullptr;
  const float* iInfoScale = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  const float* rig28 = nullptr;
  float Tbc12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  bool bLarge = false;
  std::vector<uint8_t> eraseFlag;      // out [nE]
  int outerIterations = 0, lmTrials = 0;
  bool ok = false;                     // false = "FAIL LOCAL-INERTIAL BA" (nothing to write back)
};
// What the three Optimizer::InertialOptimization overloads read and write (Optimizer.cc:2979-3428), flattened as
// morb_inertial_optimization_batch takes one problem: the keyframes in temporal order (every link joins neighbours), their IMU states, which
// of them carry an EdgeInertialGS to their predecessor and its preintegration, the flags and priors, and Rwg / scale / bg / ba.
struct InertialOptimizationView {
  int nKF = 0;
  float* kfState = nullptr;                        // [nKF][21] in / out: Rwb row-major, twb, velocity, gyro bias, acc bias
  const uint8_t* hasLink = nullptr;                // [nKF]
  const morb_imu_preintegrated* pre = nullptr;     // [nKF]; pre[k] is read where hasLink[k] != 0
  bool bMono = false, bFixedVel = false;           // first overload only
  float priorG = 1e2f, priorA = 1e6f;              // first and second overload
  double global16[16] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0};   // in / out: Rwg (row-major), scale, bg, ba
  std::vector<uint8_t> reintegrate;                // out [nKF]: 1 where the reference calls mpImuPreintegrated->Reintegrate()
  int outerIterations = 0, lmTrials = 0, nLinks = 0;
  bool ok = false;                                 // false: fewer than two keyframes or no link, nothing written
  double chi2[2] = {0, 0};                         // activeRobustChi2 before and after
};
// The graph Optimizer::LocalBundleAdjustment assembles (Optimizer.cc:1058-1351), flattened.
struct LocalBAView {
  int nKF = 0, nMP = 0, nE = 0;
  float* kfPose = nullptr;          // [nKF][7] in / out
  const uint8_t* kfFixed = nullptr; // [nKF]
  float* mpPos = nullptr;           // [nMP][3] in / out
  const int* eKF = nullptr;         // [nE]
  const int* eMP = nullptr;         // [nE]
  const float* eObs = nullptr;      // [nE][3] (x, y, uRight or < 0)
  const float* eInvSigma2 = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  bool inertialMap = false;         // pMap->IsInertial() (:1137)
  const float* rig28 = nullptr;     // KannalaBrandt8 rig (as PoseOptimizationView::rig28): edges with eRight[e] != 0 are right-camera observations
  const uint8_t* eRight = nullptr;
  std::vector<uint8_t> eraseFlag;   // out [nE]: observations the reference erases (:1366-1401)
  int outerIterations = 0, lmTrials = 0;
};
// The graph the welding bundle adjustment of map merging assembles (Optimizer.cc:3459-3648), flattened as morb_merge_bundle_adjustment takes it.
struct MergeBAView {
  int nKF = 0, nMP = 0, nE = 0;
  float* kfPose = nullptr;          // [nKF][7] in / out (free keyframes)
  const uint8_t* kfFixed = nullptr; // [nKF] 1 = vpFixedKF, 0 = vpAdjustKF
  float* mpPos = nullptr;           // [nMP][3] in / out
  const int* eKF = nullptr;         // [nE]
  const int* eMP = nullptr;         // [nE]
  const float* eObs = nullptr;      // [nE][3] (x, y, uRight or < 0); with camL8 every edge is monocular and the third slot is not read
  const float* eInvSigma2 = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  const float* camL8 = nullptr;     // KannalaBrandt8 left camera (fx fy cx cy k0..k3): pKF->mpCamera of every edge
  std::vector<uint8_t> eraseFlag;   // out [nE]: observations the reference erases (:3705-3739)
  std::vector<uint8_t> levelFlag;   // out [nE]: edges put on level 1 between the rounds (:3662-3690)
  int stats[6] = {0, 0, 0, 0, 0, 0};   // out: as morb_merge_bundle_adjustment's stats6
};
// The graph Optimizer::BundleAdjustment assembles over a whole map (Optimizer.cc:113-268), flattened as morb_bundle_adjustment takes it: keyframes by
// ascending mnId, edges by point, within a point by observing keyframe, the left observation before the right camera's.
struct GlobalBAView {
  int nKF = 0, nMP = 0, nE = 0;
  float* kfPose = nullptr;          // [nKF][7] in / out (free keyframes that carry an edge)
  const uint8_t* kfFixed = nullptr; // [nKF] 1 = mnId == GetInitKFid() (:121), and what the caller fixes besides
  float* mpPos = nullptr;           // [nMP][3] in / out (points that carry an edge)
  const int* eKF = nullptr;         // [nE]
  const int* eMP = nullptr;         // [nE]
  const float* eObs = nullptr;      // [nE][3] (x, y, uRight or < 0); with rig28 the third slot is not read
  const float* eInvSigma2 = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  const float* rig28 = nullptr;     // KannalaBrandt8 rig (as LocalBAView::rig28): edges with eRight[e] != 0 are EdgeSE3ProjectXYZToBody
  const uint8_t* eRight = nullptr;
  int stats[4] = {0, 0, 0, 0};      // out: as morb_bundle_adjustment's stats4
  double chi2[2] = {0, 0};          // out: the active robust chi2 before and after
};
// The graph Optimizer::MergeInertialBA assembles (Optimizer.cc:3985-4272), flattened as morb_merge_inertial_ba takes it.
struct MergeInertialBAView {
  int nKF = 0, nMP = 0, nE = 0, nI = 0;
  float* kfState = nullptr;            // [nKF][21] in / out: Rwb row-major, twb, velocity, gyro bias, acc bias (kind 0: all; kind 3: Rwb, twb only)
  const uint8_t* kfKind = nullptr;     // [nKF] 0 free, 15 unknowns (vpOptimizableKFs and the head of the current chain, vpOptimizableCovKFs[0]);
                                       //       1 fixed with an IMU state that enters a link (lFixedKeyFrames); 2 fixed observer;
                                       //       3 free in the pose only (the further vpOptimizableCovKFs, and keyframes with !bImu)
  float* mpPos = nullptr;              // [nMP][3] in / out
  const int* eKF = nullptr;            // [nE]
  const int* eMP = nullptr;            // [nE]
  const float* eObs = nullptr;         // [nE][3] (x, y, uRight or < 0); with rig28 every edge is an EdgeMono(0) and the third slot is not read
  const float* eInvSigma2 = nullptr;   // [nE]
  const int* iKF1 = nullptr;           // [nI] mPrevKF of the link's keyframe (kind 0 or 1)
  const int* iKF2 = nullptr;           // [nI] the keyframe owning iPre[i] (kind 0 or 1)
  const morb_imu_preintegrated* iPre = nullptr;   // [nI] mpImuPreintegrated, after SetNewBias(mPrevKF->GetImuBias()) (:4092)
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  const float* rig28 = nullptr;        // KannalaBrandt8 rig (as LocalInertialBAView::rig28); this function makes left-camera edges only
  float Tbc12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  std::vector<uint8_t> eraseFlag;      // out [nE]: observations the reference erases (:4287-4310)
  int outerIterations = 0, lmTrials = 0;
  bool ran = false;                    // false: *pbStopFlag was set at entry (:4276), nothing written
};
// The graph Optimizer::FullInertialBA assembles over a whole map (Optimizer.cc:392-687), flattened as morb_full_inertial_ba takes it: keyframes by
// ascending mnId, edges by point, within a point by observing keyframe, the left observation before the right camera's.
struct FullInertialBAView {
  int nKF = 0, nMP = 0, nE = 0, nI = 0;
  float* kfState = nullptr;            // [nKF][21] in / out: Rwb row-major, twb, velocity, gyro bias, acc bias (kind 0: all; kind 3: Rwb, twb only)
  const uint8_t* kfKind = nullptr;     // [nKF] 0 free, 15 unknowns (bImu and in a link; 9 with bInit); 1 fixed with an IMU state in a link, 2 fixed observer
                                       //       (bFixLocal); 3 free in the pose only (!bImu, or no link)
  float* mpPos = nullptr;              // [nMP][3] in / out (points that carry an edge)
  const int* eKF = nullptr;            // [nE]
  const int* eMP = nullptr;            // [nE]
  const float* eObs = nullptr;         // [nE][3] (x, y, uRight or < 0); with rig28 the third slot is not read
  const float* eInvSigma2 = nullptr;   // [nE]
  const int* iKF1 = nullptr;           // [nI] mPrevKF of the link's keyframe
  const int* iKF2 = nullptr;           // [nI] the keyframe owning iPre[i]
  const morb_imu_preintegrated* iPre = nullptr;   // [nI] mpImuPreintegrated, after SetNewBias(mPrevKF->GetImuBias()) (:455)
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  const float* rig28 = nullptr;        // KannalaBrandt8 rig (as LocalInertialBAView::rig28): edges with eRight[e] != 0 are EdgeMono(1)
  const uint8_t* eRight = nullptr;
  float Tbc12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  float bias6[6] = {0, 0, 0, 0, 0, 0}; // in / out with bInit: the shared gyro, then accelerometer bias (in: the last keyframe's, pIncKF)
  int stats[4] = {0, 0, 0, 0};         // out: as morb_full_inertial_ba's stats4 (all zero: *pbStopFlag was set at entry, nothing written)
  double chi2[2] = {0, 0};             // out: the active robust chi2 before and after
};

// The graph Optimizer::OptimizeEssentialGraph assembles (Optimizer.cc:1477-1682; the second overload's at :1760-2020), flattened as
// morb_optimize_essential_graph takes it.  Vertices in ascending mnId: the matrix is then a block band plus the loop edges' long rows.
struct EssentialGraphView {
  int nKF = 0, nE = 0, nMP = 0;
  double* kfSim3 = nullptr;            // [nKF][8] in / out: qx qy qz qw tx ty tz s (CorrectedSim3's entry, or the pose with s = 1)
  const uint8_t* kfFlags = nullptr;    // [nKF] bit 0 setFixed(true), bit 1 _fix_scale
  const int* eI = nullptr;             // [nE] setVertex(0, .)
  const int* eJ = nullptr;             // [nE] setVertex(1, .)
  const double* eSji = nullptr;        // [nE][8] the measurement, in the reference's insertion order
  float* mpPos = nullptr;              // [nMP][3] in / out: the point correction of :1707-1731 (nMP = 0: none)
  const int* mpRef = nullptr;          // [nMP] vertex of mnCorrectedReference / of the reference keyframe, -1 = leave the point alone
  int stats[4] = {0, 0, 0, 0};         // out: as morb_optimize_essential_graph's stats4
  double chi2[2] = {0, 0};             // out: the active chi2 before and after
};
// What the second overload of Optimizer::OptimizeEssentialGraph reads and writes (Optimizer.cc:1737-2063), flattened as
// morb_optimize_essential_graph_merge takes it.  Vertices in ascending mnId; the entry applies the good / bad rule to the candidates itself.
struct MergeEssentialGraphView {
  int nKF = 0, nC = 0, nMP = 0;
  const uint8_t* kfLists = nullptr;    // [nKF] bit 0 vpFixedKFs, bit 1 vpFixedCorrectedKFs, bit 2 vpNonFixedKFs: 1, 2, 4 or 6
  float* kfTcw = nullptr;              // [nKF][7] in / out: GetPose(), unit quaternion xyzw and translation
  float* kfTwc = nullptr;              // [nKF][7] in / out: GetPoseInverse()
  float* kfTcwBefMerge = nullptr;      // [nKF][7] in / out: mTcwBefMerge (read for bit 1, written for bit 2)
  float* kfTwcBefMerge = nullptr;      // [nKF][7] in / out: mTwcBefMerge
  const int* cI = nullptr;             // [nC] setVertex(0, .) of a candidate edge, in the insertion order of :1888-1999
  const int* cJ = nullptr;             // [nC] setVertex(1, .)
  uint8_t* cKept = nullptr;            // [nC] out: 1 where both ends are good or both are bad (:1907-1913)
  float* mpPos = nullptr;              // [nMP][3] in / out: the point correction of :2034-2062 (nMP = 0: none)
  const int* mpRef = nullptr;          // [nMP] vertex of the reference keyframe, -1 = leave the point alone
  int stats[4] = {0, 0, 0, 0};         // out: as morb_optimize_essential_graph's stats4
  double chi2[2] = {0, 0};             // out: the active chi2 before and after
};
// The graph Optimizer::OptimizeEssentialGraph4DoF assembles (Optimizer.cc:5194-5426), flattened as morb_optimize_essential_graph_4dof takes
// it.  Vertices in ascending mnId.  A vertex's camera pose and body state are given independently, as ImuCamPose's constructors fill them.
struct PoseGraph4DoFView {
  int nKF = 0, nE = 0, nMP = 0;
  double* kfPose = nullptr;            // [nKF][12] in / out: Rcw[0] row-major, tcw[0]
  const double* kfBody = nullptr;      // [nKF][12] Rwb row-major, twb at entry
  const uint8_t* kfFixed = nullptr;    // [nKF] setFixed(true)
  float Tcb12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};   // mImuCalib.mTcb: R row-major, t
  const int* eI = nullptr;             // [nE] setVertex(0, .)
  const int* eJ = nullptr;             // [nE] setVertex(1, .)
  const double* eTij = nullptr;        // [nE][12] dRij row-major, dtij, in the reference's insertion order
  float* mpPos = nullptr;              // [nMP][3] in / out: the point correction of :5451-5470 (nMP = 0: none)
  const int* mpRef = nullptr;          // [nMP] vertex of the reference keyframe, -1 = leave the point alone
  const double* kfScw = nullptr;       // [nKF][8] vScw at entry (qx qy qz qw tx ty tz s), read when nMP > 0
  int stats[4] = {0, 0, 0, 0};         // out: as morb_optimize_essential_graph_4dof's stats4
  double chi2[2] = {0, 0};             // out: the active chi2 before and after
};
// What Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) reads and writes
// (Optimizer.cc:2065-2322), per KF1 feature i < N as morb_optimize_sim3_batch (include/morb_hip.h) takes it: entry bits (matched, pMP1
// present, pMP1 bad, pMP2 bad), world positions of pMP1 / pMP2, i2, the two keypoints and their mvInvLevelSigma2; the keyframe poses
// (R row-major + t), the cameras (kind 0 pinhole / 1 KB8 + 8 parameters), th2, the flags and g2oS12 (qx qy qz qw tx ty tz s).
struct OptimizeSim3View {
  int N = 0;
  const uint8_t* entry = nullptr;
  const float *Xw1 = nullptr, *Xw2 = nullptr;
  const int* i2 = nullptr;
  const float *obs1 = nullptr, *invSigma2_1 = nullptr, *obs2 = nullptr, *invSigma2_2 = nullptr;
  float T1w[12] = {0}, T2w[12] = {0}, cam1[9] = {0}, cam2[9] = {0};
  float th2 = 10.f;
  bool bFixScale = false, bAllPoints = false;
  double S12[8] = {0, 0, 0, 1, 0, 0, 0, 1};   // in / out (written only when the function reaches its end)
  std::vector<uint8_t> keep;                 // out: vpMatches1[i] != NULL on return
  int stats[8] = {0};                        // out: as morb_optimize_sim3_batch's d_stats (stats[4] = reached the end)
};

// What Tracking::CreateInitialMapMonocular hands its numeric part (Tracking.cc:2345-2430) and gets back, flattened as
// morb_create_initial_map_monocular_batch takes one problem: the two frames' mvKeysUn, vnMatches12 and TwoViewReconstruction's T21, vP3D,
// vbTriangulated; mvLevelSigma2 / mvScaleFactors and the camera; out: keyframe 2's pose and, by frame-1 keypoint, the map points' fields.
struct InitialMapView {
  int n1 = 0, n2 = 0;
  const morb_keypoint *keysUn1 = nullptr, *keysUn2 = nullptr;   // [n1], [n2]
  const int* matches12 = nullptr;                               // [n1]: frame-2 keypoint or negative
  const uint8_t* triangulated = nullptr;                        // [n1]
  const float* P3D = nullptr;                                   // [n1][3]
  float T21[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};         // in: R row-major, then t
  int nlevels = 0;
  float scaleFactors[16] = {0}, levelSigma2[16] = {0};
  float cam8[8] = {0};                                          // fx fy cx cy, then k0..k3 when kb8
  bool kb8 = false;
  float depthScale = 1.f;                                       // 1; 4 for IMU-monocular; 0 = no scaling (what BundleAdjustment itself leaves)
  int minTracked = 50;
  int status = 0;                                               // out: 1 = ok, else the reset reasons as bits (2 negative median, 4 too few points)
  float Tcw2[12] = {0};
  std::vector<float> mpPos, mpNormal, mpDist;                   // [n1][3], [n1][3], [n1][2] (mfMaxDistance, mfMinDistance)
  std::vector<uint8_t> hasMP;                                   // [n1]
  int nPoints = 0, outerIterations = 0, lmTrials = 0;
  bool stopSeen = false;
  double chi2[2] = {0, 0};
  float medianDepth = 0.f;
};

class Optimizer {
  friend class Sim3Solver;    // Sim3Solver.h: the solver runs on the kLoopClosing handle, under its mutex
  friend class MLPnPsolver;   // MLPnPsolver.h: the relocalisation solver runs on the kTracking handle, under its mutex
  friend class TwoViewReconstruction;   // TwoViewReconstruction.h: the monocular initialisation, on the kTracking handle as well

 public:
  // static int PoseOptimization(Frame* pFrame)  Optimizer.h:86 -> number of inliers
  static int PoseOptimization(PoseOptimizationView& f, int device = 0) {
    if (f.N <= 0) return 0;
    const int N = f.N;
    Slot& o = slot(device, kTracking);
    std::lock_guard<std::mutex> lock(o.mu);   // one caller per handle at a time (Tracking's handle is not LocalMapping's: see slot())
    Call c(device, morb_optimizer_stream(o.h));   // uploads, the kernel, downloads: this handle's stream, never the null stream
    const int* d_count = c.in(&N, 1);
    const uint8_t* d_hasMP = c.in(f.hasMapPoint, N);
    const float *d_obs = c.in(f.obs, (size_t)N * 3), *d_invSigma2 = c.in(f.invSigma2, N), *d_Xw = c.in(f.worldPos, (size_t)N * 3);
    float* d_pose = c.in(f.pose, 7);
    // mvbOutlier is only written for features that hold a map point (Optimizer.cc:817, :860): the others keep what they had
    uint8_t* d_outlier = (int)f.mvbOutlier.size() == N ? c.in(f.mvbOutlier.data(), N) : c.out_filled<uint8_t>(N, 0);
    int* d_nInliers = c.out<int>(1);
    if (f.rig28) {
      float trl7[7];
      rot_to_pose7(f.rig28 + 16, trl7);
      const int* d_nLeft = c.in(&f.nLeft, 1);
      check(morb_pose_optimization_fisheye_batch(o.h, 1, N, d_count, d_nLeft, d_hasMP, d_obs, d_invSigma2, d_Xw, f.rig28, f.rig28 + 8, trl7, d_pose,
                                                 d_outlier, d_nInliers, nullptr, nullptr));
    } else
    check(morb_pose_optimization_batch(o.h, 1, N, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, f.fx, f.fy, f.cx, f.cy, f.mbf, d_pose, d_outlier,
                                       d_nInliers, nullptr, nullptr));
    c.wait();   // (the tracking handle's stream: a LocalBundleAdjustment on the mapping handle keeps running)
    c.fetch(d_pose, f.pose, 7);
    f.mvbOutlier = c.fetch(d_outlier, N);
    return c.fetch(d_nInliers, 1)[0];
  }

  // static void LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int&, int&, int&, int&)  Optimizer.h:67-69.  pbStopFlag is
  // the reference's own bool (LocalMapping::mbAbortBA): it is polled at every LM iteration and trial.
  static void LocalBundleAdjustment(LocalBAView& g, bool* pbStopFlag, int device = 0) {
    static_assert(sizeof(bool) == 1, "pbStopFlag is read as one byte");
    g.eraseFlag.assign(g.nE, 0);
    int stats[2] = {0, 0};
    Slot& o = slot(device, kMapping);
    std::lock_guard<std::mutex> lock(o.mu);   // the one-shot entry point works in the handle's grow-only workspace
    morb_adapter::hip_check(hipSetDevice(device), "hipSetDevice");
    if (g.rig28) {
      float trl7[7];
      rot_to_pose7(g.rig28 + 16, trl7);
      std::vector<float> obs2((size_t)g.nE * 2);
      for (int e = 0; e < g.nE; ++e) { obs2[2 * e] = g.eObs[3 * e]; obs2[2 * e + 1] = g.eObs[3 * e + 1]; }
      check(morb_local_bundle_adjustment_fisheye(o.h, g.nKF, g.kfPose, g.kfFixed, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, obs2.data(), g.eRight, g.eInvSigma2,
                                                 g.rig28, g.rig28 + 8, trl7, g.inertialMap ? 1 : 0, reinterpret_cast<const unsigned char*>(pbStopFlag),
                                                 g.eraseFlag.data(), stats));
    } else
    check(morb_local_bundle_adjustment(o.h, g.nKF, g.kfPose, g.kfFixed, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, g.eObs, g.eInvSigma2, g.fx,
                                       g.fy, g.cx, g.cy, g.mbf, g.inertialMap ? 1 : 0, reinterpret_cast<const unsigned char*>(pbStopFlag),
                                       g.eraseFlag.data(), stats));
    g.outerIterations = stats[0]; g.lmTrials = stats[1];
  }

  // void static LocalBundleAdjustment(KeyFrame* pMainKF, vector<KeyFrame*> vpAdjustKF, vector<KeyFrame*> vpFixedKF, bool* pbStopFlag)  Optimizer.h:115-118:
  // the welding bundle adjustment of LoopClosing::MergeLocal (LoopClosing.cc:1652), on the loop-closing handle.  pbStopFlag is the caller's own bool,
  // read at entry, polled at every LM iteration and trial and between the two rounds.
  static void LocalBundleAdjustment(MergeBAView& g, bool* pbStopFlag, int device = 0) {
    static_assert(sizeof(bool) == 1, "pbStopFlag is read as one byte");
    g.eraseFlag.assign(g.nE, 0); g.levelFlag.assign(g.nE, 0);
    Slot& o = slot(device, kLoopClosing);
    std::lock_guard<std::mutex> lock(o.mu);   // the entry point works in the handle's grow-only workspace
    morb_adapter::hip_check(hipSetDevice(device), "hipSetDevice");
    const uint8_t* stop = reinterpret_cast<const uint8_t*>(pbStopFlag);
    if (g.camL8) {
      std::vector<float> obs2((size_t)g.nE * 2);
      for (int e = 0; e < g.nE; ++e) { obs2[2 * e] = g.eObs[3 * e]; obs2[2 * e + 1] = g.eObs[3 * e + 1]; }
      check(morb_merge_bundle_adjustment_fisheye(o.h, g.nKF, g.kfPose, g.kfFixed, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, obs2.data(), g.eInvSigma2, g.camL8,
                                                 stop, g.eraseFlag.data(), g.levelFlag.data(), g.stats));
    } else
    check(morb_merge_bundle_adjustment(o.h, g.nKF, g.kfPose, g.kfFixed, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, g.eObs, g.eInvSigma2, g.fx, g.fy, g.cx,
                                       g.cy, g.mbf, stop, g.eraseFlag.data(), g.levelFlag.data(), g.stats));
  }

  // void static BundleAdjustment(const vector<KeyFrame*>& vpKF, const vector<MapPoint*>& vpMP, int nIterations, bool* pbStopFlag, const unsigned long
  // nLoopKF, const bool bRobust)  Optimizer.h:49-52 over a whole map: the global bundle adjustment LoopClosing::RunGlobalBundleAdjustment starts
  // (LoopClosing.cc:2302), on the loop-closing handle.  pbStopFlag is the caller's own bool (mbStopGBA), read at entry and polled at every LM
  // iteration and trial.
  static void BundleAdjustment(GlobalBAView& g, int nIterations, bool bRobust, bool* pbStopFlag, int device = 0) {
    static_assert(sizeof(bool) == 1, "pbStopFlag is read as one byte");
    Slot& o = slot(device, kLoopClosing);
    std::lock_guard<std::mutex> lock(o.mu);   // the entry point works in the handle's grow-only workspace
    morb_adapter::hip_check(hipSetDevice(device), "hipSetDevice");
    const uint8_t* stop = reinterpret_cast<const uint8_t*>(pbStopFlag);
    if (g.rig28) {
      float trl7[7];
      rot_to_pose7(g.rig28 + 16, trl7);
      std::vector<float> obs2((size_t)g.nE * 2);
      for (int e = 0; e < g.nE; ++e) { obs2[2 * e] = g.eObs[3 * e]; obs2[2 * e + 1] = g.eObs[3 * e + 1]; }
      check(morb_bundle_adjustment_fisheye(o.h, g.nKF, g.kfPose, g.kfFixed, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, obs2.data(), g.eRight, g.eInvSigma2, g.rig28,
                                           g.rig28 + 8, trl7, nIterations, bRobust ? 1 : 0, stop, g.stats, g.chi2));
    } else
    check(morb_bundle_adjustment(o.h, g.nKF, g.kfPose, g.kfFixed, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, g.eObs, g.eInvSigma2, g.fx, g.fy, g.cx, g.cy,
                                 g.mbf, nIterations, bRobust ? 1 : 0, stop, g.stats, g.chi2));
  }

  // static void OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3, const
  // KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>& LoopConnections, const bool& bFixScale)  Optimizer.h:76-81.  The
  // entry takes host arrays and stages them itself.
  static void OptimizeEssentialGraph(EssentialGraphView& g, int device = 0) {
    Slot& o = slot(device, kLoopClosing);
    std::lock_guard<std::mutex> lock(o.mu);   // the entry point works in the handle's grow-only workspace
    morb_adapter::hip_check(hipSetDevice(device), "hipSetDevice");
    check(morb_optimize_essential_graph(o.h, g.nKF, g.kfSim3, g.kfFlags, g.nE, g.eI, g.eJ, g.eSji, g.nMP, g.mpPos, g.mpRef, g.stats, g.chi2));
  }

  // static void OptimizeEssentialGraph(KeyFrame* pCurKF, vector<KeyFrame*>& vpFixedKFs, vector<KeyFrame*>& vpFixedCorrectedKFs,
  // vector<KeyFrame*>& vpNonFixedKFs, vector<MapPoint*>& vpNonCorrectedMPs)  Optimizer.h:82-86: map merging's pose graph, on the loop-closing
  // handle (LoopClosing's thread runs loops and merges one after the other).
  static void OptimizeEssentialGraph(MergeEssentialGraphView& g, int device = 0) {
    Slot& o = slot(device, kLoopClosing);
    std::lock_guard<std::mutex> lock(o.mu);
    morb_adapter::hip_check(hipSetDevice(device), "hipSetDevice");
    check(morb_optimize_essential_graph_merge(o.h, g.nKF, g.kfLists, g.kfTcw, g.kfTwc, g.kfTcwBefMerge, g.kfTwcBefMerge, g.nC, g.cI, g.cJ, g.cKept, g.nMP, g.mpPos,
                                              g.mpRef, g.stats, g.chi2));
  }

  // static void OptimizeEssentialGraph4DoF(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3, const
  // KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>& LoopConnections)  Optimizer.h:89-94.  It shares the loop-closing
  // handle's workspace with OptimizeEssentialGraph; the handle's mutex keeps the two apart.
  static void OptimizeEssentialGraph4DoF(PoseGraph4DoFView& g, int device = 0) {
    Slot& o = slot(device, kLoopClosing);
    std::lock_guard<std::mutex> lock(o.mu);
    morb_adapter::hip_check(hipSetDevice(device), "hipSetDevice");
    check(morb_optimize_essential_graph_4dof(o.h, g.nKF, g.kfPose, g.kfBody, g.kfFixed, g.Tcb12, g.nE, g.eI, g.eJ, g.eTij, g.nMP, g.mpPos, g.mpRef, g.kfScw,
                                             g.stats, g.chi2));
  }

  // static int PoseInertialOptimizationLastKeyFrame(Frame* pFrame, bool bRecInit)  Optimizer.h:87 / ...LastFrame  Optimizer.h:88: one frame per call
  static int PoseInertialOptimizationLastKeyFrame(PoseInertialView& v, bool bRecInit = false, int device = 0) { return pose_inertial(v, bRecInit, false, device); }
  static int PoseInertialOptimizationLastFrame(PoseInertialView& v, bool bRecInit = false, int device = 0) { return pose_inertial(v, bRecInit, true, device); }

  // static void LocalInertialBA(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int&, int&, int&, int&, bool bLarge, bool bRecInit)  Optimizer.h:97-101
  // (bRecInit is folded into iRobust by the caller, Optimizer.cc:2563)
  static void LocalInertialBA(LocalInertialBAView& g, int device = 0) {
    g.eraseFlag.assign(g.nE, 0);
    int stats[3] = {0, 0, 0};
    Slot& o = slot(device, kMapping);
    std::lock_guard<std::mutex> lock(o.mu);
    morb_adapter::hip_check(hipSetDevice(device), "hipSetDevice");
    if (g.rig28)
      check(morb_local_inertial_ba_fisheye(o.h, g.nKF, g.kfState, g.kfKind, g.nMP, g.mpPos, g.mpClose, g.nE, g.eKF, g.eMP, g.eObs, g.eRight, g.eInvSigma2, g.nI,
                                           g.iKF1, g.iKF2, g.iPre, g.iRobust, g.iInfoScale, g.rig28, g.Tbc12, g.bLarge ? 1 : 0, g.eraseFlag.data(), stats));
    else
      check(morb_local_inertial_ba(o.h, g.nKF, g.kfState, g.kfKind, g.nMP, g.mpPos, g.mpClose, g.nE, g.eKF, g.eMP, g.eObs, g.eInvSigma2, g.nI, g.iKF1, g.iKF2,
                                   g.iPre, g.iRobust, g.iInfoScale, g.fx, g.fy, g.cx, g.cy, g.mbf, g.Tbc12, g.bLarge ? 1 : 0, g.eraseFlag.data(), stats));
    g.outerIterations = stats[0]; g.lmTrials = stats[1]; g.ok = stats[2] != 0;
  }

  // void static MergeInertialBA(KeyFrame* pCurrKF, KeyFrame* pMergeKF, bool* pbStopFlag, Map* pMap, LoopClosing::KeyFrameAndPose& corrPoses)
  // Optimizer.h:110-112: the welding bundle adjustment of an inertial map merge (LoopClosing.cc:1649-1650, :2099), on the loop-closing handle.
  // pbStopFlag is the caller's own bool, read at entry and polled at every LM iteration and trial.
  static void MergeInertialBA(MergeInertialBAView& g, bool* pbStopFlag, int device = 0) {
    static_assert(sizeof(bool) == 1, "pbStopFlag is read as one byte");
    g.eraseFlag.assign(g.nE, 0);
    int stats[3] = {0, 0, 0};
    Slot& o = slot(device, kLoopClosing);
    std::lock_guard<std::mutex> lock(o.mu);   // the entry point works in the handle's grow-only workspace
    morb_adapter::hip_check(hipSetDevice(device), "hipSetDevice");
    const uint8_t* stop = reinterpret_cast<const uint8_t*>(pbStopFlag);
    if (g.rig28)
      check(morb_merge_inertial_ba_fisheye(o.h, g.nKF, g.kfState, g.kfKind, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, g.eObs, g.eInvSigma2, g.nI, g.iKF1, g.iKF2,
                                           g.iPre, g.rig28, g.Tbc12, stop, g.eraseFlag.data(), stats));
    else
      check(morb_merge_inertial_ba(o.h, g.nKF, g.kfState, g.kfKind, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, g.eObs, g.eInvSigma2, g.nI, g.iKF1, g.iKF2, g.iPre,
                                   g.fx, g.fy, g.cx, g.cy, g.mbf, g.Tbc12, stop, g.eraseFlag.data(), stats));
    g.outerIterations = stats[0]; g.lmTrials = stats[1]; g.ran = stats[2] != 0;
  }

  // void static FullInertialBA(Map* pMap, int its, const bool bFixLocal, const unsigned long nLoopKF, bool* pbStopFlag, bool bInit, float priorG,
  // float priorA, Eigen::VectorXd* vSingVal, bool* bHess)  Optimizer.h:55-58: the inertial whole-map bundle adjustment, on the handle of the role
  // that calls it (LocalMapping::InitializeIMU: kMapping; LoopClosing::RunGlobalBundleAdjustment: kLoopClosing).  pbStopFlag is the caller's own
  // bool (or NULL), read at entry and polled at every LM iteration and trial.
  enum Role { kTracking = 0, kMapping = 1, kLoopClosing = 2 };   // (the roles: see optimizer() below)
  static void FullInertialBA(FullInertialBAView& g, int its, bool bInit, float priorG, float priorA, bool* pbStopFlag, Role role, int device = 0) {
    static_assert(sizeof(bool) == 1, "pbStopFlag is read as one byte");
    Slot& o = slot(device, role);
    std::lock_guard<std::mutex> lock(o.mu);   // the entry point works in the handle's grow-only workspace
    morb_adapter::hip_check(hipSetDevice(device), "hipSetDevice");
    const uint8_t* stop = reinterpret_cast<const uint8_t*>(pbStopFlag);
    if (g.rig28)
      check(morb_full_inertial_ba_fisheye(o.h, g.nKF, g.kfState, g.kfKind, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, g.eObs, g.eRight, g.eInvSigma2, g.nI, g.iKF1,
                                          g.iKF2, g.iPre, g.rig28, g.Tbc12, its, bInit ? 1 : 0, priorG, priorA, g.bias6, stop, g.stats, g.chi2));
    else
      check(morb_full_inertial_ba(o.h, g.nKF, g.kfState, g.kfKind, g.nMP, g.mpPos, g.nE, g.eKF, g.eMP, g.eObs, g.eInvSigma2, g.nI, g.iKF1, g.iKF2, g.iPre,
                                  g.fx, g.fy, g.cx, g.cy, g.mbf, g.Tbc12, its, bInit ? 1 : 0, priorG, priorA, g.bias6, stop, g.stats, g.chi2));
  }

  // void static InertialOptimization(Map*, ...)  Optimizer.h:103-112 in its three overloads: mode 0 = (Rwg, scale, bg, ba, bMono, covInertial,
  // bFixedVel, bGauss, priorG, priorA), 1 = (bg, ba, priorG, priorA), 2 = (Rwg, scale).  One problem through morb_inertial_optimization_batch:
  // modes 0 and 2 (LocalMapping) on the mapping handle, mode 1 (LoopClosing's merge) on the loop-closing handle.
  static void InertialOptimization(InertialOptimizationView& v, int mode, int device = 0) {
    v.reintegrate.assign(v.nKF > 0 ? v.nKF : 0, 0);
    v.outerIterations = v.lmTrials = v.nLinks = 0; v.ok = false; v.chi2[0] = v.chi2[1] = 0;
    if (v.nKF < 2) return;
    const int N = v.nKF;
    Slot& o = slot(device, mode == 1 ? kLoopClosing : kMapping);
    std::lock_guard<std::mutex> lock(o.mu);
    Call c(device, morb_optimizer_stream(o.h));
    const int start[2] = {0, N}, flags = (v.bMono ? 1 : 0) | (v.bFixedVel ? 2 : 0);
    const float prior2[2] = {v.priorG, v.priorA};
    const int *d_start = c.in(start, 2), *d_flags = c.in(&flags, 1);
    float* d_state = c.in(v.kfState, (size_t)N * 21);
    const uint8_t* d_hasLink = c.in(v.hasLink, N);
    const morb_imu_preintegrated* d_pre = c.in(v.pre, N);
    const float* d_prior2 = c.in(prior2, 2);
    double* d_global = c.in(v.global16, 16);
    uint8_t* d_reint = c.out_filled<uint8_t>(N, 0);
    int* d_stats = c.out<int>(4);
    double* d_chi2 = c.out_filled<double>(2, 0);
    check(morb_inertial_optimization_batch(o.h, 1, N, d_start, d_state, d_hasLink, d_pre, mode, d_flags, d_prior2, d_global, d_reint, d_stats, d_chi2,
                                           nullptr));
    c.wait();
    const std::vector<int> st = c.fetch(d_stats, 4);
    v.outerIterations = st[0]; v.lmTrials = st[1]; v.ok = st[2] != 0; v.nLinks = st[3];
    if (!v.ok) return;
    c.fetch(d_state, v.kfState, (size_t)N * 21); c.fetch(d_global, v.global16, 16); c.fetch(d_chi2, v.chi2, 2);
    v.reintegrate = c.fetch(d_reint, N);
  }

  // static int OptimizeSim3(KeyFrame*, KeyFrame*, vector<MapPoint*>&, g2o::Sim3&, float th2, bool bFixScale, Matrix<double,7,7>&, bool bAllPoints)
  // Optimizer.h:97-101 -> nIn (0 on the early return).  One problem through morb_optimize_sim3_batch on the loop-closing handle.
  static int OptimizeSim3(OptimizeSim3View& v, int device = 0) {
    const int N = v.N;
    v.keep.assign(N > 0 ? N : 0, 0);
    for (int i = 0; i < N; ++i) v.keep[i] = v.entry[i] & 1;
    for (int& s : v.stats) s = 0;
    if (N <= 0) return 0;
    Slot& o = slot(device, kLoopClosing);
    std::lock_guard<std::mutex> lock(o.mu);
    Call c(device, morb_optimizer_stream(o.h));
    const uint8_t fix = v.bFixScale ? 1 : 0;
    const int* d_count = c.in(&N, 1);
    const uint8_t* d_entry = c.in(v.entry, N);
    const float *d_Xw1 = c.in(v.Xw1, (size_t)N * 3), *d_Xw2 = c.in(v.Xw2, (size_t)N * 3);
    const int* d_i2 = c.in(v.i2, N);
    const float *d_obs1 = c.in(v.obs1, (size_t)N * 2), *d_invSigma2_1 = c.in(v.invSigma2_1, N);
    const float *d_obs2 = c.in(v.obs2, (size_t)N * 2), *d_invSigma2_2 = c.in(v.invSigma2_2, N);
    const float *d_T1w = c.in(v.T1w, 12), *d_T2w = c.in(v.T2w, 12), *d_cam1 = c.in(v.cam1, 9), *d_cam2 = c.in(v.cam2, 9), *d_th2 = c.in(&v.th2, 1);
    const uint8_t* d_fixScale = c.in(&fix, 1);
    double* d_S12 = c.in(v.S12, 8);
    uint8_t* d_keep = c.out<uint8_t>(N);
    int *d_nIn = c.out<int>(1), *d_stats = c.out<int>(8);
    check(morb_optimize_sim3_batch(o.h, 1, N, d_count, d_entry, d_Xw1, d_Xw2, d_i2, d_obs1, d_invSigma2_1, d_obs2, d_invSigma2_2, d_T1w, d_T2w, d_cam1,
                                   d_cam2, d_th2, d_fixScale, v.bAllPoints ? 1 : 0, d_S12, d_keep, d_nIn, d_stats, nullptr));
    c.wait();
    c.fetch(d_S12, v.S12, 8);
    v.keep = c.fetch(d_keep, N);
    c.fetch(d_stats, v.stats, 8);
    return c.fetch(d_nIn, 1)[0];
  }

  // void static BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)  Optimizer.h:46-50 on the map of a monocular
  // initialisation: two keyframes, the first fixed, every point seen by both.  One problem through morb_create_initial_map_monocular_batch with
  // the view's depthScale and minTracked (0 = the bare bundle adjustment), on the tracking handle: Tracking::CreateInitialMapMonocular calls it.
  static void BundleAdjustment(InitialMapView& v, int nIterations, bool bRobust, int device = 0, const bool* pbStopFlag = nullptr) {
    const int n1 = v.n1 > 0 ? v.n1 : 0, n2 = v.n2 > 0 ? v.n2 : 0, cap = std::max(std::max(n1, n2), 1);
    v.mpPos.assign((size_t)n1 * 3, 0.f); v.mpNormal.assign((size_t)n1 * 3, 0.f); v.mpDist.assign((size_t)n1 * 2, 0.f); v.hasMP.assign(n1, 0);
    morb_frame_params P = {};
    P.fx = v.cam8[0]; P.fy = v.cam8[1]; P.cx = v.cam8[2]; P.cy = v.cam8[3];
    P.nlevels = v.nlevels;
    for (int k = 0; k < 16; ++k) { P.scaleFactors[k] = v.scaleFactors[k]; P.levelSigma2[k] = v.levelSigma2[k]; }
    std::vector<morb_keypoint> pool((size_t)2 * cap);
    for (int i = 0; i < n1; ++i) pool[i] = v.keysUn1[i];
    for (int i = 0; i < n2; ++i) pool[(size_t)cap + i] = v.keysUn2[i];
    std::vector<int> m12(cap, -1);
    std::vector<uint8_t> tri(cap, 0);
    std::vector<float> p3d((size_t)cap * 3, 0.f);
    for (int i = 0; i < n1; ++i) { m12[i] = v.matches12[i]; tri[i] = v.triangulated[i]; for (int k = 0; k < 3; ++k) p3d[3 * (size_t)i + k] = v.P3D[3 * (size_t)i + k]; }
    const int img[2] = {0, 1}, count[2] = {n1, n2}, ok = 1;
    const unsigned char stop = pbStopFlag && *pbStopFlag ? 1 : 0;   // (sampled at the call: the device reads its copy)
    Slot& o = slot(device, kTracking);
    std::lock_guard<std::mutex> lock(o.mu);
    Call c(device, morb_optimizer_stream(o.h));
    const int *d_img = c.in(img, 2), *d_count = c.in(count, 2), *d_m12 = c.in(m12.data(), cap), *d_ok = c.in(&ok, 1);
    const morb_keypoint* d_kps = c.in(pool.data(), pool.size());
    const float *d_T21 = c.in(v.T21, 12), *d_P3D = c.in(p3d.data(), p3d.size());
    const uint8_t* d_tri = c.in(tri.data(), cap);
    const unsigned char* d_stop = pbStopFlag ? c.in(&stop, 1) : nullptr;
    int *d_status = c.out<int>(1), *d_stats = c.out<int>(4);
    float *d_Tcw2 = c.out<float>(12), *d_pos = c.out<float>((size_t)cap * 3), *d_nrm = c.out<float>((size_t)cap * 3), *d_dist = c.out<float>((size_t)cap * 2),
          *d_median = c.out<float>(1);
    uint8_t* d_has = c.out<uint8_t>(cap);
    double* d_chi2 = c.out<double>(2);
    check(morb_create_initial_map_monocular_batch(o.h, &P, v.cam8, v.kb8 ? 1 : 0, 1, cap, d_img, d_img + 1, d_count, d_kps, d_m12, d_ok, d_T21, d_P3D, d_tri,
                                                  nIterations, bRobust ? 1 : 0, v.depthScale, v.minTracked, d_stop, d_status, d_Tcw2, d_pos, d_nrm, d_dist,
                                                  d_has, d_stats, d_chi2, d_median, nullptr));
    c.wait();
    v.status = c.fetch(d_status, 1)[0];
    const std::vector<int> st = c.fetch(d_stats, 4);
    v.nPoints = st[0]; v.outerIterations = st[1]; v.lmTrials = st[2]; v.stopSeen = st[3] != 0;
    c.fetch(d_Tcw2, v.Tcw2, 12); c.fetch(d_chi2, v.chi2, 2); c.fetch(d_median, &v.medianDepth, 1);
    if (n1 > 0) { c.fetch(d_pos, v.mpPos.data(), (size_t)n1 * 3); c.fetch(d_nrm, v.mpNormal.data(), (size_t)n1 * 3); c.fetch(d_dist, v.mpDist.data(), (size_t)n1 * 2);
                  c.fetch(d_has, v.hasMP.data(), n1); }
  }
  // The numeric part of void Tracking::CreateInitialMapMonocular() (Tracking.cc:2394-2429) in one call: GlobalBundleAdjustemnt(map, 20), the median
  // depth, the reset test, the rescaling and UpdateNormalAndDepth.  Returns false for "Wrong initialization, reseting..." (v.status says why).
  static bool CreateInitialMapMonocular(InitialMapView& v, bool bImuMonocular = false, int device = 0) {
    v.depthScale = bImuMonocular ? 4.f : 1.f;
    v.minTracked = 50;
    BundleAdjustment(v, 20, true, device);
    return v.status == 1;
  }

  // ---- the reference's own signatures (include/Optimizer.h:67-101) as static member templates: the call sites of src/Tracking.cc and
  // src/LocalMapping.cc compile unchanged (definitions: Optimizer_reference.h, included below) ----
  template <class FrameT> static int PoseOptimization(FrameT* pFrame);
  template <class FrameT> static int PoseInertialOptimizationLastKeyFrame(FrameT* pFrame, bool bRecInit = false);
  template <class FrameT> static int PoseInertialOptimizationLastFrame(FrameT* pFrame, bool bRecInit = false);
  template <class KF, class MapT>
  static void LocalBundleAdjustment(KF* pKF, bool* pbStopFlag, MapT* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges);
  // (include/Optimizer.h:115-118; call site LoopClosing.cc:1652-1653)
  template <class KF>
  static void LocalBundleAdjustment(KF* pMainKF, std::vector<KF*> vpAdjustKF, std::vector<KF*> vpFixedKF, bool* pbStopFlag);
  template <class KF, class MapT>
  static void LocalInertialBA(KF* pKF, bool* pbStopFlag, MapT* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges, bool bLarge = false,
                              bool bRecInit = false);
  // (include/Optimizer.h:110-112; call sites LoopClosing.cc:1649-1650, :2099)
  template <class KF, class MapT, class CorrMap>
  static void MergeInertialBA(KF* pCurrKF, KF* pMergeKF, bool* pbStopFlag, MapT* pMap, CorrMap& corrPoses);
  template <class KF, class MP, class Sim3T, class Mat77>
  static int OptimizeSim3(KF* pKF1, KF* pKF2, std::vector<MP*>& vpMatches1, Sim3T& g2oS12, const float th2, const bool bFixScale, Mat77& mAcumHessian,
                          const bool bAllPoints = false);

  // (include/Optimizer.h:76-81; call site LoopClosing.cc:1206-1208): overload 1 of OptimizeEssentialGraph.  CorrMap = LoopClosing::KeyFrameAndPose
  // (KeyFrame* -> g2o::Sim3), ConnMap = map<KeyFrame*, set<KeyFrame*>>
  template <class MapT, class KF, class CorrMap, class ConnMap>
  static void OptimizeEssentialGraph(MapT* pMap, KF* pLoopKF, KF* pCurKF, const CorrMap& NonCorrectedSim3, const CorrMap& CorrectedSim3,
                                     const ConnMap& LoopConnections, const bool& bFixScale);

  // (include/Optimizer.h:82-86; call site LoopClosing.cc:1747-1749): overload 2 of OptimizeEssentialGraph, the pose graph of a map merge
  template <class KF, class MP>
  static void OptimizeEssentialGraph(KF* pCurKF, std::vector<KF*>& vpFixedKFs, std::vector<KF*>& vpFixedCorrectedKFs, std::vector<KF*>& vpNonFixedKFs,
                                     std::vector<MP*>& vpNonCorrectedMPs);

  // (include/Optimizer.h:89-94; call site LoopClosing.cc:1201-1203): the pose graph of an inertial map whose IMU is initialised
  template <class MapT, class KF, class CorrMap, class ConnMap>
  static void OptimizeEssentialGraph4DoF(MapT* pMap, KF* pLoopKF, KF* pCurKF, const CorrMap& NonCorrectedSim3, const CorrMap& CorrectedSim3,
                                         const ConnMap& LoopConnections);

  // (include/Optimizer.h:46-53; call site Tracking.cc:2398) on the map of a monocular initialisation; any other map shape throws, or, with
  // MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT defined, goes to WholeMapBundleAdjustment
  template <class MapT>
  static void GlobalBundleAdjustemnt(MapT* pMap, int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true);
  template <class KF, class MP>
  static void BundleAdjustment(const std::vector<KF*>& vpKFs, const std::vector<MP*>& vpMP, int nIterations = 5, bool* pbStopFlag = NULL,
                               const unsigned long nLoopKF = 0, const bool bRobust = true);

  // the same function over any map (morb_bundle_adjustment*): what BundleAdjustment<KF, MP> hands a map that is not the initial-map shape to when
  // MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT is defined before this header is included (call site LoopClosing.cc:2302)
  template <class KF, class MP>
  static void WholeMapBundleAdjustment(const std::vector<KF*>& vpKFs, const std::vector<MP*>& vpMP, int nIterations = 5, bool* pbStopFlag = NULL,
                                       const unsigned long nLoopKF = 0, const bool bRobust = true);

  // (include/Optimizer.h:55-58; call sites LoopClosing.cc:2305 and LocalMapping.cc:1244-1249).  VecX stands for Eigen::VectorXd: vSingVal and
  // bHess are never touched by the reference either.
  template <class MapT, class VecX = void>
  static void FullInertialBA(MapT* pMap, int its, const bool bFixLocal = false, const unsigned long nLoopId = 0, bool* pbStopFlag = NULL, bool bInit = false,
                             float priorG = 1e2, float priorA = 1e6, VecX* vSingVal = NULL, bool* bHess = NULL);

  // (include/Optimizer.h:103-112; call sites LocalMapping.cc:1205, :1391 and LoopClosing.cc:1902)
  template <class MapT, class Mat3d, class Vec3d, class MatXd>
  static void InertialOptimization(MapT* pMap, Mat3d& Rwg, double& scale, Vec3d& bg, Vec3d& ba, bool bMono, MatXd& covInertial, bool bFixedVel = false,
                                   bool bGauss = false, float priorG = 1e2, float priorA = 1e6);
  template <class MapT, class Vec3d>
  static void InertialOptimization(MapT* pMap, Vec3d& bg, Vec3d& ba, float priorG = 1e2, float priorA = 1e6);
  template <class MapT, class Mat3d>
  static void InertialOptimization(MapT* pMap, Mat3d& Rwg, double& scale);

  // The reference's Optimizer is a stateless static class entered concurrently from Tracking (PoseOptimization, every frame) and from
  // LocalMapping (LocalBundleAdjustment, hundreds of milliseconds of LM trials): each role has its own handle — own stream, own
  // workspace — per device, created once (std::call_once), so a tracked frame never queues behind local-mapping trials; a mutex per
  // handle serialises callers of the same role.
  static morb_optimizer* optimizer(int device = 0, Role role = kTracking) { return slot(device, role).h; }

 private:
  template <class FrameT> static void write_back_inertial(FrameT* pFrame, const PoseInertialView& v);
  template <class MapT, class Fill, class Back> static void inertial_optimization_on_map(MapT* pMap, int mode, Fill fill, Back back);
  template <class SE3> static SE3 se3_from_matrix(const double R[9], const double t[3]);
  template <class KF, class MP>
  static bool initial_map_bundle_adjustment(const std::vector<KF*>& vpKFs, const std::vector<MP*>& vpMP, int nIterations, bool* pbStopFlag,
                                            const unsigned long nLoopKF, const bool bRobust, std::string* whyNot);
  // rotation (9, row-major) + translation (3) -> unit quaternion xyzw + translation (the *_fisheye pose entries take Trl that way)
  static void rot_to_pose7(const float* Rt12, float out[7]) {
    const float* R = Rt12;
    const float tr = R[0] + R[4] + R[8];
    float q[4];   // x y z w
    if (tr > 0.f) { const float s = std::sqrt(tr + 1.f) * 2.f; q[3] = 0.25f * s; q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s; }
    else if (R[0] > R[4] && R[0] > R[8]) { const float s = std::sqrt(1.f + R[0] - R[4] - R[8]) * 2.f; q[3] = (R[7] - R[5]) / s; q[0] = 0.25f * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s; }
    else if (R[4] > R[8]) { const float s = std::sqrt(1.f + R[4] - R[0] - R[8]) * 2.f; q[3] = (R[2] - R[6]) / s; q[0] = (R[1] + R[3]) / s; q[1] = 0.25f * s; q[2] = (R[5] + R[7]) / s; }
    else { const float s = std::sqrt(1.f + R[8] - R[0] - R[4]) * 2.f; q[3] = (R[3] - R[1]) / s; q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25f * s; }
    for (int k = 0; k < 4; ++k) out[k] = q[k];
    for (int k = 0; k < 3; ++k) out[4 + k] = Rt12[9 + k];
  }
  // one frame through morb_pose_inertial_optimization_last_{keyframe,frame}[_fisheye]_batch
  static int pose_inertial(PoseInertialView& v, bool bRecInit, bool lastFrame, int device) {
    if (v.N <= 0) return 0;
    const int N = v.N;
    Slot& o = slot(device, kTracking);
    std::lock_guard<std::mutex> lock(o.mu);
    Call c(device, morb_optimizer_stream(o.h));
    const int* d_count = c.in(&N, 1);
    const int* d_nLeft = v.rig28 ? c.in(&v.nLeft, 1) : nullptr;
    const uint8_t* d_hasMP = c.in(v.hasMapPoint, N);
    const float *d_obs = c.in(v.obs, (size_t)N * 3), *d_invSigma2 = c.in(v.invSigma2, N), *d_Xw = c.in(v.worldPos, (size_t)N * 3);
    const uint8_t* d_close = c.in(v.close, N);
    const float* d_other = c.in(v.otherState, 21);   // the fixed keyframe's state / the free previous frame's
    const morb_imu_preintegrated* d_pre = c.in(&v.pre, 1);
    float* d_state = c.in(v.state, 21);
    uint8_t* d_outlier = (int)v.mvbOutlier.size() == N ? c.in(v.mvbOutlier.data(), N) : c.out_filled<uint8_t>(N, 0);
    int* d_nInliers = c.out<int>(1);
    double* d_prior = c.out<double>(246);
    if (!lastFrame) {
      if (v.rig28)
        check(morb_pose_inertial_optimization_last_keyframe_fisheye_batch(o.h, 1, N, d_count, d_nLeft, d_hasMP, d_obs, d_invSigma2, d_Xw, d_close, v.rig28,
                                                                          v.Tbc12, d_other, d_pre, bRecInit ? 1 : 0, d_state, d_outlier, d_nInliers,
                                                                          d_prior, nullptr));
      else
        check(morb_pose_inertial_optimization_last_keyframe_batch(o.h, 1, N, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, d_close, v.fx, v.fy, v.cx, v.cy,
                                                                  v.mbf, v.Tbc12, d_other, d_pre, bRecInit ? 1 : 0, d_state, d_outlier, d_nInliers,
                                                                  d_prior, nullptr));
    } else {
      const morb_imu_preintegrated* d_preKF = c.in(&v.preKF, 1);
      const double* d_prevPrior = c.in(v.prevPrior, 246);
      if (v.rig28)
        check(morb_pose_inertial_optimization_last_frame_fisheye_batch(o.h, 1, N, d_count, d_nLeft, d_hasMP, d_obs, d_invSigma2, d_Xw, d_close, v.rig28,
                                                                       v.Tbc12, d_other, d_pre, d_preKF, d_prevPrior, bRecInit ? 1 : 0, d_state,
                                                                       d_outlier, d_nInliers, d_prior, nullptr));
      else
        check(morb_pose_inertial_optimization_last_frame_batch(o.h, 1, N, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, d_close, v.fx, v.fy, v.cx, v.cy,
                                                               v.mbf, v.Tbc12, d_other, d_pre, d_preKF, d_prevPrior, bRecInit ? 1 : 0, d_state, d_outlier,
                                                               d_nInliers, d_prior, nullptr));
    }
    c.wait();
    c.fetch(d_state, v.state, 21); c.fetch(d_prior, v.prior, 246);
    v.mvbOutlier = c.fetch(d_outlier, N);
    return c.fetch(d_nInliers, 1)[0];
  }
  using Call = morb_adapter::CallStaging;   // one per staged call: device, the handle's stream, this thread's staging (device_buffer.h)
  struct Slot { std::once_flag once; std::mutex mu; morb_optimizer* h = nullptr; };
  static Slot& slot(int device, Role role) {
    if (device < 0 || device >= morb_adapter::kMaxDevices) throw std::runtime_error("bad device");
    static Slot slots[morb_adapter::kMaxDevices][3];
    Slot& o = slots[device][role];
    std::call_once(o.once, [&] {
      if (morb_optimizer_create(&o.h, device) != MORB_OK) { o.h = nullptr; throw std::runtime_error(std::string("morb_optimizer_create: ") + morb_last_error()); }
      morb_optimizer_set_exact_order(o.h, 1);   // the drop-in follows g2o's LM path decision for decision (edge-order sums); a frame at a time the cost is latency, not throughput
    });
    if (!o.h) throw std::runtime_error("morb_optimizer_create failed earlier");
    return o;
  }
  static void check(int rc) { if (rc < 0) throw std::runtime_error(morb_last_error()); }
};

}  // namespace ORB_SLAM3

#include "Optimizer_reference.h"
