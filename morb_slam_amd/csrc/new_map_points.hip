// LocalMapping::CreateNewMapPoints between SearchForTriangulation and Fuse (reference src/LocalMapping.cc:489-709): per match the
// parallax test, Triangulate or UnprojectStereo, the depth, reprojection and scale tests, and the fields a new MapPoint gets from
// ComputeDistinctiveDescriptors and UpdateNormalAndDepth.  The arithmetic is include/morb/new_map_points_math.h (over
// morb/camera_math.h), which the CPU oracle compiles too; this file is the mapping onto the device.
//
// k_new_map_points: one workgroup of 256 threads per keyframe pair.
//   phase 1  the non-negative entries of the pair's match12 row are compacted into LDS in ascending i (ballot + prefix per wave, wave
//            totals through LDS): matches are sparse in cap, and a thread per feature would leave most lanes idle through the FP64
//            Jacobi of Triangulate.  The same pass clears the pair's status row.
//   phase 2  thread t takes matches t, t + 256, ...: nmp_decide, then for a created point its row of the caller's tables and the two
//            byte stores of 1 into d_hasMP (AddMapPoint, :700-701).
//   counters per-thread integers, summed by a DPP wave reduction and then over the four waves: no atomics, a rerun is bit-identical.
// 256 threads: a neighbour pair has a few hundred matches at most, so one pass of phase 2 covers it; the kernel's registers (the
// Jacobi's 32 doubles, the poses, the KB8 polynomial: 185 VGPRs) allow two waves per SIMD whatever the block size, i.e. two such
// workgroups per CU.  LDS is 4 * cap bytes of list.  DESIGN.md section 6 has the code object's figures and the timings.
#include <vector>

#include "common.h"
#include "handles.h"
#include "morb/new_map_points_math.h"
#include "wave.h"

namespace {

using namespace morb;
using namespace morbnmp;

constexpr int NMP_THREADS = 256;
constexpr int NMP_MAX_CAP = 32768;   // the LDS list: 4 * cap bytes of the CU's 160 KiB

struct NmpArgs {
  morb_frame_params P;
  Camera camL, camR;
  int rig, cap, nimg, nrows;
  const int* d_count;
  const morb_keypoint* d_kps;
  const morb_keypoint* d_kpsRaw;
  const uint8_t* d_desc;
  const float* d_uRight;
  const float* d_depth;
  const int *d_img1, *d_img2, *d_nLeft1, *d_nLeft2, *d_match12;
  const float* d_poses;            // [npairs][4 | 8][12]
  const uint8_t* d_kf2First;       // [npairs]
  float ratioFactor, thFarPoints;
  int inertial, farPoints;
  int* d_status;
  int* d_stats;
  const int* d_row;
  float *d_Xw, *d_normal, *d_maxDist, *d_minDist;
  uint8_t* d_mpDesc;
  int *d_obsImg2, *d_obsIdx2;
  uint8_t* d_hasMP;
};

__global__ __launch_bounds__(NMP_THREADS) void k_new_map_points(const NmpArgs a) {
  extern __shared__ __align__(16) int s_list[];
  __shared__ int s_wcnt[NMP_THREADS / 64];
  __shared__ int s_red[NMP_THREADS / 64][NMP_STATS_LEN];
  __shared__ float s_pose[NMP_PAIR_POSES_RIG * NMP_POSE];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cap = a.cap;
  const int img1 = a.d_img1[p], img2 = a.d_img2[p], row = a.d_row[p];
  int* status = a.d_status + (size_t)p * cap;
  // a pair that names an image or a row outside the tables touches nothing but its own status and stats
  const bool bad = img1 < 0 || img1 >= a.nimg || img2 < 0 || img2 >= a.nimg || row < 0 || row >= a.nrows;
  if (bad) {
    for (int i = tid; i < cap; i += NMP_THREADS) status[i] = NMP_NONE;
    if (tid < NMP_STATS_LEN) a.d_stats[p * NMP_STATS_LEN + tid] = -1;
    return;
  }
  const int n1 = min(max(a.d_count[img1], 0), cap), n2 = min(max(a.d_count[img2], 0), cap);
  const int nposes = a.rig ? NMP_PAIR_POSES_RIG : NMP_PAIR_POSES;
  if (tid < nposes * NMP_POSE) s_pose[tid] = a.d_poses[(size_t)p * nposes * NMP_POSE + tid];
  const int* m12 = a.d_match12 + (size_t)p * cap;

  // phase 1
  int nmatch = 0;
  for (int start = 0; start < cap; start += NMP_THREADS) {
    const int i = start + tid;
    const int m = i < n1 ? m12[i] : -1;
    const bool valid = m >= 0 && m < n2;
    if (i < cap) status[i] = NMP_NONE;
    const unsigned long long b = __ballot(valid);
    if (lane == 0) s_wcnt[wave] = __popcll(b);
    __syncthreads();
    int wbase = nmatch, total = 0;
#pragma unroll
    for (int w = 0; w < NMP_THREADS / 64; ++w) {
      const int c = s_wcnt[w];
      if (w < wave) wbase += c;
      total += c;
    }
    if (valid) s_list[wbase + __popcll(b & ((1ull << lane) - 1ull))] = i;
    nmatch += total;
    __syncthreads();
  }

  // phase 2
  Params P;
  P.fx = a.P.fx; P.fy = a.P.fy; P.cx = a.P.cx; P.cy = a.P.cy;
  P.invfx = 1.0f / a.P.fx; P.invfy = 1.0f / a.P.fy;
  P.mb = a.P.mb; P.mbf = a.P.mbf;
  P.ratioFactor = a.ratioFactor; P.thFarPoints = a.thFarPoints;
  P.inertial = a.inertial; P.farPoints = a.farPoints;
  P.scaleFactors = a.P.scaleFactors; P.levelSigma2 = a.P.levelSigma2;
  const int nl = a.P.nlevels;
  const int nLeft1 = a.rig ? a.d_nLeft1[p] : 0, nLeft2 = a.rig ? a.d_nLeft2[p] : 0;
  const bool fromKf2 = nmp_descriptor_from_kf2(a.d_kf2First[p]);
  int nCreated = 0, nTotalStereo = 0, nAttempt = 0, nGoodProj = 0, nStereo = 0;
  const size_t f1 = (size_t)img1 * cap, f2 = (size_t)img2 * cap;
  for (int k = tid; k < nmatch; k += NMP_THREADS) {
    const int i1 = s_list[k], i2 = m12[i1];
    const morb_keypoint kp1 = a.d_kps[f1 + i1], kp2 = a.d_kps[f2 + i2];
    Side s1, s2;
    const int right1 = a.rig && i1 >= nLeft1, right2 = a.rig && i2 >= nLeft2;
    // (pose, inverse) blocks: pinhole 0, 1 | 2, 3; rig left 0, 1, right 2, 3 | left 4, 5, right 6, 7
    const float* T1 = s_pose + (right1 ? 2 : 0) * NMP_POSE;
    const float* T2 = s_pose + ((a.rig ? 4 : 2) + (right2 ? 2 : 0)) * NMP_POSE;
    const float Ow1[3] = {T1[NMP_POSE + 3], T1[NMP_POSE + 7], T1[NMP_POSE + 11]};
    const float Ow2[3] = {T2[NMP_POSE + 3], T2[NMP_POSE + 7], T2[NMP_POSE + 11]};
    s1.Tcw = T1; s1.Twc = T1 + NMP_POSE;
    s2.Tcw = T2; s2.Twc = T2 + NMP_POSE;
    for (int c = 0; c < 3; ++c) { s1.Ow[c] = Ow1[c]; s2.Ow[c] = Ow2[c]; }
    s1.cam = right1 ? a.camR : a.camL;
    s2.cam = right2 ? a.camR : a.camL;
    s1.x = kp1.x; s1.y = kp1.y; s1.octave = min(max(kp1.octave, 0), nl - 1);
    s2.x = kp2.x; s2.y = kp2.y; s2.octave = min(max(kp2.octave, 0), nl - 1);
    s1.rawx = kp1.x; s1.rawy = kp1.y; s2.rawx = kp2.x; s2.rawy = kp2.y;
    s1.ur = -1.f; s2.ur = -1.f; s1.depth = -1.f; s2.depth = -1.f;
    if (!a.rig && a.d_uRight) {
      s1.ur = a.d_uRight[f1 + i1]; s1.depth = a.d_depth[f1 + i1];
      s2.ur = a.d_uRight[f2 + i2]; s2.depth = a.d_depth[f2 + i2];
      if (a.d_kpsRaw) {
        s1.rawx = a.d_kpsRaw[f1 + i1].x; s1.rawy = a.d_kpsRaw[f1 + i1].y;
        s2.rawx = a.d_kpsRaw[f2 + i2].x; s2.rawy = a.d_kpsRaw[f2 + i2].y;
      }
    }
    s1.bStereo = s1.ur >= 0; s2.bStereo = s2.ur >= 0;
    float x3D[3];
    int flags = 0;
    const int st = nmp_decide(P, s1, s2, x3D, &flags);
    status[i1] = st;
    nTotalStereo += flags & 1;
    nAttempt += (flags >> 1) & 1;
    nGoodProj += (flags >> 2) & 1;
    if (!nmp_created(st)) continue;
    nCreated += 1;
    nStereo += st != NMP_TRIANGULATED;
    float normal[3], maxD, minD;
    // the reference distance is to the current keyframe's LEFT centre (pRefKF->GetCameraCenter())
    const float OwRef[3] = {s_pose[NMP_POSE + 3], s_pose[NMP_POSE + 7], s_pose[NMP_POSE + 11]};
    nmp_point_fields(x3D, Ow1, Ow2, OwRef, a.P.scaleFactors[s1.octave], a.P.scaleFactors[nl - 1], normal, &maxD, &minD);
    const size_t o = (size_t)row * cap + i1;
    a.d_Xw[o * 3] = x3D[0]; a.d_Xw[o * 3 + 1] = x3D[1]; a.d_Xw[o * 3 + 2] = x3D[2];
    a.d_normal[o * 3] = normal[0]; a.d_normal[o * 3 + 1] = normal[1]; a.d_normal[o * 3 + 2] = normal[2];
    a.d_maxDist[o] = maxD;
    a.d_minDist[o] = minD;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.d_desc + (fromKf2 ? f2 + i2 : f1 + i1) * 32);
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.d_mpDesc + o * 32);
#pragma unroll
    for (int w = 0; w < 8; ++w) dst[w] = src[w];
    a.d_obsImg2[o] = img2;
    a.d_obsIdx2[o] = i2;
    a.d_hasMP[f1 + i1] = 1;
    a.d_hasMP[f2 + i2] = 1;
  }
  {
    const int c0 = morbwave::sum_i32(nCreated), c1 = morbwave::sum_i32(nTotalStereo), c2 = morbwave::sum_i32(nAttempt),
              c3 = morbwave::sum_i32(nGoodProj), c4 = morbwave::sum_i32(nStereo);
    if (lane == 0) {
      s_red[wave][NMP_S_CREATED] = c0; s_red[wave][NMP_S_TOTAL_STEREO_PTS] = c1; s_red[wave][NMP_S_STEREO_ATTEMPT] = c2;
      s_red[wave][NMP_S_STEREO_GOOD_PROJ] = c3; s_red[wave][NMP_S_COUNT_STEREO] = c4;
    }
  }
  __syncthreads();
  if (tid < NMP_STATS_LEN) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < NMP_THREADS / 64; ++w) s += s_red[w][tid];
    a.d_stats[p * NMP_STATS_LEN + tid] = s;
  }
}

int create_new_map_points_impl(morb_matcher* m, const morb_frame_params* P, int npairs, const int* d_img1, const int* d_img2,
                               const int* d_nLeft1, const int* d_nLeft2, int nimg, int cap, const int* d_count, const morb_keypoint* d_kps,
                               const morb_keypoint* d_kpsRaw, const uint8_t* d_desc, const float* d_uRight, const float* d_depth,
                               const float* camL8, const float* camR8, const int* d_match12, const float* poses, const uint8_t* kf2First,
                               float ratioFactor, int mbInertial, int mbFarPoints, float mThFarPoints, int* d_status, int* d_stats,
                               int nrows, const int* d_row, float* d_Xw, float* d_normal, float* d_maxDist, float* d_minDist,
                               uint8_t* d_mpDesc, int* d_obsImg2, int* d_obsIdx2, uint8_t* d_hasMP, void* stream) {
  MORB_REQUIRE(m && P && d_img1 && d_img2 && d_count && d_kps && d_desc && d_match12 && poses && kf2First && d_status && d_stats && d_row &&
                   d_Xw && d_normal && d_maxDist && d_minDist && d_mpDesc && d_obsImg2 && d_obsIdx2 && d_hasMP, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(npairs > 0 && nimg > 0 && nrows > 0 && cap > 0, MORB_ERR_INVALID, "bad sizes");
  MORB_REQUIRE(cap <= NMP_MAX_CAP, MORB_ERR_UNSUPPORTED, "cap beyond the match list the LDS holds (32768)");
  MORB_REQUIRE(P->nlevels >= 1 && P->nlevels <= 16, MORB_ERR_INVALID, "bad nlevels");
  MORB_REQUIRE((d_uRight == nullptr) == (d_depth == nullptr), MORB_ERR_INVALID, "mvuRight and mvDepth come together");
  MORB_REQUIRE(!(mbFarPoints && !(mThFarPoints > 0)), MORB_ERR_INVALID, "mbFarPoints needs a positive mThFarPoints");
  const bool rig = d_nLeft1 != nullptr;
  MORB_ENTER(st, m, stream);
  const int nposes = rig ? NMP_PAIR_POSES_RIG : NMP_PAIR_POSES;
  const size_t nf = (size_t)npairs * nposes * NMP_POSE;
  // one block: the poses, then a flag byte per pair
  float* dT = nullptr;
  int rc = grow(m->newPointPairs, nf + (size_t)div_up(npairs, 4), &dT);
  if (rc != MORB_OK) return rc;
  uint8_t* dFlag = reinterpret_cast<uint8_t*>(dT + nf);
  MORB_HIP_CHECK(hipMemcpyAsync(dT, poses, sizeof(float) * nf, hipMemcpyHostToDevice, st));
  MORB_HIP_CHECK(hipMemcpyAsync(dFlag, kf2First, (size_t)npairs, hipMemcpyHostToDevice, st));
  MORB_HIP_CHECK(hipStreamSynchronize(st));  // both are the caller's memory
  NmpArgs a;
  a.P = *P;
  a.camL.kb8 = a.camR.kb8 = rig ? 1 : 0;
  const float K[8] = {P->fx, P->fy, P->cx, P->cy, 0, 0, 0, 0};
  for (int i = 0; i < 8; ++i) { a.camL.p[i] = rig ? camL8[i] : K[i]; a.camR.p[i] = rig ? camR8[i] : K[i]; }
  a.rig = rig; a.cap = cap; a.nimg = nimg; a.nrows = nrows;
  a.d_count = d_count; a.d_kps = d_kps; a.d_kpsRaw = d_kpsRaw; a.d_desc = d_desc; a.d_uRight = d_uRight; a.d_depth = d_depth;
  a.d_img1 = d_img1; a.d_img2 = d_img2; a.d_nLeft1 = d_nLeft1; a.d_nLeft2 = d_nLeft2; a.d_match12 = d_match12;
  a.d_poses = dT; a.d_kf2First = dFlag;
  a.ratioFactor = ratioFactor; a.thFarPoints = mThFarPoints; a.inertial = mbInertial ? 1 : 0; a.farPoints = mbFarPoints ? 1 : 0;
  a.d_status = d_status; a.d_stats = d_stats; a.d_row = d_row;
  a.d_Xw = d_Xw; a.d_normal = d_normal; a.d_maxDist = d_maxDist; a.d_minDist = d_minDist; a.d_mpDesc = d_mpDesc;
  a.d_obsImg2 = d_obsImg2; a.d_obsIdx2 = d_obsIdx2; a.d_hasMP = d_hasMP;
  hipLaunchKernelGGL(k_new_map_points, dim3(npairs), dim3(NMP_THREADS), sizeof(int) * (size_t)cap, st, a);
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}

}  // namespace

extern "C" int morb_create_new_map_points_batch(morb_matcher* m, const morb_frame_params* P, int npairs, const int* d_img1, const int* d_img2,
                                                int nimg, int cap, const int* d_count, const morb_keypoint* d_kps,
                                                const morb_keypoint* d_kpsRaw, const uint8_t* d_desc, const float* d_uRight,
                                                const float* d_depth, const int* d_match12, const float* poses, const uint8_t* kf2First,
                                                float ratioFactor, int mbInertial, int mbFarPoints, float mThFarPoints, int* d_status,
                                                int* d_stats, int nrows, const int* d_row, float* d_Xw, float* d_normal, float* d_maxDist,
                                                float* d_minDist, uint8_t* d_mpDesc, int* d_obsImg2, int* d_obsIdx2, uint8_t* d_hasMP,
                                                void* stream) {
  return create_new_map_points_impl(m, P, npairs, d_img1, d_img2, nullptr, nullptr, nimg, cap, d_count, d_kps, d_kpsRaw, d_desc, d_uRight, d_depth,
                                    nullptr, nullptr, d_match12, poses, kf2First, ratioFactor, mbInertial, mbFarPoints, mThFarPoints, d_status,
                                    d_stats, nrows, d_row, d_Xw, d_normal, d_maxDist, d_minDist, d_mpDesc, d_obsImg2, d_obsIdx2, d_hasMP, stream);
}

extern "C" int morb_create_new_map_points_fisheye_batch(morb_matcher* m, const morb_frame_params* P, int npairs, const int* d_img1,
                                                        const int* d_img2, const int* d_nLeft1, const int* d_nLeft2, int nimg, int cap,
                                                        const int* d_count, const morb_keypoint* d_kps, const uint8_t* d_desc,
                                                        const float* camL8, const float* camR8, const int* d_match12, const float* poses,
                                                        const uint8_t* kf2First, float ratioFactor, int mbInertial, int mbFarPoints,
                                                        float mThFarPoints, int* d_status, int* d_stats, int nrows, const int* d_row,
                                                        float* d_Xw, float* d_normal, float* d_maxDist, float* d_minDist, uint8_t* d_mpDesc,
                                                        int* d_obsImg2, int* d_obsIdx2, uint8_t* d_hasMP, void* stream) {
  MORB_REQUIRE(d_nLeft1 && d_nLeft2 && camL8 && camR8, MORB_ERR_INVALID, "rig form: NLeft of both keyframes and both cameras");
  return create_new_map_points_impl(m, P, npairs, d_img1, d_img2, d_nLeft1, d_nLeft2, nimg, cap, d_count, d_kps, nullptr, d_desc, nullptr, nullptr,
                                    camL8, camR8, d_match12, poses, kf2First, ratioFactor, mbInertial, mbFarPoints, mThFarPoints, d_status,
                                    d_stats, nrows, d_row, d_Xw, d_normal, d_maxDist, d_minDist, d_mpDesc, d_obsImg2, d_obsIdx2, d_hasMP, stream);
}
