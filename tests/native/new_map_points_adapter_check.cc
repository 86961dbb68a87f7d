// Drives ORB_SLAM3::LocalMappingT::CreateNewMapPoints (include/morb/LocalMapping.h) on the GPU with the mock KeyFrame / MapPoint / Atlas
// of tests/native/mock_ref and tests/native/mock_local_mapping: one current keyframe and its neighbours, read from a file that
// tests/test_new_map_points_adapter_gpu.py writes from synth.make_local_mapping_scene; that test compares what this program writes with
// a host replay driven by the CPU oracles.
//   in:  int32 nkf (current first), cap, nlevels, mono, gated; float fx fy cx cy mb mbf, scaleFactors[nlevels], levelSigma2[nlevels];
//        per keyframe: int32 N; float Tcw R[9] t[3] Ow[3], ep[2]; float xy[N][2]; int32 octave[N]; int32 node[N]; uint8 desc[N][32]
//   out: int32 nkf - 1 flags kf2First (std::less of the mock pointers); int32 ncreated; per created point: int32 neighbour, idx1, idx2,
//        status; float Xw[3], normal[3], maxDistance, minDistance; uint8 descriptor[32]; then per keyframe int32 table[N]: the creation
//        index of the point at each feature or -1; then int32 nrecent and the creation indices of mlpRecentAddedMapPoints; then int32
//        atlas size, observations that disagree, points not updated exactly once.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "local_mapping_mock.h"   // tests/native/mock_local_mapping
#include "LocalMapping.h"         // include/morb

using namespace ORB_SLAM3;
typedef LocalMappingT<LMKeyFrame, LMMapPoint, LMAtlas, LMTracker, Eigen::Vector3f> LocalMapping;

template <class T> static bool rd(FILE* f, T* p, size_t n = 1) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  FILE* w = fopen(argv[2], "wb");
  if (!f || !w) return 2;
  int nkf, cap, nlevels, mono, gated;
  float cam[6];
  if (!(rd(f, &nkf) && rd(f, &cap) && rd(f, &nlevels) && rd(f, &mono) && rd(f, &gated) && rd(f, cam, 6))) return 3;
  std::vector<float> sf(nlevels), s2(nlevels);
  if (!(rd(f, sf.data(), nlevels) && rd(f, s2.data(), nlevels))) return 3;
  std::vector<LMKeyFrame> kfs(nkf);
  std::vector<GeometricCamera> cams(nkf);
  for (int k = 0; k < nkf; ++k) {
    LMKeyFrame& K = kfs[k];
    float pose[15], ep[2];
    if (!(rd(f, &K.N) && rd(f, pose, 15) && rd(f, ep, 2))) return 3;
    for (int i = 0; i < 9; ++i) K.mTcw.R[i] = pose[i];
    for (int i = 0; i < 3; ++i) { K.mTcw.t[i] = pose[9 + i]; K.mTcw.Ow[i] = pose[12 + i]; }
    std::vector<float> xy((size_t)K.N * 2);
    std::vector<int> oct(K.N), node(K.N);
    K.mDescriptors.data.resize((size_t)K.N * 32); K.mDescriptors.rows = K.N;
    if (!(rd(f, xy.data(), xy.size()) && rd(f, oct.data(), K.N) && rd(f, node.data(), K.N) && rd(f, K.mDescriptors.data.data(), (size_t)K.N * 32))) return 3;
    K.mvKeysUn.resize(K.N);
    for (int i = 0; i < K.N; ++i) { K.mvKeysUn[i].pt.x = xy[2 * i]; K.mvKeysUn[i].pt.y = xy[2 * i + 1]; K.mvKeysUn[i].octave = oct[i]; K.mvKeysUn[i].size = 31.f; K.mFeatVec[node[i]].push_back(i); }
    K.mvKeys = K.mvKeysUn;
    K.mvpMapPoints.assign(K.N, nullptr);
    K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mb = cam[4]; K.mbf = cam[5];
    K.mnMaxX = 752; K.mnMaxY = 480; K.mfGridElementWidthInv = 64.f / 752.f; K.mfGridElementHeightInv = 48.f / 480.f;
    K.mnScaleLevels = nlevels; K.mvScaleFactors = sf; K.mvLevelSigma2 = s2; K.mfScaleFactor = sf[1]; K.mfLogScaleFactor = std::log(sf[1]);
    cams[k].mvParameters = {cam[0], cam[1], cam[2], cam[3]};
    cams[k].ep.v[0] = ep[0]; cams[k].ep.v[1] = ep[1];
    K.mpCamera = &cams[k];
    K.mnId = k;
    K.medianDepth = 6.f;
  }
  for (int k = 1; k < nkf; ++k) kfs[0].mvpBest.push_back(&kfs[k]);
  // the gated neighbour, when asked for: moved onto the current keyframe's centre, so that its baseline is below mb
  if (gated > 0) for (int i = 0; i < 3; ++i) kfs[gated].mTcw.Ow[i] = kfs[0].mTcw.Ow[i] + 0.01f;

  LMAtlas atlas;
  LMTracker tracker;
  LocalMapping lm(0);
  lm.mpCurrentKeyFrame = &kfs[0]; lm.mpAtlas = &atlas; lm.mpTracker = &tracker; lm.mbMonocular = mono != 0;
  lm.CreateNewMapPoints();

  for (int k = 1; k < nkf; ++k) { const int first = std::less<KeyFrame*>()(&kfs[k], &kfs[0]) ? 1 : 0; fwrite(&first, 4, 1, w); }
  const int nc = (int)lm.created.size();
  fwrite(&nc, 4, 1, w);
  std::map<MapPoint*, int> order;
  int disagree = 0, notOnce = 0;
  for (int i = 0; i < nc; ++i) {
    const auto& c = lm.created[i];
    order[c.pMP] = i;
    const int hdr[4] = {(int)(static_cast<LMKeyFrame*>(c.pKF2) - &kfs[0]), c.idx1, c.idx2, c.status};
    fwrite(hdr, 4, 4, w);
    fwrite(c.Xw, 4, 3, w); fwrite(c.normal, 4, 3, w); fwrite(&c.maxDistance, 4, 1, w); fwrite(&c.minDistance, 4, 1, w);
    fwrite(c.descriptor, 1, 32, w);
    // the two observations the point carries, and its position
    if (std::get<0>(c.pMP->GetIndexInKeyFrame(&kfs[0])) != c.idx1 || std::get<0>(c.pMP->GetIndexInKeyFrame(c.pKF2)) != c.idx2 ||
        c.pMP->mObservations.size() != 2 || c.pMP->mWorldPos(0) != c.Xw[0] || c.pMP->mpRefKF != &kfs[0] || c.pMP->mpMap != &atlas.map)
      ++disagree;
    if (c.pMP->nDescriptorUpdates != 1 || c.pMP->nUpdates != 1) ++notOnce;
  }
  for (int k = 0; k < nkf; ++k) {
    std::vector<int> table(kfs[k].N, -1);
    for (int i = 0; i < kfs[k].N; ++i) if (kfs[k].mvpMapPoints[i]) table[i] = order.at(kfs[k].mvpMapPoints[i]);
    fwrite(table.data(), 4, table.size(), w);
  }
  const int nr = (int)lm.mlpRecentAddedMapPoints.size();
  fwrite(&nr, 4, 1, w);
  for (MapPoint* p : lm.mlpRecentAddedMapPoints) { const int o = order.at(p); fwrite(&o, 4, 1, w); }
  bool atlasOrder = (int)atlas.points.size() == nc;
  for (int i = 0; atlasOrder && i < nc; ++i) atlasOrder = order.at(atlas.points[i]) == i;
  const int tail[3] = {atlasOrder ? nc : -1, disagree, notOnce};
  fwrite(tail, 4, 3, w);
  fclose(f);
  fclose(w);
  printf("neighbours %d created %d\n", nkf - 1, nc);
  for (MapPoint* p : atlas.points) delete static_cast<LMMapPoint*>(p);
  return 0;
}
