// KeyFrameDatabase in the reference's call forms, against the mocks of tests/native/mock_ref (mock_types.h) and
// tests/native/mock_keyframe_database: the calls of LoopClosing.cc:484 and Tracking.cc:3369 as the reference writes them, in members
// marked `used` so that every template is instantiated, and, in main, the host side of the class with NO GPU call: add / erase / clear
// / clearMap and the flattening of a query (tests/test_keyframe_database_cpu.py).
#include <cstdio>
#include <vector>

#include "keyframe_database_mock.h"   // tests/native/mock_keyframe_database
#include "KeyFrameDatabase.h"         // include/morb

namespace ORB_SLAM3 {

struct LoopClosingCheck {
  KeyFrameDatabase* mpKeyFrameDB = nullptr;
  KeyFrame* mpCurrentKF = nullptr;
  __attribute__((used)) int NewDetectCommonRegions() {
    std::vector<KeyFrame*> vpMergeBowCand, vpLoopBowCand;
    // ---- LoopClosing.cc:484-485 ----
    mpKeyFrameDB->DetectNBestCandidates(mpCurrentKF, vpLoopBowCand,
                                        vpMergeBowCand, 3);
    // ---- end ----
    mpKeyFrameDB->add(mpCurrentKF);           // LoopClosing.cc:338 and others
    mpKeyFrameDB->erase(mpCurrentKF);         // KeyFrame.cc:716 and others
    return (int)(vpLoopBowCand.size() + vpMergeBowCand.size());
  }
};

struct TrackingCheck {
  KeyFrameDatabase* mpKeyFrameDB = nullptr;
  AtlasMock* mpAtlas = nullptr;
  Frame mCurrentFrame;
  __attribute__((used)) bool Relocalization() {
    // ---- Tracking.cc:3368-3372 ----
    vector<KeyFrame*> vpCandidateKFs =
        mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame,
                                                     mpAtlas->GetCurrentMap());

    if (vpCandidateKFs.empty()) {
      return false;
    }
    // ---- end ----
    mpKeyFrameDB->clear();                                // Tracking.cc:3645
    mpKeyFrameDB->clearMap(mpAtlas->GetCurrentMap());     // Tracking.cc:3705
    return true;
  }
};

}  // namespace ORB_SLAM3

using namespace ORB_SLAM3;

#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  ORBVocabulary voc;
  KeyFrameDatabase db(voc);
  db.SetORBVocabulary(&voc);
  Map maps[2];
  maps[1].mbBad = true;
  std::vector<KeyFrame> kf(6);
  for (int k = 0; k < 6; ++k) {
    kf[k].mnId = k + 1;
    kf[k].mpMap = &maps[k >= 4];
    kf[k].mBowVec[k] = 0.5; kf[k].mBowVec[k + 1] = 0.25; kf[k].mBowVec[100] = 0.25;   // word 100 is everybody's
  }
  kf[5].mBowVec.clear(); kf[5].mBowVec[7] = 1.0;   // shares nothing with keyframe 0
  kf[2].mbBad = true;
  kf[2].mPlaceRecognitionScore = 0.375f;
  kf[1].mvpOrdered = {&kf[2], &kf[0], &kf[3]};   // kf[0] is never added: no row
  kf[0].mspConnected = {&kf[1], &kf[5], &kf[3]};
  for (int k : {3, 1, 2, 4, 5}) db.add(&kf[k]);   // rows 0..4 = keyframes 3 1 2 4 5, add ranks 0..4
  EXPECT(db.rows() == 5 && db.add_rank(0) == 0 && db.add_rank(4) == 4);
  db.erase(&kf[3]);
  EXPECT(db.add_rank(0) == -1);
  db.erase(&kf[0]);   // not in the database: nothing happens
  db.add(&kf[3]);     // back in, at the end of the add order, in its old row
  EXPECT(db.rows() == 5 && db.add_rank(0) == 5);
  KeyFrameDatabaseView v;
  std::vector<int> touched;
  db.flatten<KeyFrame>(kf[0].mBowVec, kf[0].GetMap(), false, v, &touched, &kf[0]);
  EXPECT(v.word == (std::vector<int>{0, 1, 100}) && v.value == (std::vector<double>{0.5, 0.25, 0.25}));
  EXPECT(v.ncovis == 10 && v.covis.size() == 50 && v.covis[10] == 2 && v.covis[11] == -1 && v.covis[12] == 0 && v.covis[13] == -1);
  EXPECT(v.mapId[0] == v.queryMap && v.mapId[3] != v.queryMap && v.mapId[4] == v.mapId[3]);
  EXPECT(v.flags == (std::vector<uint8_t>{0, 0, 1, 2, 2}) && v.prevScore[2] == 0.375f && v.prevScore[0] == 0.f);
  EXPECT(v.connected.size() == 3);   // rows 1, 0 and 4, in the set's order (by address)
  EXPECT(touched.size() == 2);   // keyframes 1 and 3 share word 100 (and 1) with the query; keyframe 5 shares none
  db.clearMap(&maps[1]);
  EXPECT(db.add_rank(3) == -1 && db.add_rank(4) == -1 && db.add_rank(1) == 1);
  kf[1].mpMap = &maps[1];     // a keyframe that changed map is cleared with its new map
  db.clearMap(&maps[1]);
  EXPECT(db.add_rank(1) == -1 && db.add_rank(2) == 2);
  db.clear();
  EXPECT(db.add_rank(2) == -1 && db.add_rank(0) == -1 && db.rows() == 5);
  const int w[2] = {3, 9};
  const double val[2] = {0.5, 0.5};
  EXPECT(db.add_row(w, val, 2) == 5 && db.add_rank(5) == 6);
  db.erase_row(5);
  EXPECT(db.add_rank(5) == -1);
  printf("flatten ok\n");
  return 0;
}
