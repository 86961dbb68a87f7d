// Drives ORB_SLAM3::KeyFrameDatabase in the reference's signatures (include/morb/KeyFrameDatabase.h) on the GPU with the mock KeyFrame /
// Frame / Map of tests/native/mock_keyframe_database: ONE database object, a script of add / erase / clearMap / DetectNBestCandidates /
// DetectRelocalizationCandidates in one process.  tests/test_keyframe_database_adapter_gpu.py writes the scene and the script and
// compares what this program prints with the CPU oracle driven through the same sequence.
//   in (text):  nmaps nrows; nmaps bad flags; per row: map bad nwords (word value)* ncovis row* nconnected row*; nops; per op one of
//               "A row", "E row", "M map", "N row nNumCandidates", "R row frameId map" (the frame's BoW vector is that row's)
//   out (text): per detection "N nLoop ids.. nMerge ids.." or "R n ids..", then one line per keyframe with the six fields the
//               reference writes: mnPlaceRecognitionQuery / Words / Score, mnRelocQuery / Words / Score (floats as %a).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "keyframe_database_mock.h"   // tests/native/mock_keyframe_database
#include "KeyFrameDatabase.h"         // include/morb

using namespace ORB_SLAM3;

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.txt out.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  FILE* w = fopen(argv[2], "w");
  if (!f || !w) return 2;
  int nmaps, n;
  if (fscanf(f, "%d %d", &nmaps, &n) != 2) return 3;
  std::vector<Map> maps(nmaps);
  for (Map& m : maps) { int b; if (fscanf(f, "%d", &b) != 1) return 3; m.mbBad = b != 0; }
  std::vector<KeyFrame> kfs(n);
  for (int k = 0; k < n; ++k) {
    int map, bad, nw, nc;
    if (fscanf(f, "%d %d %d", &map, &bad, &nw) != 3) return 3;
    kfs[k].mnId = k + 1; kfs[k].mpMap = &maps[map]; kfs[k].mbBad = bad != 0;
    for (int i = 0; i < nw; ++i) {
      int word; char val[64];
      if (fscanf(f, "%d %63s", &word, val) != 2) return 3;
      kfs[k].mBowVec[(DBoW2::WordId)word] = strtod(val, nullptr);
    }
    if (fscanf(f, "%d", &nc) != 1) return 3;
    for (int i = 0, r; i < nc; ++i) { if (fscanf(f, "%d", &r) != 1) return 3; kfs[k].mvpOrdered.push_back(&kfs[r]); }
    if (fscanf(f, "%d", &nc) != 1) return 3;
    for (int i = 0, r; i < nc; ++i) { if (fscanf(f, "%d", &r) != 1) return 3; kfs[k].mspConnected.insert(&kfs[r]); }
  }
  ORBVocabulary voc;
  KeyFrameDatabase db(voc);
  db.SetORBVocabulary(&voc);
  int nops, detections = 0;
  if (fscanf(f, "%d", &nops) != 1) return 3;
  for (int o = 0; o < nops; ++o) {
    char op[4];
    int a, b = 0, c = 0;
    if (fscanf(f, "%3s %d", op, &a) != 2) return 3;
    if (op[0] == 'A') db.add(&kfs[a]);
    else if (op[0] == 'E') db.erase(&kfs[a]);
    else if (op[0] == 'M') db.clearMap(&maps[a]);
    else if (op[0] == 'N') {
      if (fscanf(f, "%d", &b) != 1) return 3;
      std::vector<KeyFrame*> vpLoopBowCand, vpMergeBowCand;
      db.DetectNBestCandidates(&kfs[a], vpLoopBowCand, vpMergeBowCand, b);
      fprintf(w, "N %zu", vpLoopBowCand.size());
      for (KeyFrame* k : vpLoopBowCand) fprintf(w, " %d", (int)(k - kfs.data()));
      fprintf(w, " %zu", vpMergeBowCand.size());
      for (KeyFrame* k : vpMergeBowCand) fprintf(w, " %d", (int)(k - kfs.data()));
      fprintf(w, "\n");
    } else if (op[0] == 'R') {
      if (fscanf(f, "%d %d", &b, &c) != 2) return 3;
      Frame F;
      F.mnId = b; F.mBowVec = kfs[a].mBowVec;
      vector<KeyFrame*> vpCandidateKFs = db.DetectRelocalizationCandidates(&F, &maps[c]);
      fprintf(w, "R %zu", vpCandidateKFs.size());
      for (KeyFrame* k : vpCandidateKFs) fprintf(w, " %d", (int)(k - kfs.data()));
      fprintf(w, "\n");
    } else return 3;
    if (op[0] == 'N' || op[0] == 'R') {
      ++detections;
      for (const KeyFrame& k : kfs)
        fprintf(w, "%lu %d %a %lu %d %a\n", k.mnPlaceRecognitionQuery, k.mnPlaceRecognitionWords, (double)k.mPlaceRecognitionScore, k.mnRelocQuery,
                k.mnRelocWords, (double)k.mRelocScore);
    }
  }
  fclose(f);
  fclose(w);
  printf("ops %d detections %d\n", nops, detections);
  return 0;
}
