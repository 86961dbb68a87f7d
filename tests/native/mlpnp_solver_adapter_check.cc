// Drives ORB_SLAM3::MLPnPsolver in the reference's signature (include/morb/MLPnPsolver.h) on the GPU with the mock Frame / MapPoint of
// tests/native/mock_ref and the Matrix4f of tests/native/mock_mlpnp_solver, after srand(seed), two ways: a relocalisation loop over all
// candidates (iterate(5, ..) round-robin, a candidate discarded on bNoMore, every candidate kept being called until it is discarded or
// `rounds` rounds are done) and, after another srand(seed), one direct iterate(5, ..) on the first candidate alone.
// tests/test_mlpnp_solver_adapter_gpu.py writes the candidates and compares what this program writes with the CPU oracle fed the same
// rand() stream.
//   in:  int32 K, seed, rounds, kind; float cam[8], levelSigma2[8]; int32 nKeys (mvKeysUn.size()); per key: float x, y; int32 octave;
//        per candidate: int32 n, minInliers, maxIterations, minSet; double probability; float epsilon, th2;
//                       per feature: uint8 bits (1 matched, 2 bad), float Xw[3]
//   out: per call in call order: int32 candidate, ok, bNoMore, nInliers, vbInliers.size(); uint8 vbInliers[n]; float Tout[16];
//        then int32 -1, the next rand() value, 0, 0, 0; then the direct call in the per-call layout (candidate = 0).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "Frame.h"   // tests/native/mock_ref
#include "MapPoint.h"
#include "relocalization_mock.h"   // tests/native/mock_mlpnp_solver
#include "MLPnPsolver.h"           // include/morb

namespace ORB_SLAM3 { std::mutex MapPoint::mGlobalMutex; }
using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n = 1) { return fread(p, sizeof(T), n, f) == n; }

struct Cand {
  int n, minIn, maxIts, minSet;
  double prob;
  float eps, th2;
  std::vector<MapPoint*> matches;
};

static void record(FILE* w, int cand, bool ok, bool noMore, int nIn, const std::vector<bool>& vb, int n, const Eigen::Matrix4f& T) {
  const int hdr[5] = {cand, ok, noMore, nIn, (int)vb.size()};
  fwrite(hdr, 4, 5, w);
  std::vector<uint8_t> m(n > 0 ? n : 1, 0);
  for (int i = 0; i < n && i < (int)vb.size(); ++i) m[i] = vb[i];
  fwrite(m.data(), 1, n, w);
  float t[16];
  for (int i = 0; i < 16; ++i) t[i] = T(i / 4, i % 4);
  fwrite(t, 4, 16, w);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int K, seed, rounds, kind, nKeys;
  float cam[8], lev[8];
  if (!(rd(f, &K) && rd(f, &seed) && rd(f, &rounds) && rd(f, &kind) && rd(f, cam, 8) && rd(f, lev, 8) && rd(f, &nKeys))) return 3;
  GeometricCamera c;
  c.mvParameters.assign(cam, cam + (kind ? 8 : 4));
  Frame F;
  F.mpCamera = &c;
  F.mvLevelSigma2.assign(lev, lev + 8);
  F.mvKeysUn.resize(nKeys);
  F.N = nKeys;
  for (int i = 0; i < nKeys; ++i)
    if (!(rd(f, &F.mvKeysUn[i].pt.x) && rd(f, &F.mvKeysUn[i].pt.y) && rd(f, &F.mvKeysUn[i].octave))) return 3;
  std::vector<std::unique_ptr<MapPoint>> pts;
  std::vector<Cand> cands(K);
  for (Cand& cd : cands) {
    if (!(rd(f, &cd.n) && rd(f, &cd.minIn) && rd(f, &cd.maxIts) && rd(f, &cd.minSet) && rd(f, &cd.prob) && rd(f, &cd.eps) && rd(f, &cd.th2))) return 3;
    cd.matches.assign(cd.n, nullptr);
    for (int i = 0; i < cd.n; ++i) {
      uint8_t e;
      float X[3];
      if (!(rd(f, &e) && rd(f, X, 3))) return 3;
      if (!(e & 1)) continue;
      pts.emplace_back(new MapPoint);
      pts.back()->mWorldPos = Eigen::Vector3f(X[0], X[1], X[2]);
      pts.back()->mbBad = (e & 2) != 0;
      cd.matches[i] = pts.back().get();
    }
  }
  fclose(f);
  FILE* w = fopen(argv[2], "wb");
  if (!w) return 4;
  int calls = 0, found = 0;
  {   // a throw-away call first: whatever the HIP runtime does when it starts happens before srand(seed)
    MLPnPsolver warm(F, cands[0].matches);
    std::vector<bool> vb;
    int nIn = 0;
    bool bNoMore = false;
    Eigen::Matrix4f T;
    warm.iterate(1, bNoMore, vb, nIn, T);
  }
  {   // the relocalisation loop
    srand(seed);
    std::vector<std::unique_ptr<MLPnPsolver>> solvers;
    std::vector<bool> discarded(K, false);
    for (Cand& cd : cands) {
      solvers.emplace_back(new MLPnPsolver(F, cd.matches));
      solvers.back()->SetRansacParameters(cd.prob, cd.minIn, cd.maxIts, cd.minSet, cd.eps, cd.th2);
    }
    for (int round = 0; round < rounds; ++round)
      for (int i = 0; i < K; ++i) {
        if (discarded[i]) continue;
        std::vector<bool> vb;
        int nIn = -1;
        bool bNoMore = false;
        Eigen::Matrix4f T;
        const bool ok = solvers[i]->iterate(5, bNoMore, vb, nIn, T);
        if (bNoMore) discarded[i] = true;
        record(w, i, ok, bNoMore, nIn, vb, cands[i].n, T);
        ++calls;
        found += ok;
      }
    const int marker[5] = {-1, rand(), 0, 0, 0};   // the next rand() value: where the loop left the stream
    fwrite(marker, 4, 5, w);
  }
  {   // a direct call
    srand(seed);
    MLPnPsolver S(F, cands[0].matches);
    S.SetRansacParameters(cands[0].prob, cands[0].minIn, cands[0].maxIts, cands[0].minSet, cands[0].eps, cands[0].th2);
    std::vector<bool> vb;
    int nIn = -1;
    bool bNoMore = false;
    Eigen::Matrix4f T;
    const bool ok = S.iterate(5, bNoMore, vb, nIn, T);
    record(w, 0, ok, bNoMore, nIn, vb, cands[0].n, T);
  }
  fclose(w);
  printf("calls %d with a pose %d\n", calls, found);
  return 0;
}
