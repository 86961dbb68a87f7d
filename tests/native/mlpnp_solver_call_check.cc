// MLPnPsolver in a relocalisation caller's form, written for this test against the mocks of tests/native/mock_ref and
// tests/native/mock_mlpnp_solver: one solver per candidate constructed from (Frame&, vector<MapPoint*>&), the six-argument
// SetRansacParameters, iterate(5, ..) into an Eigen::Matrix4f, round-robin until every candidate is discarded or one gives a pose.
// It compiles <=> the adapter class accepts such a caller; the enclosing function is marked `used`, so every member is instantiated
// (tests/test_mlpnp_solver_cpu.py).
#include <vector>

#include "Frame.h"   // tests/native/mock_ref
#include "MapPoint.h"
#include "relocalization_mock.h"   // tests/native/mock_mlpnp_solver
#include "MLPnPsolver.h"           // include/morb

namespace ORB_SLAM3 {
std::mutex MapPoint::mGlobalMutex;

struct RelocalizationCheck {
  Frame mCurrentFrame;

  __attribute__((used)) int Relocalize(std::vector<std::vector<MapPoint*>>& vvpMapPointMatches) {
    const int nKFs = (int)vvpMapPointMatches.size();
    std::vector<MLPnPsolver*> solvers(nKFs, nullptr);
    std::vector<bool> discarded(nKFs, false);
    int nCandidates = 0;
    for (int i = 0; i < nKFs; ++i) {
      if (vvpMapPointMatches[i].size() < 15) { discarded[i] = true; continue; }
      solvers[i] = new MLPnPsolver(mCurrentFrame, vvpMapPointMatches[i]);
      solvers[i]->SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991);
      ++nCandidates;
    }
    int found = -1, total = 0;
    while (nCandidates > 0 && found < 0) {
      for (int i = 0; i < nKFs && found < 0; ++i) {
        if (discarded[i]) continue;
        std::vector<bool> vbInliers;
        int nInliers = 0;
        bool bNoMore = false;
        Eigen::Matrix4f eigTcw;
        const bool bTcw = solvers[i]->iterate(5, bNoMore, vbInliers, nInliers, eigTcw);
        if (bNoMore) { discarded[i] = true; --nCandidates; }
        if (bTcw) { found = i; total = nInliers + (int)eigTcw(0, 0) + (int)vbInliers.size(); }
      }
    }
    MLPnPsolver defaults(mCurrentFrame, vvpMapPointMatches[0]);   // the constructor's own SetRansacParameters()
    defaults.SetRansacParameters();
    for (MLPnPsolver* s : solvers) delete s;
    return total + defaults.state().N;
  }
};
}  // namespace ORB_SLAM3
