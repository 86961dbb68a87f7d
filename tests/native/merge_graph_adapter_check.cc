// Optimizer::OptimizeEssentialGraph(MergeEssentialGraphView&) of include/morb/Optimizer.h driven from C++ on the library
// (tests/test_merge_graph_adapter_gpu.py): `merge_graph_adapter_check <problem.bin> <result.bin>`.  The problem file is
// tests/merge_graph_cases.py::problem_bytes: nKF, nC, nMP (int32), kfLists, the four pose arrays, cI, cJ, mpPos, mpRef.  The result file
// holds the four pose arrays, mpPos, cKept, stats and chi2 as the view holds them behind the call.
#include <cstdio>
#include <fstream>
#include <vector>

#include "Optimizer.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(std::ifstream& f, std::vector<T>& v, size_t n) { v.resize(n); f.read(reinterpret_cast<char*>(v.data()), n * sizeof(T)); return (bool)f || n == 0; }
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s problem.bin result.bin\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  std::vector<int> hd, cI, cJ, mpRef;
  std::vector<uint8_t> lists;
  std::vector<float> pose[4], mpPos;
  if (!rd(in, hd, 3)) return 3;
  const size_t nKF = hd[0], nC = hd[1], nMP = hd[2];
  bool ok = rd(in, lists, nKF);
  for (auto& p : pose) ok = ok && rd(in, p, nKF * 7);
  ok = ok && rd(in, cI, nC) && rd(in, cJ, nC) && rd(in, mpPos, nMP * 3) && rd(in, mpRef, nMP);
  if (!ok) return 3;
  std::vector<uint8_t> kept(nC, 0);
  MergeEssentialGraphView g;
  g.nKF = (int)nKF; g.nC = (int)nC; g.nMP = (int)nMP;
  g.kfLists = lists.data(); g.kfTcw = pose[0].data(); g.kfTwc = pose[1].data(); g.kfTcwBefMerge = pose[2].data(); g.kfTwcBefMerge = pose[3].data();
  g.cI = nC ? cI.data() : nullptr; g.cJ = nC ? cJ.data() : nullptr; g.cKept = nC ? kept.data() : nullptr;
  g.mpPos = nMP ? mpPos.data() : nullptr; g.mpRef = nMP ? mpRef.data() : nullptr;
  Optimizer::OptimizeEssentialGraph(g);
  std::ofstream out(argv[2], std::ios::binary);
  for (auto& p : pose) wr(out, p.data(), p.size());
  wr(out, mpPos.data(), mpPos.size()); wr(out, kept.data(), kept.size()); wr(out, g.stats, 4); wr(out, g.chi2, 2);
  return out ? 0 : 1;
}
