// Optimizer::OptimizeEssentialGraph(EssentialGraphView&) of include/morb/Optimizer.h on one problem read from a file.
// Run as `essential_graph_adapter_check <in.bin> <out.bin>`; tests/test_essential_graph_adapter_gpu.py compares what it dumps with the C entry
// called from Python.  Built with -DEG_STUB_ENTRY (tests/test_essential_graph_cpu.py, under -fsanitize=address,undefined, no library and no
// GPU) the C entries the call reaches are stubs defined here: morb_optimize_essential_graph records its arguments into out.bin and returns
// canned results, which the program checks the view holds afterwards.
// in.bin: int nKF, nE, nMP; double kfSim3[nKF][8]; uint8 kfFlags[nKF]; int eI[nE], eJ[nE]; double eSji[nE][8]; float mpPos[nMP][3]; int mpRef[nMP].
// out.bin: kfSim3, mpPos, stats[4], chi2[2] after the call (stubbed: the recorded arguments in in.bin's layout come first).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "Optimizer.h"

using namespace ORB_SLAM3;

template <class T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), n * sizeof(T)); }
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

#ifdef EG_STUB_ENTRY
static std::ofstream* g_out = nullptr;
static int g_calls = 0;
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
int morb_optimizer_create(morb_optimizer** out, int) { static int token; *out = reinterpret_cast<morb_optimizer*>(&token); return MORB_OK; }
int morb_optimizer_set_exact_order(morb_optimizer*, int) { return MORB_OK; }
const char* morb_last_error(void) { return "stub"; }
int morb_optimize_essential_graph(morb_optimizer* o, int nKF, double* kfSim3, const uint8_t* kfFlags, int nE, const int* eI, const int* eJ,
                                  const double* eSji, int nMP, float* mpPos, const int* mpRef, int* stats4, double* chi2) {
  ++g_calls;
  if (!o) return MORB_ERR_INVALID;
  const int hd[3] = {nKF, nE, nMP};
  wr(*g_out, hd, 3); wr(*g_out, kfSim3, (size_t)nKF * 8); wr(*g_out, kfFlags, nKF); wr(*g_out, eI, nE); wr(*g_out, eJ, nE); wr(*g_out, eSji, (size_t)nE * 8);
  wr(*g_out, mpPos, (size_t)nMP * 3); wr(*g_out, mpRef, nMP);
  for (int i = 0; i < nKF * 8; ++i) kfSim3[i] = 100.0 + i;
  for (int i = 0; i < nMP * 3; ++i) mpPos[i] = 200.f + i;
  const int s[4] = {3, 12, nKF - 1, 77};
  std::memcpy(stats4, s, sizeof s);
  chi2[0] = 5.5; chi2[1] = 0.25;
  return MORB_OK;
}
}
#endif

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s in.bin out.bin\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  int hd[3];
  rd(in, hd, 3);
  const int nKF = hd[0], nE = hd[1], nMP = hd[2];
  std::vector<double> S((size_t)nKF * 8), M((size_t)nE * 8);
  std::vector<uint8_t> flags(nKF);
  std::vector<int> eI(nE), eJ(nE), ref(nMP);
  std::vector<float> mp((size_t)nMP * 3);
  rd(in, S.data(), S.size()); rd(in, flags.data(), nKF); rd(in, eI.data(), nE); rd(in, eJ.data(), nE); rd(in, M.data(), M.size());
  rd(in, mp.data(), mp.size()); rd(in, ref.data(), nMP);
  if (!in) { std::printf("short input\n"); return 2; }
  std::ofstream out(argv[2], std::ios::binary);
#ifdef EG_STUB_ENTRY
  g_out = &out;
#endif
  EssentialGraphView g;
  g.nKF = nKF; g.nE = nE; g.nMP = nMP; g.kfSim3 = S.data(); g.kfFlags = flags.data(); g.eI = eI.data(); g.eJ = eJ.data(); g.eSji = M.data();
  g.mpPos = nMP ? mp.data() : nullptr; g.mpRef = nMP ? ref.data() : nullptr;
  Optimizer::OptimizeEssentialGraph(g);
  wr(out, S.data(), S.size()); wr(out, mp.data(), mp.size()); wr(out, g.stats, 4); wr(out, g.chi2, 2);
#ifdef EG_STUB_ENTRY
  if (g_calls != 1 || g.stats[1] != 12 || g.chi2[1] != 0.25 || S[0] != 100.0) { std::printf("FAILED: the view does not hold the entry's results\n"); return 1; }
  std::printf("essential graph view ok\n");
#endif
  return out ? 0 : 1;
}
