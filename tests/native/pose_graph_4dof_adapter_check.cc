// Optimizer::OptimizeEssentialGraph4DoF(PoseGraph4DoFView&) of include/morb/Optimizer.h on one problem read from a file.
// Run as `pose_graph_4dof_adapter_check <in.bin> <out.bin>`; tests/test_pose_graph_4dof_adapter_gpu.py compares what it dumps with the C entry
// called from Python.  Built with -DPG4_STUB_ENTRY (tests/test_pose_graph_4dof_cpu.py, under -fsanitize=address,undefined, no library and no
// GPU) the C entries the call reaches are stubs defined here: morb_optimize_essential_graph_4dof records its arguments into out.bin and
// returns canned results, which the program checks the view holds afterwards.
// in.bin: int nKF, nE, nMP; double kfPose[nKF][12], kfBody[nKF][12]; uint8 kfFixed[nKF]; float Tcb12[12]; int eI[nE], eJ[nE]; double eTij[nE][12];
// float mpPos[nMP][3]; int mpRef[nMP]; double kfScw[nKF][8].
// out.bin: kfPose, mpPos, stats[4], chi2[2] after the call (stubbed: the recorded arguments in in.bin's layout come first).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "Optimizer.h"

using namespace ORB_SLAM3;

template <class T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), n * sizeof(T)); }
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

#ifdef PG4_STUB_ENTRY
static std::ofstream* g_out = nullptr;
static int g_calls = 0;
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
int morb_optimizer_create(morb_optimizer** out, int) { static int token; *out = reinterpret_cast<morb_optimizer*>(&token); return MORB_OK; }
int morb_optimizer_set_exact_order(morb_optimizer*, int) { return MORB_OK; }
const char* morb_last_error(void) { return "stub"; }
int morb_optimize_essential_graph_4dof(morb_optimizer* o, int nKF, double* kfPose, const double* kfBody, const uint8_t* kfFixed, const float* Tcb12, int nE,
                                       const int* eI, const int* eJ, const double* eTij, int nMP, float* mpPos, const int* mpRef, const double* kfScw,
                                       int* stats4, double* chi2) {
  ++g_calls;
  if (!o) return MORB_ERR_INVALID;
  const int hd[3] = {nKF, nE, nMP};
  wr(*g_out, hd, 3); wr(*g_out, kfPose, (size_t)nKF * 12); wr(*g_out, kfBody, (size_t)nKF * 12); wr(*g_out, kfFixed, nKF); wr(*g_out, Tcb12, 12);
  wr(*g_out, eI, nE); wr(*g_out, eJ, nE); wr(*g_out, eTij, (size_t)nE * 12); wr(*g_out, mpPos, (size_t)nMP * 3); wr(*g_out, mpRef, nMP);
  if (nMP) wr(*g_out, kfScw, (size_t)nKF * 8);
  for (int i = 0; i < nKF * 12; ++i) kfPose[i] = 100.0 + i;
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
  std::vector<double> P((size_t)nKF * 12), B((size_t)nKF * 12), M((size_t)nE * 12), scw((size_t)nKF * 8);
  std::vector<uint8_t> fixed(nKF);
  std::vector<int> eI(nE), eJ(nE), ref(nMP);
  std::vector<float> mp((size_t)nMP * 3);
  PoseGraph4DoFView g;
  rd(in, P.data(), P.size()); rd(in, B.data(), B.size()); rd(in, fixed.data(), nKF); rd(in, g.Tcb12, 12); rd(in, eI.data(), nE); rd(in, eJ.data(), nE);
  rd(in, M.data(), M.size()); rd(in, mp.data(), mp.size()); rd(in, ref.data(), nMP); rd(in, scw.data(), scw.size());
  if (!in) { std::printf("short input\n"); return 2; }
  std::ofstream out(argv[2], std::ios::binary);
#ifdef PG4_STUB_ENTRY
  g_out = &out;
#endif
  g.nKF = nKF; g.nE = nE; g.nMP = nMP; g.kfPose = P.data(); g.kfBody = B.data(); g.kfFixed = fixed.data(); g.eI = eI.data(); g.eJ = eJ.data(); g.eTij = M.data();
  g.mpPos = nMP ? mp.data() : nullptr; g.mpRef = nMP ? ref.data() : nullptr; g.kfScw = nMP ? scw.data() : nullptr;
  Optimizer::OptimizeEssentialGraph4DoF(g);
  wr(out, P.data(), P.size()); wr(out, mp.data(), mp.size()); wr(out, g.stats, 4); wr(out, g.chi2, 2);
#ifdef PG4_STUB_ENTRY
  if (g_calls != 1 || g.stats[1] != 12 || g.chi2[1] != 0.25 || P[0] != 100.0) { std::printf("FAILED: the view does not hold the entry's results\n"); return 1; }
  std::printf("pose graph 4dof view ok\n");
#endif
  return out ? 0 : 1;
}
