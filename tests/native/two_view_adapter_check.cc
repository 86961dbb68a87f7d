// Drives ORB_SLAM3::TwoViewReconstruction in the reference's signature (include/morb/TwoViewReconstruction.h) on the GPU with the mock
// keypoints / SE3f / Point3f of tests/native/mock_ref and tests/native/mock_two_view: one reconstructor, Reconstruct on every problem of
// the input file in turn, in ONE process, so that the second call continues the rand() stream of the first.
// tests/test_two_view_adapter_gpu.py writes the problems and compares what this program writes with the CPU oracle fed the same stream.
//   in:  int32 K; float K4[4], sigma; int32 iterations; per problem: int32 n1, n2; float kp1[n1][2], kp2[n2][2]; int32 matches12[n1]
//   out: per problem: int32 ok, vP3D.size(), vbTriangulated.size(); float R[9], t[3]; float vP3D[n1][3]; uint8 vbTriangulated[n1];
//        then int32 the next rand() value: where the calls left the stream.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "two_view_mock.h"            // tests/native/mock_two_view
#include "TwoViewReconstruction.h"    // include/morb

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n = 1) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  FILE* w = fopen(argv[2], "wb");
  if (!f || !w) return 2;
  int K, iterations;
  float K4[4], sigma;
  if (!(rd(f, &K) && rd(f, K4, 4) && rd(f, &sigma) && rd(f, &iterations))) return 3;
  Eigen::Matrix3f Km;
  Km(0, 0) = K4[0]; Km(1, 1) = K4[1]; Km(0, 2) = K4[2]; Km(1, 2) = K4[3]; Km(0, 1) = 0.f; Km(1, 0) = 0.f; Km(2, 0) = 0.f; Km(2, 1) = 0.f;
  TwoViewReconstruction tvr(Km, sigma, iterations);
  int found = 0;
  for (int k = 0; k < K; ++k) {
    int n1, n2;
    if (!(rd(f, &n1) && rd(f, &n2))) return 3;
    std::vector<float> a((size_t)n1 * 2), b((size_t)n2 * 2);
    std::vector<int> m(n1);
    if (!(rd(f, a.data(), a.size()) && rd(f, b.data(), b.size()) && rd(f, m.data(), m.size()))) return 3;
    std::vector<cv::KeyPoint> k1(n1), k2(n2);
    for (int i = 0; i < n1; ++i) { k1[i].pt.x = a[(size_t)i * 2]; k1[i].pt.y = a[(size_t)i * 2 + 1]; }
    for (int i = 0; i < n2; ++i) { k2[i].pt.x = b[(size_t)i * 2]; k2[i].pt.y = b[(size_t)i * 2 + 1]; }
    Sophus::SE3f T21;
    std::vector<cv::Point3f> vP3D(3, cv::Point3f(9.f, 9.f, 9.f));   // stale content a true return must replace
    std::vector<bool> vbTriangulated(2, true);
    const bool ok = tvr.Reconstruct(k1, k2, m, T21, vP3D, vbTriangulated);
    const int hdr[3] = {ok, (int)vP3D.size(), (int)vbTriangulated.size()};
    fwrite(hdr, 4, 3, w);
    fwrite(T21.R, 4, 9, w);
    fwrite(T21.t, 4, 3, w);
    std::vector<float> P((size_t)n1 * 3, 0.f);
    std::vector<uint8_t> tri(n1 > 0 ? n1 : 1, 0);
    if (ok)
      for (int i = 0; i < n1; ++i) { P[(size_t)i * 3] = vP3D[i].x; P[(size_t)i * 3 + 1] = vP3D[i].y; P[(size_t)i * 3 + 2] = vP3D[i].z; tri[i] = vbTriangulated[i]; }
    fwrite(P.data(), 4, P.size(), w);
    fwrite(tri.data(), 1, n1, w);
    found += ok;
  }
  const int marker = rand();
  fwrite(&marker, 4, 1, w);
  fclose(f);
  fclose(w);
  printf("problems %d reconstructed %d\n", K, found);
  return 0;
}
