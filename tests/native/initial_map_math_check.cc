// include/morb/initial_map_math.h, serially, as a stand-alone program for the sanitizers (tests/test_initial_map_cpu.py builds it with
// -fsanitize=address,undefined): the depth keys keep the order of the floats and invert exactly, the bit-by-bit selection the kernel runs on
// them finds the depth of rank (n - 1) / 2 of a sort for every n from 1 to 70 and for data with ties, negative values and both zeros,
// the status bits, the scaling, the camera centre and the fields of UpdateNormalAndDepth against plain double arithmetic.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "morb/initial_map_math.h"

using namespace morbim;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

// the kernel's selection: fix the key of the wanted rank from the top bit down by counting
static float select_rank(const std::vector<float>& z, int rank) {
  uint32_t prefix = 0, mask = 0;
  for (int bit = 31; bit >= 0; --bit) {
    int cnt = 0;
    for (float v : z) { const uint32_t k = im_depth_key(v); cnt += ((k & mask) == prefix && !((k >> bit) & 1u)) ? 1 : 0; }
    if (rank >= cnt) { rank -= cnt; prefix |= 1u << bit; }
    mask |= 1u << bit;
  }
  return im_key_depth(prefix);
}

int main() {
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> U(-20.f, 20.f);
  const float special[] = {0.f, -0.f, 1.f, -1.f, 1e-38f, -1e-38f, 3.4e38f, -3.4e38f, 5.5f, 5.5f};
  for (float a : special)
    for (float b : special) {
      CHECK((a < b) == (im_depth_key(a) < im_depth_key(b)) || (a == 0.f && b == 0.f));
      uint32_t ua, ub; float r = im_key_depth(im_depth_key(a));
      memcpy(&ua, &a, 4); memcpy(&ub, &r, 4);
      CHECK(ua == ub);
    }
  CHECK(im_median_rank(1) == 0 && im_median_rank(2) == 0 && im_median_rank(3) == 1 && im_median_rank(50) == 24 && im_median_rank(51) == 25);
  CHECK(im_median_depth(nullptr, 0) == -1.f);
  for (int n = 1; n <= 70; ++n)
    for (int rep = 0; rep < 4; ++rep) {
      std::vector<float> z(n);
      for (float& v : z) v = rep == 3 ? (float)(int)U(rng) / 4 : U(rng) + (rep == 1 ? 25.f : 0.f);   // rep 3: many ties, rep 1: all positive
      if (rep == 2 && n > 2) { z[0] = 0.f; z[1] = -0.f; }
      const float want = im_median_depth(z.data(), n), got = select_rank(z, im_median_rank(n));
      CHECK(want == got);
    }
  CHECK(im_status(5.f, 50, 50) == IM_OK && im_status(5.f, 49, 50) == IM_RESET_COUNT && im_status(-1.f, 50, 50) == IM_RESET_MEDIAN);
  CHECK(im_status(-0.5f, 3, 50) == (IM_RESET_MEDIAN | IM_RESET_COUNT) && im_status(0.f, 50, 50) == IM_OK);
  {
    const float X[3] = {1.5f, -2.f, 7.25f};
    CHECK(im_kf1_depth(X) == 7.25f);
    float Y[3] = {1.5f, -2.f, 7.25f};
    const float inv = 4.0f / 5.5f;
    im_scale3(Y, inv);
    CHECK(Y[0] == 1.5f * inv && Y[1] == -2.f * inv && Y[2] == 7.25f * inv);
    // a rotation about z by 0.3 and a translation: Ow = -R^T t
    const float c = std::cos(0.3f), s = std::sin(0.3f);
    const float T[12] = {c, -s, 0, s, c, 0, 0, 0, 1, 0.4f, -0.1f, 0.05f};
    float Ow[3];
    im_camera_centre(T, Ow);
    const double w[3] = {-((double)c * 0.4f + (double)s * -0.1f), -((double)-s * 0.4f + (double)c * -0.1f), -0.05f};
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(Ow[k] - w[k]) < 1e-6);
    float nrm[3], d2[2];
    im_point_fields(X, Ow, 1.44f, 3.583f, nrm, d2);
    double a[3], b[3], la = 0, lb = 0;
    for (int k = 0; k < 3; ++k) { a[k] = X[k]; b[k] = (double)X[k] - Ow[k]; la += a[k] * a[k]; lb += b[k] * b[k]; }
    la = std::sqrt(la); lb = std::sqrt(lb);
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(nrm[k] - (a[k] / la + b[k] / lb) / 2) < 1e-6);
    CHECK(std::fabs(d2[0] - lb * 1.44) < 1e-5 && std::fabs(d2[1] - lb * 1.44 / 3.583) < 1e-5);
  }
  std::printf("initial map math ok\n");
  return 0;
}
