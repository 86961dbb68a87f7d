// A program of its own over include/morb/camera_math.h, built by tests/test_camera_math_cpu.py with -fsanitize=address,undefined and
// linked with oracle/liboracle.so: the host build of the header against the oracle's independent KannalaBrandt8 (oracle/fisheye.cc),
// bit for bit on seeded random inputs with the two TUM-VI cameras; the pinhole model against values written out by hand; null_vector4
// on hand-made systems.  Prints the counts and, for triangulate_matches, how often each return occurred.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "morb/camera_math.h"

extern "C" {
float orc_kb8_triangulate_matches(const float* cam1_8, const float* cam2_8, float x1, float y1, float x2, float y2, const float* R12,
                                  const float* t12, float sigmaLevel, float unc, float* p3D);
void orc_kb8_project_f(const float* cam8, const float* v3, float* uv);
void orc_kb8_project_d(const float* cam8, const double* v3, double* uv);
void orc_kb8_unproject(const float* cam8, float x, float y, float* ray);
void orc_kb8_project_jac(const float* cam8, const double* v3, double* J6);
}

using morbcam::Camera;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++bad; } } while (0)

// splitmix64: the same stream wherever the program is built
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

// Examples/Stereo/TUM-VI.yaml: Camera1, Camera2, Stereo.T_c1_c2 (right-camera coordinates -> left-camera coordinates)
static const Camera kCam[2] = {
    {1, {(float)190.97847715128717, (float)190.9733070521226, (float)254.93170605935475, (float)256.8974428996504,
         (float)0.0034823894022493434, (float)0.0007150348452162257, (float)-0.0020532361418706202, (float)0.00020293673591811182}},
    {1, {(float)190.44236969414825, (float)190.4344384721956, (float)252.59949716835982, (float)254.91723064636983,
         (float)0.0034003170790442797, (float)0.001766278153469831, (float)-0.00266312569781606, (float)0.0003299517423931039}}};
static const float kRlr[9] = {(float)0.999999445773493,  (float)0.000791687752817,  (float)0.000694034010224,
                              (float)-0.000823363992158, (float)0.998899461915674,  (float)0.046895490788700,
                              (float)-0.000656143613644, (float)-0.046896036240590, (float)0.998899560146304};
static const float kTlr[3] = {(float)0.101063427414194, (float)0.001946204678584, (float)0.001015350132563};

// Rodrigues: the rotation by `angle` about the unit axis (ax, ay, az), row-major
static void rotation(double ax, double ay, double az, double angle, float* R) {
  const double n = std::sqrt(ax * ax + ay * ay + az * az), x = ax / n, y = ay / n, z = az / n, c = std::cos(angle), s = std::sin(angle), t = 1 - c;
  const double M[9] = {t * x * x + c, t * x * y - s * z, t * x * z + s * y, t * x * y + s * z, t * y * y + c, t * y * z - s * x,
                       t * x * z - s * y, t * y * z + s * x, t * z * z + c};
  for (int i = 0; i < 9; ++i) R[i] = (float)M[i];
}

static int histogram[6];   // accepted, -1 .. -5
static int tri_mismatch = 0, tri_cases = 0;
static float triangulate_both(const Camera& c1, const Camera& c2, const float* R12, const float* t12, float x1, float y1, float x2, float y2,
                              float sigma1, float unc) {
  float pa[3] = {-7.f, -7.f, -7.f}, pb[3] = {-7.f, -7.f, -7.f};
  const float a = morbcam::triangulate_matches(c1.p, c2.p, R12, t12, x1, y1, x2, y2, sigma1, unc, pa);
  const float b = orc_kb8_triangulate_matches(c1.p, c2.p, x1, y1, x2, y2, R12, t12, sigma1, unc, pb);
  ++tri_cases;
  if (std::memcmp(&a, &b, 4) != 0 || std::memcmp(pa, pb, 12) != 0) ++tri_mismatch;
  if (a > 0) CHECK(pa[2] == a); else CHECK(pa[0] == -7.f && pa[1] == -7.f && pa[2] == -7.f);
  return a;
}
static void count(float d) {
  if (d > 0) ++histogram[0];
  else if (d == -1.f || d == -2.f || d == -3.f || d == -4.f || d == -5.f) ++histogram[(int)-d];
  else { std::printf("FAILED triangulate_matches returned %g\n", (double)d); ++bad; }
}

int main(int argc, char** argv) {
  const int scale = argc > 1 ? std::atoi(argv[1]) : 1;   // (a multiplier of the counts, for a longer run by hand)
  const int nFloat = 300000 * scale, nDouble = 100000 * scale, nTri = 60000 * scale;

  // ---- KannalaBrandt8, float: points at |x|, |y| < 5 and z in (-5, 9); pixels within 300 of the principal point
  {
    int mp = 0, mu = 0;
    for (int i = 0; i < nFloat; ++i) {
      const Camera& c = kCam[i & 1];
      const float X[3] = {(float)uniform(-5, 5), (float)uniform(-5, 5), (float)uniform(-5, 9)};
      float a[2], b[2];
      morbcam::project(c, X, a[0], a[1]);
      orc_kb8_project_f(c.p, X, b);
      mp += std::memcmp(a, b, 8) != 0;
      const float px = c.p[2] + (float)uniform(-300, 300), py = c.p[3] + (float)uniform(-300, 300);
      float ra[3], rb[3];
      morbcam::unproject(c, px, py, ra);
      orc_kb8_unproject(c.p, px, py, rb);
      mu += std::memcmp(ra, rb, 12) != 0;
    }
    std::printf("project cases %d mismatches %d\nunproject cases %d mismatches %d\n", nFloat, mp, nFloat, mu);
    bad += mp + mu;
  }
  // ---- KannalaBrandt8, FP64 forms of the optimisers
  {
    int md = 0, mj = 0;
    for (int i = 0; i < nDouble; ++i) {
      const Camera& c = kCam[i & 1];
      const double X[3] = {uniform(-5, 5), uniform(-5, 5), uniform(-5, 9)};
      double a[2], b[2], Ja[6], Jb[6];
      morbcam::kb8_project_d(c.p, X, a);
      orc_kb8_project_d(c.p, X, b);
      md += std::memcmp(a, b, 16) != 0;
      morbcam::kb8_project_jac(c.p, X, Ja);
      orc_kb8_project_jac(c.p, X, Jb);
      mj += std::memcmp(Ja, Jb, 48) != 0;
    }
    std::printf("project_d cases %d mismatches %d\nproject_jac cases %d mismatches %d\n", nDouble, md, nDouble, mj);
    bad += md + mj;
  }
  // ---- TriangulateMatches.  Three kinds of case, a third each:
  //   0  the rig's own pose, a true point at 0.2 .. 12 m seen by both cameras, pixel noise of 0 .. 3 px on either side, sigma1 and unc the
  //      level sigma2 of a random octave, unc now and then 1e-3: accepted, -1 (far points: the baseline is 0.1 m), -4, -5;
  //   1  the rig's own pose, two unrelated pixels: -2 above all;
  //   2  a random rotation of any angle and a translation of up to 1 m, two unrelated pixels: -2, -3 and the rest.
  {
    for (int i = 0; i < nTri; ++i) {
      const int kind = i % 3, side = (i / 3) & 1;
      const Camera &c1 = kCam[side], &c2 = kCam[side ^ 1];
      float R12[9], t12[3], x1, y1, x2, y2;
      if (kind == 2) {
        rotation(uniform(-1, 1), uniform(-1, 1), uniform(-1, 1) + 1e-3, uniform(-3.14, 3.14), R12);
        for (int k = 0; k < 3; ++k) t12[k] = (float)uniform(-1, 1);
      } else {
        std::memcpy(R12, kRlr, sizeof R12);
        std::memcpy(t12, kTlr, sizeof t12);
      }
      const float sigma1 = (float)std::pow(1.44, (double)(next_u64() % 8));
      const float unc = next_u64() % 8 == 0 ? 1e-3f : (float)std::pow(1.44, (double)(next_u64() % 8));
      if (kind == 0) {
        const double z = std::exp(uniform(std::log(0.2), std::log(12.0)));
        const float X1[3] = {(float)(z * uniform(-1, 1)), (float)(z * uniform(-1, 1)), (float)z};
        float X2[3];   // R12^T (X1 - t12)
        for (int r = 0; r < 3; ++r) X2[r] = (R12[r] * (X1[0] - t12[0]) + R12[3 + r] * (X1[1] - t12[1])) + R12[6 + r] * (X1[2] - t12[2]);
        const double noise = next_u64() % 2 ? 0.0 : uniform(0, 3);
        morbcam::project(c1, X1, x1, y1);
        morbcam::project(c2, X2, x2, y2);
        x1 += (float)uniform(-noise, noise); y1 += (float)uniform(-noise, noise);
        x2 += (float)uniform(-noise, noise); y2 += (float)uniform(-noise, noise);
      } else {
        x1 = c1.p[2] + (float)uniform(-300, 300); y1 = c1.p[3] + (float)uniform(-300, 300);
        x2 = c2.p[2] + (float)uniform(-300, 300); y2 = c2.p[3] + (float)uniform(-300, 300);
      }
      count(triangulate_both(c1, c2, R12, t12, x1, y1, x2, y2, sigma1, unc));
    }
    // -3 by hand as well (the generator reaches it only through kind 2): camera 2 turned by 180 degrees about y, so that the point
    // (0.2, 0, 1) of camera 1 is (-0.1, 0, -1) in camera 2, behind it, on the line of the pixel of (0.1, 0, 1)
    {
      const float R12[9] = {-1, 0, 0, 0, 1, 0, 0, 0, -1}, t12[3] = {0.1f, 0, 0}, X1[3] = {0.2f, 0, 1}, X2[3] = {0.1f, 0, 1};
      float x1, y1, x2, y2;
      morbcam::project(kCam[0], X1, x1, y1);
      morbcam::project(kCam[1], X2, x2, y2);
      CHECK(triangulate_both(kCam[0], kCam[1], R12, t12, x1, y1, x2, y2, 1.f, 1.f) == -3.f);
    }
    std::printf("triangulate_matches cases %d mismatches %d\n", tri_cases, tri_mismatch);
    std::printf("triangulate_matches histogram accepted %d", histogram[0]);
    for (int k = 1; k <= 5; ++k) std::printf(" -%d %d", k, histogram[k]);
    std::printf("\n");
    bad += tri_mismatch;
  }

  // ---- Pinhole by hand: every quotient and product below is exact in float
  {
    const Camera pin{0, {500.f, 400.f, 320.f, 240.f, 9.f, 9.f, 9.f, 9.f}};   // (a pinhole camera ignores k0..k3)
    const float X[3] = {1.f, 2.f, 4.f};
    float u, v, ray[3];
    morbcam::project(pin, X, u, v);
    CHECK(u == 445.f && v == 440.f);
    morbcam::unproject(pin, 445.f, 440.f, ray);
    CHECK(ray[0] == 0.25f && ray[1] == 0.5f && ray[2] == 1.f);
    const float Y[3] = {-3.f, 0.f, 8.f};
    morbcam::project(pin, Y, u, v);
    CHECK(u == 132.5f && v == 240.f);
    morbcam::unproject(pin, 70.f, 40.f, ray);
    CHECK(ray[0] == -0.5f && ray[1] == -0.5f && ray[2] == 1.f);
  }

  // ---- null_vector4: the sheared system of new_map_points_math_check.cc, whose null vector is exactly (0, 0, 1, 0)
  {
    double v[4];
    const float A[16] = {-1, 0, 0, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, -1, 0, 0};
    morbcam::null_vector4(A, v);
    CHECK(v[3] == 0.0 && std::fabs(std::fabs(v[2]) - 1.0) < 1e-12);
  }
  std::printf("mismatches %d\n", bad);
  return bad != 0;
}
