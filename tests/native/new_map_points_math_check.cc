// A program of its own over include/morb/new_map_points_math.h, built by tests/test_new_map_points_cpu.py with
// -fsanitize=address,undefined: the enums by name, and the header's functions on hand-made inputs: a point recovered from its two
// projections (pinhole and KannalaBrandt8), the two ends the corpus cannot reach (x3Dh(3) == 0 and a zero distance), UnprojectStereo,
// the point's derived fields and the pair gate.
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "morb/new_map_points_math.h"

using namespace morbnmp;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++bad; } } while (0)

int main() {
#define MORB_NMP_X(n) std::printf("status %s %d\n", #n, (int)NMP_##n);
  MORB_NMP_STATUS(MORB_NMP_X)
#undef MORB_NMP_X
#define MORB_NMP_X(n) std::printf("stat %s %d\n", #n, (int)NMP_S_##n);
  MORB_NMP_STATS(MORB_NMP_X)
#undef MORB_NMP_X
  std::printf("len %d %d\n", (int)NMP_STATUS_LEN, (int)NMP_STATS_LEN);

  const float sf[8] = {1.f, 1.2f, 1.44f, 1.728f, 2.0736f, 2.48832f, 2.985984f, 3.5831808f};
  float s2[8];
  for (int i = 0; i < 8; ++i) s2[i] = sf[i] * sf[i];
  Params P{};
  P.fx = 458.654f; P.fy = 457.296f; P.cx = 367.215f; P.cy = 248.375f; P.invfx = 1.0f / P.fx; P.invfy = 1.0f / P.fy;
  P.mb = 0.11f; P.mbf = P.fx * P.mb; P.ratioFactor = 1.8f; P.thFarPoints = 0.f; P.inertial = 0; P.farPoints = 0;
  P.scaleFactors = sf; P.levelSigma2 = s2;
  const Camera pin{0, {P.fx, P.fy, P.cx, P.cy, 0, 0, 0, 0}};
  const Camera kb8{1, {190.978f, 190.973f, 254.932f, 256.897f, 0.0034824f, 0.00071503f, -0.0020532f, 0.00020294f}};

  // two cameras one metre apart along x, a point at (0.4, -0.2, 5)
  const float T1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, T2[12] = {1, 0, 0, -1, 0, 1, 0, 0, 0, 0, 1, 0};
  const float W1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, W2[12] = {1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0};
  const float X[3] = {0.4f, -0.2f, 5.f}, X2[3] = {X[0] - 1.f, X[1], X[2]};   // the point in either camera
  for (const Camera& c : {pin, kb8}) {
    Side a{}, b{};
    a.Tcw = T1; a.Twc = W1; b.Tcw = T2; b.Twc = W2;
    b.Ow[0] = 1.f;
    a.cam = b.cam = c;
    float uv[2];
    morbcam::project(c, X, uv[0], uv[1]); a.x = a.rawx = uv[0]; a.y = a.rawy = uv[1];
    morbcam::project(c, X2, uv[0], uv[1]); b.x = b.rawx = uv[0]; b.y = b.rawy = uv[1];
    a.ur = b.ur = a.depth = b.depth = -1.f;
    float x3D[3]; int fl = -1;
    const int st = nmp_decide(P, a, b, x3D, &fl);
    CHECK(st == NMP_TRIANGULATED && fl == 0);
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(x3D[k] - X[k]) < 1e-3f);
    float ray[3];
    morbcam::unproject(c, a.x, a.y, ray);
    CHECK(std::fabs(ray[0] - X[0] / X[2]) < 1e-5f && std::fabs(ray[1] - X[1] / X[2]) < 1e-5f);
    // a centre that is not the pose's: the point itself, so that dist2 == 0 exactly (the pose's own centre gives z2 == 0 first)
    for (int k = 0; k < 3; ++k) b.Ow[k] = x3D[k];
    CHECK(nmp_decide(P, a, b, x3D, &fl) == NMP_ZERO_DIST);
    b.Ow[0] = 1.f; b.Ow[1] = b.Ow[2] = 0.f;
    // the far test, then a stereo feature in keyframe 1 with its true depth: still triangulated, counted as a stereo point
    Params Q = P; Q.farPoints = 1; Q.thFarPoints = 4.f;
    CHECK(nmp_decide(Q, a, b, x3D, &fl) == NMP_FAR_POINT);
    if (!c.kb8) {
      a.bStereo = 1; a.depth = X[2]; a.ur = a.x - P.mbf / X[2];
      CHECK(nmp_decide(P, a, b, x3D, &fl) == NMP_TRIANGULATED && fl == 1);
      a.ur += 9.f;
      CHECK(nmp_decide(P, a, b, x3D, &fl) == NMP_REPROJ1);
    }
  }

  // x3Dh(3) == 0: the second "pose" is sheared so that the null vector of A is exactly (0, 0, 1, 0) while the rays are 45 degrees apart
  {
    const float S2[12] = {1, 0, 0, 1, 0, 1, 0, 0, 1, 0, 1, 0};
    const float xc[3] = {0, 0, 1};
    float x3D[3] = {7, 7, 7};
    CHECK(!nmp_triangulate(xc, xc, T1, S2, x3D));
    CHECK(x3D[0] == 7.f);
    Side a{}, b{};
    a.Tcw = T1; a.Twc = W1; b.Tcw = S2; b.Twc = W2;
    a.cam = b.cam = pin;
    a.x = b.x = P.cx; a.y = b.y = P.cy;
    a.ur = b.ur = a.depth = b.depth = -1.f;
    int fl = -1;
    CHECK(nmp_decide(P, a, b, x3D, &fl) == NMP_TRIANGULATE_FALSE && fl == 0);
  }

  // UnprojectStereo, the derived fields, the gate
  {
    float x3D[3];
    CHECK(!nmp_unproject_stereo(0.f, 10, 10, P.cx, P.cy, P.invfx, P.invfy, W2, x3D));
    CHECK(nmp_unproject_stereo(2.f, P.cx, P.cy, P.cx, P.cy, P.invfx, P.invfy, W2, x3D) && x3D[0] == 1.f && x3D[1] == 0.f && x3D[2] == 2.f);
    const float O1[3] = {0, 0, 0}, O2[3] = {2, 0, 0}, Pw[3] = {1, 0, 1};
    float n[3], mx, mn;
    nmp_point_fields(Pw, O1, O2, O1, sf[2], sf[7], n, &mx, &mn);
    CHECK(n[0] == 0.f && n[1] == 0.f && std::fabs(n[2] - std::sqrt(0.5f)) < 1e-6f);
    CHECK(std::fabs(mx - std::sqrt(2.f) * 1.44f) < 1e-6f && std::fabs(mn - mx / sf[7]) < 1e-7f);
    CHECK(nmp_descriptor_from_kf2(1) && !nmp_descriptor_from_kf2(0));
    CHECK(nmp_pair_gate(false, O1, O2, 2.5f, 0.f) && !nmp_pair_gate(false, O1, O2, 2.0f, 0.f));
    CHECK(nmp_pair_gate(true, O1, O2, 0.f, 201.f) && !nmp_pair_gate(true, O1, O2, 0.f, 199.f));
  }
  std::printf("mismatches %d\n", bad);
  return bad != 0;
}
