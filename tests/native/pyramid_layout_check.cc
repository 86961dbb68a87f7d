// Host build of morb_slam_amd/csrc/pyramid_layout.h (the stored layout of the image pyramid and the byte range each of its readers
// can touch) for tests/test_pyramid_layout_cpu.py, a program of its own so that it can run under sanitizers.  It sweeps image
// sizes, scale factors, level counts and image counts and checks, through the header's extent functions, that no reader leaves
// [0, pyrBytes + kPyrTail), that rows are 64-byte aligned with the interior at byte 3, that three border pixels are stored on every
// side, and that the bench shape takes the bytes the layout promises.  The blur's and FAST's extents are also recomputed here from
// the kernels' address expressions, window by window, and must lie inside what the header states.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "pyramid_layout.h"

using namespace morb;

static long bad = 0, cases = 0;
#define CHECK(c) do { if (!(c)) { if (++bad <= 20) std::printf("FAILED %s  (W %d H %d f %.1f L %d nimg %d level %d)\n", #c, W, H, f, L, nimg, l); } } while (0)

static void inv_scales(float f, int L, float* inv) {   // ORBextractor.cc:413-443
  float s = 1.0f;
  for (int i = 0; i < L; ++i) { if (i) s *= f; inv[i] = 1.0f / s; }
}
static bool legal(int W, int H, const float* inv, int L) {   // configure(): every level between 76 and 4095 px
  for (int l = 0; l < L; ++l) {
    const int w = pyr_level_dim(W, inv[l]), h = pyr_level_dim(H, inv[l]);
    if (w < 2 * EDGE + 35 + 3 || h < 2 * EDGE + 35 + 3 || w > 4095 || h > 4095) return false;
  }
  return true;
}

// the blur's loads as k_blur issues them: strips of 8 columns, source rows y0 - 3 + min(k, lastRow), k < 6 + rows per strip
constexpr int kBlurStripRows = 24;   // MORB_BT_ROWS
static PyrExtent blur_by_enumeration(const PyrLevelLayout& v) {
  PyrExtent e = {1ll << 60, -1};
  for (int y0 = 0; y0 < v.h; ++y0)   // (every strip origin, not only multiples of the strip height)
    for (int x = 0; x < v.w; x += 8) {
      const long long src = (long long)(kPyrPad + y0 - 3) * v.pstride + (kPyrPad - 3) + x;
      const int lastRow = v.h + 2 * kPyrPad - 1 - (kPyrPad + y0 - 3);
      e.lo = std::min(e.lo, src);
      e.hi = std::max(e.hi, src + (long long)std::min(6 + kBlurStripRows - 1, lastRow) * v.pstride + 15);
    }
  return e;
}
// FAST's tile loads as configure() lays the cells out and k_fastw reads them: th rows of P bytes from winOff - 1
static PyrExtent fast_by_enumeration(const PyrLevelLayout& v, int P) {
  const int minB = EDGE - 3, maxX = v.w - EDGE + 3, maxY = v.h - EDGE + 3;
  const float width = (float)(maxX - minB), height = (float)(maxY - minB);
  const int nCols = (int)(width / 35.f), nRows = (int)(height / 35.f);
  const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
  PyrExtent e = {1ll << 60, -1};
  for (int ci = 0; ci < nRows; ++ci)
    for (int c0 = 0; c0 < nCols; ++c0) {
      const int X0 = minB + c0 * wCell, iniY = minB + ci * hCell;
      int tw = std::min(X0 + wCell + 6, maxX) - X0, th = std::min(iniY + hCell + 6, maxY) - iniY;
      if (iniY >= maxY - 3 || tw <= 6 || th <= 6) continue;
      const long long base = (long long)(kPyrPad + iniY) * v.pstride + kPyrPad + X0 - 1;
      e.lo = std::min(e.lo, base);
      e.hi = std::max(e.hi, base + (long long)(th - 1) * v.pstride + P - 1);
    }
  return e;
}

static void check_case(int W, int H, float f, int L, int nimg) {
  float inv[16];
  inv_scales(f, L, inv);
  int l = -1;
  if (!legal(W, H, inv, L)) return;
  ++cases;
  PyrLevelLayout lv[16];
  const unsigned long long total = pyr_layout(W, H, inv, L, nimg, lv);
  unsigned long long expectOff = 0;
  for (l = 0; l < L; ++l) {
    const PyrLevelLayout& v = lv[l];
    CHECK(v.off == expectOff);   // blocks follow each other without gaps or overlap
    expectOff += v.img * (unsigned)nimg;
    CHECK(v.pstride % 64 == 0 && v.off % 64 == 0 && v.img % 64 == 0);          // rows are 64-byte aligned
    CHECK(pyr_interior(v.pstride) == pyr_at(v, 0, 0) && pyr_at(v, 0, 0) % v.pstride == 3);   // the interior sits at byte 3 of its row
    CHECK(kPyrPad >= 3 && v.pstride >= v.w + 2 * kPyrPad && v.img == (unsigned long long)(v.h + 2 * kPyrPad) * v.pstride);
    CHECK(pyr_at(v, -3, -3) >= 0 && pyr_at(v, v.w + 2, v.h + 2) < (long long)v.img);   // three stored border pixels on every side
    CHECK(pyr_at(v, -3, 0) / v.pstride == pyr_at(v, v.w + 2, 0) / v.pstride);        // ... of one row
    for (int P : {48, 64, 80}) {
      const PyrExtent e[6] = {pyr_blur_extent(v), pyr_fast_extent(v, P), pyr_describe_extent(v), pyr_stereo_extent(v),
                              pyr_resize_extent(v), pyr_gather_extent(v)};
      for (int k = 0; k < 6; ++k)
        for (int img : {0, nimg - 1}) {
          const long long b = (long long)(v.off + v.img * (unsigned)img);
          CHECK(e[k].lo <= e[k].hi);
          CHECK(b + e[k].lo >= 0);
          CHECK(b + e[k].hi < (long long)total + kPyrTail);
        }
      const PyrExtent fe = fast_by_enumeration(v, P);
      CHECK(fe.hi >= 0 && fe.lo >= e[1].lo && fe.hi <= e[1].hi);
      CHECK(pyr_extents_ok(lv, L, nimg, total, P, false) && pyr_extents_ok(lv, L, nimg, total, P, true));
    }
    const PyrExtent be = blur_by_enumeration(v), bh = pyr_blur_extent(v);
    CHECK(be.lo == bh.lo && be.hi == bh.hi);
    // what a reader USES is stored: the blur's columns -3 .. w + 2 and rows -3 .. h + 2; everything else reads the interior
    CHECK(kBlurReach <= kPyrPad);
  }
  l = -1;
  CHECK(expectOff == total);
}

int main() {
  const float factors[] = {1.1f, 1.2f, 1.5f, 2.0f};
  const int levels[] = {1, 3, 8}, images[] = {1, 3};
  for (float f : factors)
    for (int L : levels) {
      float inv[16];
      inv_scales(f, L, inv);
      std::vector<std::pair<int, int>> shapes = {{752, 480}, {1920, 1080}, {512, 512}, {640, 480}};
      int minN = 76;
      while (pyr_level_dim(minN, inv[L - 1]) < 76) ++minN;   // the smallest legal image
      shapes.push_back({minN, minN});
      shapes.push_back({minN + 1, minN});
      for (int lvl : {0, std::min(2, L - 1)}) {   // widths whose level `lvl` has no row slack at all ((w + 6) % 64 == 0), one below, one above
        int W = minN;
        while ((pyr_level_dim(W, inv[lvl]) + 2 * kPyrPad) % 64 != 0) ++W;
        for (int d = -1; d <= 1; ++d) { shapes.push_back({W + d, minN}); shapes.push_back({W + d, minN + 197}); }
        int W2 = W + 64;   // and a second such width further up
        while ((pyr_level_dim(W2, inv[lvl]) + 2 * kPyrPad) % 64 != 0) ++W2;
        for (int d = -1; d <= 1; ++d) shapes.push_back({W2 + d, minN + 1});
      }
      for (auto s : shapes)
        for (int nimg : images) check_case(s.first, s.second, f, L, nimg);
    }
  {
    // the bench shape: 752 x 480, scale 1.2, 8 levels -> 1 199 552 bytes per image (1 431 744 with the full 19-px pad)
    float inv[16];
    inv_scales(1.2f, 8, inv);
    PyrLevelLayout lv[16];
    for (int nimg : {1, 3, 1024}) {
      const int W = 752, H = 480, L = 8, l = -1; const float f = 1.2f;
      CHECK(pyr_layout(W, H, inv, L, nimg, lv) == 1199552ull * (unsigned)nimg);
    }
    const int W = 314, H = 273, L = 8, nimg = 1, l = 0; const float f = 1.2f;
    pyr_layout(W, H, inv, L, nimg, lv);
    CHECK(lv[0].pstride == 320 && lv[7].h == 76);   // the GPU test's shape: no slack at level 0, the smallest top level
  }
  {
    const int W = 0, H = 0, L = 0, nimg = 0, l = -1; const float f = 0.f;
    CHECK(pyr_stereo_scale_ok(1.1f) && pyr_stereo_scale_ok(1.2f) && pyr_stereo_scale_ok(2.0f) && !pyr_stereo_scale_ok(2.5f));
  }
  std::printf("cases %ld mismatches %ld\n", cases, bad);
  return bad != 0;
}
