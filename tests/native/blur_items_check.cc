// Host build of morb_slam_amd/csrc/blur_items.h (how k_blur numbers its 8-px x BT_ROWS strips across the levels of an image and
// turns an item number back into level, column and row) for tests/test_blur_items_cpu.py, a program of its own so that it can run
// under sanitizers.  For every pyramid it walks all items the way the kernel does (blur_locate: the span search and the 24-bit
// multiply-and-shift division) and checks that
//   * every pixel of every level is covered by exactly one (item, row, column),
//   * no item starts outside its level, and items follow each other along a strip row (a wave's loads and stores stay contiguous),
//   * the division agrees with the plain one for every item of every span, with both factors below 2^24 and the product below 2^32,
//   * an image takes ceil(items / 64) waves: the numbering unit is the image, so at most its last wave is partly filled.
#include <cmath>
#include <cstdio>
#include <vector>

#include "blur_items.h"
#include "pyramid_layout.h"

using namespace morb;

static long bad = 0, cases = 0;
static const char* what = "";
#define CHECK(c) do { if (!(c)) { if (++bad <= 20) std::printf("FAILED %s  (%s)\n", #c, what); } } while (0)

static int check_levels(const char* name, const std::vector<int>& w, const std::vector<int>& h) {
  what = name;
  ++cases;
  const int L = (int)w.size();
  std::vector<BlurSpan> sp(4 * L + 4);
  int items = -1;
  const int ns = blur_build_spans(w.data(), h.data(), L, sp.data(), (int)sp.size(), &items);
  CHECK(ns >= L);
  if (ns < L) return 0;
  long long strips = 0;
  for (int l = 0; l < L; ++l) strips += (long long)blur_strips_x(w[l]) * blur_strips_y(h[l]);
  CHECK(items == strips);
  // spans: whole strip rows of one level, in order, without gaps; the division constants fit the 24-bit multiply
  int base = 0, level = 0, sy = 0;
  for (int k = 0; k < ns; ++k) {
    const BlurSpan& s = sp[k];
    if (s.level != level) { CHECK(sy == blur_strips_y(h[level]) && s.level == level + 1); level = s.level; sy = 0; }
    CHECK(s.itemBase == base && s.sy0 == sy && s.nsy >= 1 && s.nsx == blur_strips_x(w[level]));
    const long long J = (long long)s.nsx * s.nsy;
    CHECK(J <= kBlurSpanItems && s.magic < (1u << 24) && s.shift < 32 && (unsigned long long)(J - 1) * s.magic < (1ull << 32));
    for (long long j = 0; j < J; ++j)
      if (blur_div((unsigned)j, s.magic, s.shift) != (unsigned)(j / s.nsx)) { CHECK(!"blur_div == j / nsx"); break; }
    base += (int)J; sy += s.nsy;
  }
  CHECK(level == L - 1 && sy == blur_strips_y(h[L - 1]) && base == items);
  // coverage, item by item
  std::vector<std::vector<unsigned char>> cover(L);
  for (int l = 0; l < L; ++l) cover[l].assign((size_t)w[l] * h[l], 0);
  BlurItem prev = {-1, 0, 0};
  for (int i = 0; i < items; ++i) {
    const BlurItem it = blur_locate(sp.data(), ns, i);
    CHECK(it.level >= 0 && it.level < L);
    if (it.level < 0 || it.level >= L) break;
    CHECK(it.x >= 0 && it.x < w[it.level] && it.x % BT_PX == 0 && it.y0 >= 0 && it.y0 < h[it.level] && it.y0 % BT_ROWS == 0);
    if (!(it.x >= 0 && it.x < w[it.level] && it.y0 >= 0 && it.y0 < h[it.level])) break;
    // the next item is the strip to the right, else the first strip of the next strip row, else the first strip of the next level
    if (prev.level >= 0) {
      const bool right = it.level == prev.level && it.y0 == prev.y0 && it.x == prev.x + BT_PX;
      const bool wrap = it.level == prev.level && it.y0 == prev.y0 + BT_ROWS && it.x == 0 && prev.x + BT_PX >= w[prev.level];
      const bool next = it.level == prev.level + 1 && it.y0 == 0 && it.x == 0 && prev.x + BT_PX >= w[prev.level] && prev.y0 + BT_ROWS >= h[prev.level];
      CHECK(right || wrap || next);
    } else {
      CHECK(it.level == 0 && it.x == 0 && it.y0 == 0);
    }
    prev = it;
    for (int r = 0; r < BT_ROWS && it.y0 + r < h[it.level]; ++r)        // rows past the bottom: computed, not stored
      for (int c = 0; c < BT_PX && it.x + c < w[it.level]; ++c)         // columns >= w: the row's alignment slack
        ++cover[it.level][(size_t)(it.y0 + r) * w[it.level] + it.x + c];
  }
  long long holes = 0;
  for (int l = 0; l < L; ++l)
    for (unsigned char c : cover[l]) holes += c != 1;
  CHECK(holes == 0);
  // the numbering unit is the image: ceil(items / 64) waves, all full but the last
  const int waves = blur_waves(items);
  CHECK(waves == (items + 63) / 64 && (long long)waves * 64 - items < 64);
  return waves;
}

static int check_image(const char* name, int W, int H, float f, int L) {
  std::vector<int> w(L), h(L);
  float s = 1.0f;
  for (int l = 0; l < L; ++l) {   // the extractor's level sizes (ORBextractor.cc:413-443, :1091-1092)
    if (l) s *= f;
    w[l] = pyr_level_dim(W, 1.0f / s); h[l] = pyr_level_dim(H, 1.0f / s);
  }
  return check_levels(name, w, h);
}

int main() {
  static_assert(BT_ROWS == 24 && BT_PX == 8, "the figures below are for 8 x 24 strips");
  const int bench = check_image("752x480 f1.2 L8", 752, 480, 1.2f, 8);
  what = "752x480: waves per image";
  CHECK(bench == 94);   // 5995 strips; the 256-px x 192-row tiles this numbering replaced launched 152 waves
  check_image("333x217 f1.2 L4", 333, 217, 1.2f, 4);
  check_image("601x377 f1.1 L6", 601, 377, 1.1f, 6);
  check_image("120x90 f1.2 L2", 120, 90, 1.2f, 2);
  check_image("91x91 f1.2 L2", 91, 91, 1.2f, 2);          // the smallest image configure() accepts with two levels (76 x 76 on top)
  check_image("1920x1080 f1.2 L8", 1920, 1080, 1.2f, 8);
  check_image("4095x4095 f1.2 L8", 4095, 4095, 1.2f, 8);  // levels of more than kBlurSpanItems strips: several spans per level
  // levels narrower than a strip, shorter than a strip, and both, between ordinary ones
  check_levels("narrow and short levels", {100, 5, 100, 3, 8, 9, 1}, {50, 100, 7, 3, 24, 25, 1});
  check_levels("one pixel", {1}, {1});
  check_levels("one strip row of 32768 strips", {8 * kBlurSpanItems, 16}, {30, 16});   // the widest level: one strip row per span
  {
    what = "too wide";   // refused, not mis-divided
    int w = 8 * (kBlurSpanItems + 1), h = 8, items = 0;
    BlurSpan sp[4];
    CHECK(blur_build_spans(&w, &h, 1, sp, 4, &items) == -1);
    w = 64; h = 64;
    CHECK(blur_build_spans(&w, &h, 1, sp, 0, &items) == -1);   // no room for the spans
  }
  std::printf("cases %ld mismatches %ld\n", cases, bad);
  return bad != 0;
}
