// Work items of k_blur and how an item number becomes (level, column strip, strip row).  Plain C++ with no HIP in it: the
// extractor includes it for configure() and for the kernel's one division, tests/native/blur_items_check.cc compiles it on the host.
//
// An item is a strip of BT_PX columns x BT_ROWS rows of one level, worked by one lane.  The items of an image are numbered across all
// its levels, level 0 first: along a strip row (consecutive lanes take horizontally adjacent strips, so a wave's 16-byte loads and
// 8-byte stores stay contiguous), then down to the next strip row, then on to the next level.  Every lane of every wave of an image
// has an item except in the image's last wave.
//
// The numbering is cut into spans: a run of whole strip rows of one level with at most kBlurSpanItems items.  Inside a span
// j / nsx == (j * magic) >> shift with both factors below 2^24 and the product below 2^32 (one v_mul_u32_u24, full rate; the
// compiler's own division by a run-time value is a chain of quarter-rate multiplies):
//   shift = the smallest s with 2^s >= J * nsx (J = the span's items), magic = floor(2^s / nsx) + 1, so magic * nsx - 2^s <= nsx and
//   j * (magic * nsx - 2^s) < 2^s for every j < J: the quotient is exact;  2^s < 2 * J * nsx gives magic <= 2 * J and
//   j * magic < 2 * J^2 <= 2^31 for J <= 32768.
// A 752 x 480 image has one span per level; a level needs a second span from 32768 strips (a 4095 x 4095 level has 87552).
#pragma once

namespace morb {

constexpr int BT_PX = 8;      // columns per strip: one 16-byte load and one 8-byte store per row
constexpr int BT_ROWS = 24;   // rows per strip: fewer halo rows against more dead rows below a level (16 / 24 / 32 rows: 298 / 295 / 294 us per 512 images alone on the chip, profiles/r11)
constexpr int kBlurSpanItems = 32768;
constexpr int kBlurWave = 64;

struct BlurSpan {
  int level, sy0, nsy, nsx;   // strip rows sy0 .. sy0 + nsy of the level, nsx strips each
  int itemBase;               // number of the span's first item within the image
  unsigned magic, shift;
};
struct BlurItem { int level, x, y0; };   // top-left pixel of the strip

inline int blur_strips_x(int w) { return (w + BT_PX - 1) / BT_PX; }
inline int blur_strips_y(int h) { return (h + BT_ROWS - 1) / BT_ROWS; }

// j / nsx for an item j of a span (the kernel's form: the low 32 bits of a 24 x 24-bit product)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned blur_div(unsigned j, unsigned magic, unsigned shift) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(j, magic) >> shift;
#else
  return (unsigned)(((unsigned long long)(j & 0xFFFFFFu) * (magic & 0xFFFFFFu)) & 0xFFFFFFFFull) >> shift;
#endif
}

// Spans of the levels w[l] x h[l], l < L, into out[0 .. cap).  Returns the number of spans, or -1 when they do not fit cap or a level
// is too wide for the division (more than kBlurSpanItems strips in a row).  *items receives the items of one image.
inline int blur_build_spans(const int* w, const int* h, int L, BlurSpan* out, int cap, int* items) {
  int n = 0, base = 0;
  for (int l = 0; l < L; ++l) {
    const int nsx = blur_strips_x(w[l]), nsy = blur_strips_y(h[l]);
    if (nsx < 1 || nsy < 1 || nsx > kBlurSpanItems) return -1;
    const int rowsPerSpan = kBlurSpanItems / nsx;
    for (int sy0 = 0; sy0 < nsy; sy0 += rowsPerSpan) {
      if (n >= cap) return -1;
      BlurSpan& s = out[n++];
      s.level = l; s.sy0 = sy0; s.nsy = nsy - sy0 < rowsPerSpan ? nsy - sy0 : rowsPerSpan; s.nsx = nsx;
      s.itemBase = base; base += s.nsx * s.nsy;
      const unsigned long long need = (unsigned long long)(s.nsx * s.nsy) * (unsigned)nsx;
      s.shift = 0;
      while ((1ull << s.shift) < need) ++s.shift;
      s.magic = (unsigned)((1ull << s.shift) / (unsigned)nsx) + 1u;
    }
  }
  *items = base;
  return n;
}

inline int blur_waves(int items) { return (items + kBlurWave - 1) / kBlurWave; }

// Item -> strip, the way the kernel does it: the span is the last one whose itemBase is <= item.
inline BlurItem blur_locate(const BlurSpan* sp, int n, int item) {
  int s = 0;
  for (int k = 1; k < n; ++k) s += item >= sp[k].itemBase;
  const unsigned j = (unsigned)(item - sp[s].itemBase);
  const unsigned sy = blur_div(j, sp[s].magic, sp[s].shift);
  return {sp[s].level, (int)(j - sy * (unsigned)sp[s].nsx) * BT_PX, (sp[s].sy0 + (int)sy) * BT_ROWS};
}

}  // namespace morb
