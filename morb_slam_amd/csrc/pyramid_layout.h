// Storage layout of the image pyramid (d_pyr) and the byte range every reader of it can touch.  Plain C++ with no HIP in it: the
// extractor and the stereo matcher include it, and tests/native/pyramid_layout_check.cc compiles it on the host.
//
// Two borders, two constants:
//   EDGE    = 19  the ALGORITHMIC border (EDGE_THRESHOLD, ORBextractor.cc:73): minBorder / maxBorder, the size checks, the keypoint
//                 bounds, and the pad the reference's copyMakeBorder puts around mvImagePyramid[l];
//   kPyrPad = 3   the STORED border.  Of the reference's 19 reflected pixels only the innermost three are ever read (the 7-tap blur
//                 of a pixel at the image's edge); FAST, the resize, IC_Angle and the stereo SAD read interior pixels.  The other
//                 sixteen are not computed and not stored.
// A level of one image is a block of (h + 2 * kPyrPad) rows of pstride = align_up(w + 2 * kPyrPad, 64) bytes; the interior starts
// kPyrPad rows down and kPyrPad bytes into the row.  Blocks are level-major: level l's nimg blocks follow level l - 1's.
// 3 == 19 (mod 16): every alignment the kernels were tuned around is what it was with the full pad — the blur's 16-byte loads at
// (pad - 3) + x, the dword base and byte shift of the resize windows, the patch dwords of k_describe, the FAST tile's one-column
// shift.  Another pad width needs those derived again.
//
// Wide loads run past what they use: past the padded width into the row's alignment slack or — where w + 6 is a multiple of 64 —
// into the next row, the next image, the next level, and behind the last block into the kPyrTail zeroed bytes the allocation ends
// with.  The extent functions below give, per reader, the lowest and highest byte it can touch relative to the first byte of the
// (level, image) block; pyr_extents_ok() is what configure() requires and what the host test sweeps.
#pragma once
#include <cmath>

namespace morb {

constexpr int EDGE = 19;        // EDGE_THRESHOLD  ORBextractor.cc:73
constexpr int kPyrPad = 3;      // stored border of a pyramid level
constexpr int kBlurReach = 3;   // GaussianBlur 7 x 7: the only reader of border pixels
constexpr int kPyrTail = 256;   // zeroed bytes behind the last block
static_assert(kPyrPad >= kBlurReach, "the blur reads kBlurReach border pixels");
static_assert((EDGE - kPyrPad) % 16 == 0 && kPyrPad <= EDGE, "the kernels' aligned loads assume pad == 19 (mod 16)");

struct PyrLevelLayout {
  int w, h, pstride;
  unsigned long long off, img;   // bytes: offset of the level's first block, size of one image's block
};
struct PyrExtent { long long lo, hi; };   // lowest / highest byte touched, relative to the block's first byte

inline int pyr_level_dim(int n0, float invScale) { return (int)lrintf((float)n0 * invScale); }   // cvRound(n0 * mvInvScaleFactor[l]), ORBextractor.cc:1091-1092
inline int pyr_stride(int w) { return (w + 2 * kPyrPad + 63) & ~63; }
inline long long pyr_interior(int pstride) { return (long long)kPyrPad * pstride + kPyrPad; }   // block -> first interior pixel

// Fills lv[0 .. L) for a W x H image and nimg images per level; returns the bytes of all blocks (without kPyrTail).
inline unsigned long long pyr_layout(int W, int H, const float* invScale, int L, int nimg, PyrLevelLayout* lv) {
  unsigned long long off = 0;
  for (int l = 0; l < L; ++l) {
    lv[l].w = pyr_level_dim(W, invScale[l]); lv[l].h = pyr_level_dim(H, invScale[l]);
    lv[l].pstride = pyr_stride(lv[l].w);
    lv[l].off = off; lv[l].img = (unsigned long long)(lv[l].h + 2 * kPyrPad) * lv[l].pstride;
    off += lv[l].img * (unsigned)nimg;
  }
  return off;
}

// --- readers.  v = the level read (for the resizes: the SOURCE level).  Interior coordinates (x, y) sit at block byte
// (kPyrPad + y) * pstride + kPyrPad + x.
inline long long pyr_at(const PyrLevelLayout& v, int x, int y) { return (long long)(kPyrPad + y) * v.pstride + kPyrPad + x; }

// k_resize: per source row y in [0, h) and window start b in [0, w), three aligned dwords from byte (kPyrPad + b) & ~3 of the row.
// Used: interior bytes only (the tables clamp like cv::resize).
inline PyrExtent pyr_resize_extent(const PyrLevelLayout& v) {
  return {(long long)kPyrPad * v.pstride + (kPyrPad & ~3), (long long)(kPyrPad + v.h - 1) * v.pstride + ((kPyrPad + v.w - 1) & ~3) + 11};
}
// k_resize_gather: single interior bytes.
inline PyrExtent pyr_gather_extent(const PyrLevelLayout& v) { return {pyr_at(v, 0, 0), pyr_at(v, v.w - 1, v.h - 1)}; }
// k_blur: 16-byte loads at column x - 3 for x = 0, 8, ... < w, of rows -3 .. h + 2 (the row index is clamped to the last stored row).
// Used: columns -3 .. w + 2; what lies past them only feeds output columns >= w, which land in the blurred row's own slack.
inline PyrExtent pyr_blur_extent(const PyrLevelLayout& v) {
  return {pyr_at(v, -kBlurReach, -kBlurReach), pyr_at(v, 8 * ((v.w - 1) / 8) - kBlurReach + 15, v.h - 1 + kPyrPad)};
}
// k_fastw: rows of P = 48 / 64 / 80 bytes from one column left of a cell window.  Windows start at x, y >= 16 and end at
// maxBorder = dim - 16; an evaluated window is wider than 6.  Used: the window, interior only.
inline PyrExtent pyr_fast_extent(const PyrLevelLayout& v, int P) {
  const int minB = EDGE - 3, maxX = v.w - EDGE + 3, maxY = v.h - EDGE + 3;
  return {pyr_at(v, minB - 1, minB), pyr_at(v, (maxX - 7) - 1 + P - 1, maxY - 1)};
}
// k_describe: 31 rows of eight dwords from (cx - 15, cy - 15), keypoints at EDGE <= c < dim - EDGE.  Used: interior only.
inline PyrExtent pyr_describe_extent(const PyrLevelLayout& v) {
  return {pyr_at(v, EDGE - 15, EDGE - 15), pyr_at(v, v.w - EDGE - 1 - 15 + 31, v.h - EDGE - 1 + 15)};
}
// k_stereo_match: rows v - 5 .. v + 5 of a left keypoint (EDGE <= v < h - EDGE); left patch dwords cover columns uL - 5 .. uL + 6
// (EDGE <= uL < w - EDGE), the right strip's columns uR0 - 10 .. uR0 + 13 with 0 <= uR0 and uR0 + 11 < w (the reference's guard,
// Frame.cc:981-985, which lets the strip start up to ten columns left of the image).  Used: uR0 - 10 .. uR0 + 10; see
// pyr_stereo_scale_ok() for why those are stored pixels.
inline PyrExtent pyr_stereo_extent(const PyrLevelLayout& v) {
  return {pyr_at(v, -10, EDGE - 5), pyr_at(v, v.w - 12 + 13, v.h - EDGE - 1 + 5)};
}
// The right keypoint of a stereo pair comes from level l - 1, l or l + 1 and sits at x >= EDGE on its own level, so on level l its
// column uR0 is at least round(EDGE / scaleFactor) (give or take one for the float round trip), and the strip's leftmost used
// column is uR0 - 10.  That is a stored pixel while EDGE / scaleFactor >= 8: column >= 8 - 1 - 10 = -kPyrPad.
inline bool pyr_stereo_scale_ok(float scaleFactor) { return (float)EDGE / scaleFactor >= 8.0f; }

// Every reader of every level, first and last image, stays inside [0, total + kPyrTail).
inline bool pyr_extents_ok(const PyrLevelLayout* lv, int L, int nimg, unsigned long long total, int fastP, bool gather) {
  for (int l = 0; l < L; ++l) {
    const PyrLevelLayout& v = lv[l];
    if (v.pstride % 64 != 0 || v.pstride < v.w + 2 * kPyrPad) return false;
    PyrExtent e[5] = {pyr_blur_extent(v), pyr_fast_extent(v, fastP), pyr_describe_extent(v), pyr_stereo_extent(v),
                      gather ? pyr_gather_extent(v) : pyr_resize_extent(v)};
    for (int k = 0; k < (l + 1 < L ? 5 : 4); ++k) {   // (the last level is no resize's source)
      if ((long long)v.off + e[k].lo < 0) return false;
      if (v.off + v.img * (unsigned)(nimg - 1) + (unsigned long long)e[k].hi >= total + kPyrTail) return false;
    }
  }
  return true;
}

}  // namespace morb
