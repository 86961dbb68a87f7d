// Internal layout of the extractor handle and its per-level geometry, shared by the translation units of
// libmorb_hip.so (the stereo matcher reads the pyramids the extractor owns, like Frame::ComputeStereoMatches
// reads mpORBextractorLeft->mvImagePyramid, Frame.cc:895).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "hip_owned.h"
#include "morb_hip.h"
#include "blur_items.h"       // k_blur's work items: BT_ROWS, the spans of the item numbering
#include "pyramid_layout.h"   // EDGE (the algorithmic border), kPyrPad (the stored one), the layout of d_pyr

namespace morb {
constexpr int kMaxLevels = 16;
constexpr int HALF_PATCH = 15;  // HALF_PATCH_SIZE :72
constexpr int PATCH = 31;       // PATCH_SIZE :71
constexpr int MINB = 16;        // minBorderX/Y = EDGE_THRESHOLD - 3 (:746-747)
constexpr int kLdsKeys = 3072;  // distribute: the LDS key arrays hold at least this many candidates per level (more for larger images, see configure())

struct LevelGeom {
  int w, h;
  int pstride, bstride;
  unsigned long long pyrOff, pyrImg;    // bytes: slab offset, per-image size
  unsigned long long blurOff, blurImg;
  int nCols, nRows, wCell, hCell, cellBase;
  int maxBorderX, maxBorderY;
  int quota, nIni;
  int nodeCap, listCap;
  int selBase, selCap;                  // per-image offsets into sel[]
  unsigned long long qtOff, qtImg;      // element offsets into the global key scratch
  int xtabOff, ytabOff;                 // offsets (entries) into the resize tables
  float scale;                          // mvScaleFactor[l]
  float kpSize;                         // (float)(int)(PATCH_SIZE * mvScaleFactor[l])  (:831)
  // k_distribute packs several levels of an image into one workgroup, a wave per level: the workgroup (group) and wave of this
  // level, the byte offset of its LDS region inside the workgroup's allocation, and the candidate keys its LDS arrays hold
  int distGroup, distWave, distLdsOff, distKeyCap;
  int distTeam;                         // all waves of the workgroup work this level as a team (quadtree.h: Team)
};

// k_blur: one entry per span of the item numbering (blur_items.h) with what a lane needs of the span's level.  A wave can straddle
// spans and levels, so the lanes read their entry with vector loads (five 16-byte words).
struct alignas(16) BlurSeg {
  int itemBase, nsx; unsigned magic, shift;
  int y0, w, h, pstride;                // y0: first row of the span
  int bstride; unsigned pyrImg, blurImg; int pad_;   // per-image sizes in bytes (a level of one image is far below 4 GB)
  unsigned long long pyrOff, blurOff;
};

// What k_fastw needs of every level, passed by value: the kernarg segment is read with scalar loads, so looking a
// cell's level up costs no dependent global-memory round trip.
struct FastGeom {
  int cellBase[kMaxLevels], nCols[kMaxLevels], wCell[kMaxLevels], hCell[kMaxLevels];
  int pstride[kMaxLevels], maxBorderX[kMaxLevels], maxBorderY[kMaxLevels];
  unsigned long long pyrOff[kMaxLevels], pyrImg[kMaxLevels];
  unsigned wCellMagic[kMaxLevels];      // ceil(2^16 / wCell): x / wCell == (x * magic) >> 16 for every x < 128
};

// k_fastw works cell by cell.  One descriptor per FAST cell of an image (all levels), built on the host, read with one scalar load
// (the "segment" of round 2's kernel, which ran up to three cells per workgroup; the cell count field stays at 1).
struct FastSeg {
  unsigned winOff;   // byte offset of the window's top-left pixel inside the level's stored block (pyramid_layout.h)
  int cell0;         // flat index of the segment's first cell within the image (cellBase + ci * nCols + c0)
  int geo;           // level | cells << 8 | window width << 16 | window height << 24 (width 0: nothing to evaluate)
  int key0;          // added to window coordinates to form candidate keys: c0 * wCell | (ci * hCell) << 16
};

// What k_describe needs of every level, by value (see FastGeom).
struct DescGeom {
  unsigned long long pyrOff[kMaxLevels], pyrImg[kMaxLevels], blurOff[kMaxLevels], blurImg[kMaxLevels];
  int pstride[kMaxLevels], bstride[kMaxLevels];
  float scale[kMaxLevels], kpSize[kMaxLevels];
};

struct alignas(8) ResizeTab {  // one entry per stored destination column / row (interior + kPyrPad on either side) (8-byte aligned: scalar loads need dword alignment)
  short s0, s1, c0, c1;  // source index (clipped), source index + 1 (clipped), fixed-point weights (2048 = 1)
};

// k_resize / k_level01 work on linearly numbered items (extractor.hip): per destination dword of a level (PyrCol), per destination
// row (PyrRow), per pad dword of level 0 (PyrEdge)
struct alignas(16) PyrCol {   // 48 bytes: three 16-byte loads
  int base;            // the chunk's 8-byte source window starts at byte base + sh of the source's padded row; base is a multiple of 4
  uint32_t sel[4];     // v_perm_b32 selector of pixel k: left source byte -> byte 0, right source byte -> byte 2, bytes 1 and 3 zero
  uint32_t coef[4];    // c0 | c1 << 16 (2048 = 1)
  int sh, pad_[2];
};
struct alignas(16) PyrRow { int s0, s1; uint32_t c0s, c1s; };   // source rows (clipped), vertical weights << 12
struct alignas(16) PyrEdge { int dword, base; uint32_t sel; int pad_; };   // destination dword, source byte offset of its 4-byte window, byte selector
struct PyrLevel { int nC, nG, nItems, colOff, rowOff, ldsRows; uint32_t magicC; };
struct PyrLevel0 { int nInt, j0, nEdge, nG, nIntItems, nItems; uint32_t magicInt, magicEdge; };

}  // namespace morb

struct morb_extractor {
  morb::FastGeom fastGeom = {};
  morb::DescGeom descGeom = {};
  morb::DeviceArray<int2> d_kref;   // per selected keypoint: output slot | level << 24 (or -1), packed key (k_layout -> k_describe)
  int nfeatures = 0, nlevels = 0, iniTh = 0, minTh = 0, device = 0;
  float scaleFactor = 1.2f;
  std::vector<float> scale, invScale, sigma2, invSigma2;
  std::vector<int> quota;
  int umax[16];

  int W = 0, H = 0, nimgCap = 0, nimgLast = 0;
  morb::LevelGeom geom[morb::kMaxLevels];
  int totalCells = 0, cellCap = 0, maxCells = 0, maxNodeCap = 0, maxListCap = 0;
  int fastSegs[2] = {0, 0}, fastRows[2] = {0, 0};   // k_fastw launch groups (cells, LDS window rows)
  int fastP = 128;                                  // k_fastw: LDS pitch of the segment windows
  int selPerImg = 0, blurItems = 0, blurSegs = 0, outCap = 0;   // blurItems: k_blur's items per image, blurSegs: entries of d_blurSeg
  size_t pyrBytes = 0, blurBytes = 0, qtElems = 0, distSmem = 0, fastSmem[2] = {0, 0};
  int distKeyCap = 0;                        // candidate keys of level 0 that fit the quadtree's LDS arrays (smaller levels: scaled by area)
  int distGroups = 0, distWaves = 1;         // k_distribute grid: workgroups per image, waves per workgroup
  // the same for calls with few images (latency): the big levels are worked by a team of QT_MAX_WAVES waves each
  int distGroupsTeam = 0; size_t distSmemTeam = 0;
  morb::DeviceArray<morb::LevelGeom> d_geomTeam;

  morb::Stream stream;
  morb::Stream sideStream;                   // the blur runs here, underneath the quadtree (fork after FAST, join before describe)
  morb::Event evFork, evJoin;
  morb::Event evPyr;               // recorded on the launch stream behind the last pyramid launch (morb_extractor_event_after_pyramid)
  bool wantPyrEvent = false;       // ... once a caller has asked for it
  // device tables and buffers of the configured size (configure() replaces them)
  morb::DeviceArray<morb::LevelGeom> d_geom;
  morb::DeviceArray<morb::ResizeTab> d_tabs;
  morb::DeviceArray<morb::PyrCol> d_pcol; morb::DeviceArray<morb::PyrRow> d_prow; morb::DeviceArray<morb::PyrEdge> d_pedge;
  morb::PyrLevel pyrLv[morb::kMaxLevels] = {}; morb::PyrLevel0 pyrL0 = {};
  bool pyrPacked = true;   // every level's four-pixel chunks fit k_resize's 8-byte source windows (scale factors up to ~1.75)
  morb::DeviceArray<morb::FastSeg> d_segTab;
  morb::DeviceArray<morb::BlurSeg> d_blurSeg;
  morb::DeviceArray<uint8_t> d_pyr, d_blur;
  morb::DeviceArray<uint32_t> d_cand, d_qt, d_sel;
  morb::DeviceArray<int> d_candCnt, d_selCnt, d_lap;
  morb::PinnedArray<int> status;   // pinned, device-mapped flags the kernels can raise (bit 0: a level with > 65535 FAST candidates)
  // staging for the single-image host API (grow-only)
  morb::DeviceGrow img1;    // morb_extract's image
  morb::DeviceGrow out1;    // morb_extract's result block: count | monoIndex | pad to 16 | keypoints | descriptors
  morb::PinnedGrow io1;     // pinned host staging of morb_extract: the image on the way in, the result block on the way out
  std::vector<int> lapLast;  // host mirror of d_lap
  // profiling: a ring of event sets, one per morb_extract_batch call, read back (and averaged) on demand so the
  // timed region never synchronises with the host
  bool profiling = false;
  static constexpr int kProfRing = 64;
  std::vector<morb::Event> ev;  // [kProfRing][8]
  int profCalls = 0;
  float stageMs[7] = {0};
};

