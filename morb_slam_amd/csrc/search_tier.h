// Which implementation a window search of projection.hip takes: the one rule that window_search() and best_per_query() apply, in
// plain C++ that compiles for the host (tests/native/search_tier_check.cc pins it against the Python mirror tests/search_tiers.py).
//   tier 1: k_search<MODE, true>   one workgroup per frame, the frame's grid, candidates and descriptors in LDS;
//   tier 2: k_search<MODE, false>  the same, descriptors read from global memory through featOf[p] (they do not fit LDS);
//   tier 3: k_candidates + k_resolve<MODE> / k_best_per_query, the serial replay: neither form fits LDS, a size passes 65535
//           (the 16-bit feature / position fields), the search has no k_search form, or MORB_SERIAL_RESOLVE is set.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MORB_SEARCH_TIER_FN __host__ __device__ inline
#else
#define MORB_SEARCH_TIER_FN inline
#endif

namespace morbst {

constexpr int SEARCH_GRID_CELLS = 64 * 48;             // Frame's FRAME_GRID_COLS x FRAME_GRID_ROWS
constexpr size_t SEARCH_LDS_LIMIT = 150 * 1024;        // dynamic LDS k_search may ask for (160 KB per CU on gfx950)
constexpr int SEARCH_MAX_ITEMS = 65535;

// k_search's dynamic LDS (the SearchLds carve) for a frame capacity cap and qCap queries per frame
MORB_SEARCH_TIER_FN size_t search_lds_bytes(int cap, int qCap, bool withDesc) {
  const size_t capR = (size_t)(cap + 3) & ~(size_t)3, qCapR = (size_t)(qCap + 3) & ~(size_t)3;
  return 4 * ((size_t)SEARCH_GRID_CELLS + 4) + 4 * (size_t)SEARCH_GRID_CELLS + 4 * capR + 4 * qCapR + 16 * capR + (withDesc ? 32 * capR : 0) +
         2 * capR * 3 + 4 * qCapR + 4 * (qCapR + 4) + 4 * qCapR + capR + 4 * capR;
}

// serialOnly: the search has no k_search form (the fisheye, ranged and initialisation searches) or MORB_SERIAL_RESOLVE is set
MORB_SEARCH_TIER_FN int search_tier(int cap, int qCap, bool serialOnly) {
  if (serialOnly || cap > SEARCH_MAX_ITEMS || qCap > SEARCH_MAX_ITEMS || search_lds_bytes(cap, qCap, false) > SEARCH_LDS_LIMIT) return 3;
  return search_lds_bytes(cap, qCap, true) <= SEARCH_LDS_LIMIT ? 1 : 2;
}

}  // namespace morbst
