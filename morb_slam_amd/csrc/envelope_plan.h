// The host-side symbolic pass of the map-sized pose graphs (essential_graph.hip: 7 x 7 blocks, pose_graph_4dof.hip: 4 x 4): which vertices
// are in the system, the envelope of its block rows in the caller's vertex order, the rows covering each column, and the contributions of
// the edges to every envelope block in edge insertion order.  Nothing here depends on the width of a block.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ba_host.h"

namespace morb {

struct EnvelopePlan {
  int n = 0, nBlocks = 0;
  std::vector<int> col;         // [nKF] block row of the system, -1: fixed or without an edge
  std::vector<int> rowFirst;    // [n] first block column of row i's envelope
  std::vector<int> rowOff;      // [n + 1] envelope block of (i, rowFirst[i])
  std::vector<int> colStart;    // [n + 1] the rows below j whose envelope covers column j: colRows[colStart[j] .. colStart[j + 1]), ascending
  std::vector<int> colRows;
  std::vector<int> listStart;   // [nBlocks + 1] contributions of envelope block k, in edge order
  std::vector<int> listItems;   // edge * 4 + kind: 0 / 1 diagonal block of vertex 0 / 1, 2 / 3 off-diagonal block whose row is vertex 0 / 1
};

enum class EnvelopeFit { Ok, Empty, TooLarge };

// fixedBit0[v] & 1: the vertex is fixed.  Empty: no free vertex has an edge (only P.col and P.n are set).  TooLarge: more than maxBlocks
// envelope blocks (P.col, P.n and P.rowFirst are set).
inline EnvelopeFit plan_envelope(int nKF, const uint8_t* fixedBit0, int nE, const int* eI, const int* eJ, size_t maxBlocks, EnvelopePlan& P) {
  // ---- the system: free vertices with an edge, in the caller's order; the envelope of its block rows ----
  P.col.assign(nKF, -1);
  {
    std::vector<char> used(nKF, 0);
    for (int e = 0; e < nE; ++e) used[eI[e]] = used[eJ[e]] = 1;
    int n = 0;
    for (int v = 0; v < nKF; ++v) if (!(fixedBit0[v] & 1) && used[v]) P.col[v] = n++;
    P.n = n;
  }
  const int n = P.n;
  const std::vector<int>& col = P.col;
  if (!n) return EnvelopeFit::Empty;
  std::vector<int>&rowFirst = P.rowFirst, &rowOff = P.rowOff;
  rowFirst.resize(n); rowOff.assign(n + 1, 0);
  for (int r = 0; r < n; ++r) rowFirst[r] = r;
  for (int e = 0; e < nE; ++e) {
    const int a = col[eI[e]], b = col[eJ[e]];
    if (a >= 0 && b >= 0) rowFirst[std::max(a, b)] = std::min(rowFirst[std::max(a, b)], std::min(a, b));
  }
  size_t total = 0;
  for (int r = 0; r < n; ++r) total += (size_t)(r - rowFirst[r] + 1);
  if (total > maxBlocks) return EnvelopeFit::TooLarge;
  for (int r = 0; r < n; ++r) rowOff[r + 1] = rowOff[r] + (r - rowFirst[r] + 1);
  const int nBlocks = P.nBlocks = rowOff[n];
  std::vector<int>&colStart = P.colStart, &colRows = P.colRows;
  colStart.assign(n + 1, 0); colRows.assign((size_t)std::max(nBlocks - n, 1), 0);
  for (int i = 0; i < n; ++i) for (int j = rowFirst[i]; j < i; ++j) ++colStart[j + 1];
  for (int j = 0; j < n; ++j) colStart[j + 1] += colStart[j];
  {
    std::vector<int> fill(colStart.begin(), colStart.end() - 1);
    for (int i = 0; i < n; ++i) for (int j = rowFirst[i]; j < i; ++j) colRows[fill[j]++] = i;
  }
  // contributions to the envelope blocks, in edge order
  std::vector<int> cKey, cItem;
  cKey.reserve((size_t)3 * nE); cItem.reserve((size_t)3 * nE);
  for (int e = 0; e < nE; ++e) {
    const int a = col[eI[e]], b = col[eJ[e]];
    if (a >= 0) { cKey.push_back(rowOff[a + 1] - 1); cItem.push_back(e * 4 + 0); }
    if (b >= 0) { cKey.push_back(rowOff[b + 1] - 1); cItem.push_back(e * 4 + 1); }
    if (a >= 0 && b >= 0) {
      if (a > b) { cKey.push_back(rowOff[a] + (b - rowFirst[a])); cItem.push_back(e * 4 + 2); }
      else { cKey.push_back(rowOff[b] + (a - rowFirst[b])); cItem.push_back(e * 4 + 3); }
    }
  }
  std::vector<int> listPos;
  csr_by_key(cKey.data(), (int)cKey.size(), nBlocks, P.listStart, listPos);
  P.listItems.resize(listPos.size());
  for (size_t q = 0; q < listPos.size(); ++q) P.listItems[q] = cItem[listPos[q]];
  return EnvelopeFit::Ok;
}

}  // namespace morb
