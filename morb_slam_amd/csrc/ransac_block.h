// Workgroup scaffolding the batched RANSAC solvers share (sim3_solver.hip, mlpnp_solver.hip, two_view.hip; one workgroup of whole
// waves per problem): the count of the kept entries, their compaction in entry order, the 4 x 4 identity of a record.
#pragma once
#include <hip/hip_runtime.h>

namespace morbransac {

// adds to *total (LDS, zeroed behind a barrier) how many i of [0, n) satisfy pred(i); ends in a barrier, so every thread may read it
template <int NT, class Pred>
__device__ __forceinline__ void block_count(int n, int* total, Pred pred) {
  const int t = threadIdx.x;
  int cnt = 0;
  for (int base = 0; base < n; base += NT) {
    const int i = base + t;
    cnt += __popcll(__ballot(i < n && pred(i)));
  }
  if ((t & 63) == 0) atomicAdd(total, cnt);
  __syncthreads();
}

// Compaction in entry order, one entry per thread and pass, as a pair around the caller's own store (every thread calls both):
//   for (base = 0; base < n; base += NT) { valid = ..; c = ordered_slot(valid, lane, wv, wcount, &running); if (valid) <store at c>;
//                                          ordered_commit<NW>(wcount, &running); }
// lane, wv: the thread's lane and wave (threadIdx.x & 63, >> 6), wcount: one int per wave, running: the entries kept by the passes
// before (both LDS).  ordered_slot returns the slot of a valid entry: running, plus the valid entries of the waves below (wave
// ballots), plus those of the lanes below.
__device__ __forceinline__ int ordered_slot(bool valid, int lane, int wv, int* wcount, const int* running) {
  const unsigned long long bal = __ballot(valid);
  const int below = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wcount[wv] = __popcll(bal);
  __syncthreads();
  int off = *running;
  for (int k = 0; k < wv; ++k) off += wcount[k];
  return off + below;
}
template <int NW>
__device__ __forceinline__ void ordered_commit(const int* wcount, int* running) {
  __syncthreads();
  if (threadIdx.x == 0) { int tot = 0; for (int k = 0; k < NW; ++k) tot += wcount[k]; *running += tot; }
  __syncthreads();
}

// cv::Mat::eye(4, 4, CV_32F) / Matrix4f::Identity(), row-major
__device__ __forceinline__ void identity16(float* T) {
  for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
}

}  // namespace morbransac
