// Test-only probe, the optimizer_device.h family (with quat_huber.h, wave.h and ransac_block.h): the SE3Quat algebra, Eigen's
// matrix -> quaternion in its constant-index form, glibc's small-argument sin, cube_rn, Huber's kernel; the DPP reductions of wave.h on
// whole waves; the count and the ordered compaction of ransac_block.h on whole workgroups.  Part of tests/native/libmath_probe.so.
#include "math_probe_common.h"

#include "optimizer_device.h"
#include "ransac_block.h"

// SE3 records: q (x y z w), t
namespace {
__device__ __forceinline__ SE3 ld_se3(const double* a) { SE3 s; for (int k = 0; k < 4; ++k) s.q[k] = a[k]; for (int k = 0; k < 3; ++k) s.t[k] = a[4 + k]; return s; }
__device__ __forceinline__ void st_se3(const SE3& s, double* o) { for (int k = 0; k < 4; ++k) o[k] = s.q[k]; for (int k = 0; k < 3; ++k) o[4 + k] = s.t[k]; }
}  // namespace

PROBE(q_rotate_d, double, 7, double, 3, q_rotate<double>(a, a + 4, o);)
PROBE(q_rotate_f, float, 7, float, 3, q_rotate<float>(a, a + 4, o);)
PROBE(q_to_R, double, 4, double, 9, q_to_R(a, o);)
PROBE(R_to_q_se3, double, 9, double, 4, R_to_q(a, o);)
PROBE(se3_normalize, double, 7, double, 7, SE3 s = ld_se3(a); se3_normalize(s); st_se3(s, o);)
PROBE(se3_mul, double, 14, double, 7, st_se3(se3_mul(ld_se3(a), ld_se3(a + 7)), o);)
PROBE(se3_map, double, 10, double, 3, se3_map(ld_se3(a), a + 7, o);)
PROBE(se3_from_float, float, 7, double, 7, st_se3(se3_from_float(a), o);)
PROBE(se3_exp, double, 6, double, 7, st_se3(se3_exp(a), o);)
PROBE(cube_rn, double, 1, double, 1, o[0] = cube_rn(a[0]);)
PROBE(huber, double, 2, double, 2, o[0] = huber(a[0], a[1], &o[1]);)   // (delta, e) -> (rho, w)
PROBE(sin_small, double, 1, double, 1, o[0] = sin_glibc_small(a[0]);)

// ---- wave.h: every lane of every wave active (n a multiple of the block size, one value per thread in, one out) -------------------------
namespace {
enum { W_MIN_U32, W_SUM_I32, W_MIN_U64, W_SUM_F64, W_ROW_SUM_F64, W_READLANE_F64 };
template <int SRC>
__device__ __forceinline__ double rl(double v) { return morbwave::readlane_f64(v, SRC); }
template <int OP>
__global__ void k_probe_wave(const void* in, void* out, int src) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (OP == W_MIN_U32) static_cast<uint32_t*>(out)[i] = morbwave::min_u32(static_cast<const uint32_t*>(in)[i]);
  if (OP == W_SUM_I32) static_cast<int*>(out)[i] = morbwave::sum_i32(static_cast<const int*>(in)[i]);
  if (OP == W_MIN_U64) static_cast<unsigned long long*>(out)[i] = morbwave::min_u64(static_cast<const unsigned long long*>(in)[i]);
  if (OP == W_SUM_F64) static_cast<double*>(out)[i] = morbwave::sum_f64(static_cast<const double*>(in)[i]);
  if (OP == W_ROW_SUM_F64) static_cast<double*>(out)[i] = morbwave::row_sum_f64(static_cast<const double*>(in)[i]);
  if (OP == W_READLANE_F64) {   // src is the same in every lane; the six constants the product's call sites are built like
    const double v = static_cast<const double*>(in)[i];
    double r;
    switch (src) {
      case 0: r = rl<0>(v); break;
      case 15: r = rl<15>(v); break;
      case 16: r = rl<16>(v); break;
      case 31: r = rl<31>(v); break;
      case 32: r = rl<32>(v); break;
      default: r = rl<63>(v); break;
    }
    static_cast<double*>(out)[i] = r;
  }
}
template <int OP>
int launch_wave(const void* in, void* out, int blocks, int threads, int src) {
  hipLaunchKernelGGL(k_probe_wave<OP>, dim3(blocks), dim3(threads), 0, 0, in, out, src);
  return probe_finish();
}
}  // namespace

// op: 0 min_u32, 1 sum_i32, 2 min_u64, 3 sum_f64, 4 row_sum_f64, 5 readlane_f64(src).  in / out: blocks * threads values; threads: 64 or 256.
extern "C" int probe_wave(int op, const void* in, void* out, int blocks, int threads, int src) {
  if (!in || !out) return PROBE_ERR_ARG;
  if (blocks < 1 || blocks > 4096 || (threads != 64 && threads != 256)) return PROBE_ERR_SIZE;
  if (op == W_READLANE_F64 && src != 0 && src != 15 && src != 16 && src != 31 && src != 32 && src != 63) return PROBE_ERR_SIZE;
  switch (op) {
    case W_MIN_U32: return launch_wave<W_MIN_U32>(in, out, blocks, threads, src);
    case W_SUM_I32: return launch_wave<W_SUM_I32>(in, out, blocks, threads, src);
    case W_MIN_U64: return launch_wave<W_MIN_U64>(in, out, blocks, threads, src);
    case W_SUM_F64: return launch_wave<W_SUM_F64>(in, out, blocks, threads, src);
    case W_ROW_SUM_F64: return launch_wave<W_ROW_SUM_F64>(in, out, blocks, threads, src);
    case W_READLANE_F64: return launch_wave<W_READLANE_F64>(in, out, blocks, threads, src);
  }
  return PROBE_ERR_SIZE;
}

// ---- ransac_block.h: one workgroup of NT threads per problem, as the three solver kernels run it ---------------------------------------
namespace {
// flags [n] (0 / 1) -> count[0] = block_count, count[1] = the running total of the compaction, kept [n]: the kept entries in order
template <int NT>
__global__ __launch_bounds__(NT) void k_probe_ransac(const int* __restrict__ flags, int n, int* __restrict__ count, int* __restrict__ kept) {
  constexpr int NW = NT / 64;
  __shared__ int total, running, wcount[NW];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) { total = 0; running = 0; }
  __syncthreads();
  morbransac::block_count<NT>(n, &total, [=](int i) { return flags[i] != 0; });
  for (int base = 0; base < n; base += NT) {
    const int i = base + t;
    const bool valid = i < n && flags[i] != 0;
    const int c = morbransac::ordered_slot(valid, lane, wv, wcount, &running);
    if (valid && c >= 0 && c < n) kept[c] = i;
    morbransac::ordered_commit<NW>(wcount, &running);
  }
  if (t == 0) { count[0] = total; count[1] = running; }
}
}  // namespace

extern "C" int probe_ransac_block(int nt, const int* flags, int n, int* count, int* kept) {
  if (!flags || !count || !kept) return PROBE_ERR_ARG;
  if (n < 0 || n > (1 << 20) || (nt != 64 && nt != 128 && nt != 256)) return PROBE_ERR_SIZE;
  if (nt == 64) hipLaunchKernelGGL(k_probe_ransac<64>, dim3(1), dim3(64), 0, 0, flags, n, count, kept);
  else if (nt == 128) hipLaunchKernelGGL(k_probe_ransac<128>, dim3(1), dim3(128), 0, 0, flags, n, count, kept);
  else hipLaunchKernelGGL(k_probe_ransac<256>, dim3(1), dim3(256), 0, 0, flags, n, count, kept);
  return probe_finish();
}
