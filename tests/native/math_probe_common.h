// Shared scaffolding of the math probe (tests/native/math_probe_*.hip -> tests/native/libmath_probe.so): one record in, one record out.
// PROBE(name, TI, NI, TO, NO, body) defines a device function of (const TI* a, TO* o), a kernel in which thread i reads input record i
// (NI values of TI), calls it and writes output record i (NO values of TO), and the entry point
//     int probe_<name>(const void* in, void* out, long long n);
// PROBE_HD does the same for code that also compiles for the host and adds
//     int host_<name>(const void* in, void* out, long long n);    // the same body over host arrays, at most 16 threads, no GPU
// Conventions of dense_probe.hip: every buffer is the caller's, launches go on the null stream and are waited for, the return value is
// 0, a HIP error code, or a negative refusal before any launch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <thread>
#include <vector>

namespace {

constexpr int PROBE_ERR_SIZE = -1;   // n (or a size argument) out of range
constexpr int PROBE_ERR_ARG = -3;    // a null buffer
constexpr long long PROBE_MAX_RECORDS = 1ll << 28;

inline int probe_finish() {   // the launch's own error first, then whatever the kernel ran into
  hipError_t e = hipGetLastError();
  const hipError_t s = hipDeviceSynchronize();
  if (e == hipSuccess) e = s;
  return (int)e;
}

template <class F>
__global__ __launch_bounds__(256) void k_probe_map(const typename F::in_t* __restrict__ in, typename F::out_t* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  typename F::in_t a[F::ni];
  typename F::out_t o[F::no];
  for (int k = 0; k < F::ni; ++k) a[k] = in[i * F::ni + k];
  for (int k = 0; k < F::no; ++k) o[k] = (typename F::out_t)0;
  F::run(a, o);
  for (int k = 0; k < F::no; ++k) out[i * F::no + k] = o[k];
}

template <class F>
int probe_launch_map(const void* in, void* out, long long n) {
  if (!in || !out) return PROBE_ERR_ARG;
  if (n < 1 || n > PROBE_MAX_RECORDS) return PROBE_ERR_SIZE;
  hipLaunchKernelGGL(k_probe_map<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, static_cast<const typename F::in_t*>(in),
                     static_cast<typename F::out_t*>(out), n);
  return probe_finish();
}

template <class F>
int probe_host_map(const void* in_, void* out_, long long n) {
  if (!in_ || !out_) return PROBE_ERR_ARG;
  if (n < 1 || n > PROBE_MAX_RECORDS) return PROBE_ERR_SIZE;
  const auto* in = static_cast<const typename F::in_t*>(in_);
  auto* out = static_cast<typename F::out_t*>(out_);
  const int nt = (int)std::min<long long>(16, (n + 65535) / 65536);
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([=] {
      for (long long i = n * t / nt; i < n * (t + 1) / nt; ++i) {
        typename F::out_t o[F::no];
        for (int k = 0; k < F::no; ++k) o[k] = (typename F::out_t)0;
        F::run(in + i * F::ni, o);
        for (int k = 0; k < F::no; ++k) out[i * F::no + k] = o[k];
      }
    });
  for (auto& x : th) x.join();
  return 0;
}

}  // namespace

#define PROBE_STRUCT(name, QUAL, TI, NI, TO, NO, ...)                  \
  namespace {                                                          \
  struct F_##name {                                                    \
    typedef TI in_t;                                                   \
    typedef TO out_t;                                                  \
    enum { ni = NI, no = NO };                                         \
    static QUAL void run(const TI* a, TO* o) { __VA_ARGS__ }           \
  };                                                                   \
  }
#define PROBE(name, TI, NI, TO, NO, ...)                               \
  PROBE_STRUCT(name, __device__ __forceinline__, TI, NI, TO, NO, __VA_ARGS__) \
  extern "C" int probe_##name(const void* in, void* out, long long n) { return probe_launch_map<F_##name>(in, out, n); }
#define PROBE_HD(name, TI, NI, TO, NO, ...)                            \
  PROBE_STRUCT(name, __host__ __device__ inline, TI, NI, TO, NO, __VA_ARGS__) \
  extern "C" int probe_##name(const void* in, void* out, long long n) { return probe_launch_map<F_##name>(in, out, n); } \
  extern "C" int host_##name(const void* in, void* out, long long n) { return probe_host_map<F_##name>(in, out, n); }
