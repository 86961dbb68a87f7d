// Host <-> device staging of the C++ adapters (ORBmatcher.h, Optimizer.h, Sim3Solver.h): the entry points of morb_hip.h take DEVICE
// pointers (their natural callers keep frames resident in HBM); an adapter that is handed the reference's host-side containers stages
// them per call through one CallStaging.  Plain HIP runtime C API — compiles with g++ (-I/opt/rocm/include, -lamdhip64).
// This is the only header of include/morb/ that allocates or frees HIP memory (tests/test_hip_resources_cpu.py).
#pragma once
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace morb_adapter {

inline void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// A grow-only block that one adapter call carves by bumping an offset: pinned host memory (uploads pass through it: queued without a wait,
// the caller's temporary may die at once) or device memory (every device array of the call).  A block that is too small is replaced by one
// that holds the whole call; queued copies and pointers already handed out may still name the outgrown one, so it is retired and freed when
// the next call opens (the previous CallStaging has drained the stream by then).  Only growth pays for hipMalloc / hipFree (a device-wide wait).
struct Slab {
  static constexpr size_t kAlign = 256;   // what hipMalloc guarantees, and so what the kernels have been given so far
  bool pinned = false;
  char* base = nullptr;
  size_t cap = 0, off = 0, used = 0;      // used: carved since reset(), over every block
  std::vector<char*> retired;
  void* take(size_t n) {
    n = (std::max<size_t>(n, 1) + kAlign - 1) & ~(kAlign - 1);   // (0 bytes still carves: the C entry points reject NULL)
    if (off + n > cap) {
      size_t want = cap ? cap * 2 : (size_t)1 << 20;
      while (want < used + n) want *= 2;
      char* fresh = nullptr;
      if (pinned) hip_check(hipHostMalloc(reinterpret_cast<void**>(&fresh), want, hipHostMallocDefault), "hipHostMalloc");
      else hip_check(hipMalloc(reinterpret_cast<void**>(&fresh), want), "hipMalloc");
      if (base) retired.push_back(base);
      base = fresh; cap = want; off = 0;
    }
    off += n; used += n;
    return base + off - n;
  }
  void reset() {   // only while nothing queued from or on the blocks can be in flight
    for (char* r : retired) (void)(pinned ? hipHostFree(r) : hipFree(r));
    retired.clear();
    off = used = 0;
  }
};

// The staging of the calling thread, one pair of slabs per device.  Never freed: thread-exit and static destructors may run after the
// HIP runtime has gone, so both slabs are left to process exit — pinned and device memory alike.
struct ThreadStaging { Slab pinned, device; ThreadStaging() { pinned.pinned = true; } };
constexpr int kMaxDevices = 16;
inline ThreadStaging& thread_staging(int device) {
  if (device < 0 || device >= kMaxDevices) throw std::runtime_error("bad device");
  static thread_local ThreadStaging* per_device = new ThreadStaging[kMaxDevices];
  return per_device[device];
}

// One adapter call: hipSetDevice, the stream everything of the call is queued on (the handle's own, never the null stream, where a copy
// would wait for every blocking stream of the device, i.e. for the LocalBundleAdjustment trial the mapping thread has in flight: System.cc:209
// runs Tracking and LocalMapping side by side), and the thread's slabs for that device, reset.  Calls do not nest: one CallStaging per method.
// It does not return while anything it queued can be in flight — wait() / fetch() on the normal path, the destructor on the exception
// path — so no stream handle is remembered past the call and the next call, on whatever stream, may reuse the slabs.
class CallStaging {
 public:
  CallStaging(int device, void* stream) : stream_(reinterpret_cast<hipStream_t>(stream)), t_(thread_staging(device)) {
    hip_check(hipSetDevice(device), "hipSetDevice");   // the slabs and the handle's kernels live on `device`
    t_.pinned.reset(); t_.device.reset();
  }
  ~CallStaging() { if (busy_) (void)hipStreamSynchronize(stream_); }   // (an exception is in flight: the error has nowhere to go)
  CallStaging(const CallStaging&) = delete;  CallStaging& operator=(const CallStaging&) = delete;

  // device space for n elements, not initialised (a kernel's output) ...
  template <typename T>
  T* out(size_t n) { busy_ = true; return static_cast<T*>(t_.device.take(n * sizeof(T))); }
  // ... or with every byte set
  template <typename T>
  T* out_filled(size_t n, int byte) {
    T* d = out<T>(n);
    if (n) hip_check(hipMemsetAsync(d, byte, n * sizeof(T), stream_), "hipMemset");
    return d;
  }
  // n elements of a host array, uploaded (`host` may be a temporary of the caller)
  template <typename T>
  T* in(const T* host, size_t n) {
    T* d = out<T>(n);
    if (n) { T* st = pin<T>(n); std::memcpy(st, host, n * sizeof(T)); push(d, st, n); }
    return d;
  }
  // one row of a pooled array, `cap` elements of `width`: the first n from `host` (NULL = none), the others `fill`
  template <typename T>
  T* in_rows(const T* host, size_t n, size_t cap, size_t width, T fill = T()) {
    T* d = out<T>(cap * width);
    if (cap * width == 0) return d;
    T* st = pin<T>(cap * width);
    const size_t have = host ? n * width : 0;
    std::copy(host, host + have, st);
    std::fill(st + have, st + cap * width, fill);
    push(d, st, cap * width);
    return d;
  }
  // the call's kernels have run (the handle's stream only: a device-wide wait would also wait for LocalMapping's optimizer)
  void wait() { hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize"); busy_ = false; }
  template <typename T>
  void fetch(const T* dev, T* host, size_t n) {
    if (!n) return;
    busy_ = true;
    hip_check(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H");
    wait();
  }
  template <typename T>
  std::vector<T> fetch(const T* dev, size_t n) { std::vector<T> v(n); fetch(dev, v.data(), n); return v; }

 private:
  template <typename T>
  T* pin(size_t n) { return static_cast<T*>(t_.pinned.take(n * sizeof(T))); }
  template <typename T>
  void push(T* d, const T* st, size_t n) { hip_check(hipMemcpyAsync(d, st, n * sizeof(T), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D"); }

  hipStream_t stream_;
  ThreadStaging& t_;
  bool busy_ = false;   // something has been handed out or queued since the last wait()
};

// An owning device array for a caller of the device-pointer entry points OUTSIDE an adapter call (ORBmatcher::handle(),
// Optimizer::optimizer()): blocking copies, freed with the object — an automatic variable, never static or thread_local (see above).
template <typename T>
class DeviceBuffer {
 public:
  explicit DeviceBuffer(size_t n) : n_(n) { hip_check(hipMalloc(reinterpret_cast<void**>(&p_), (n ? n : 1) * sizeof(T)), "hipMalloc"); }
  DeviceBuffer(const T* host, size_t n) : DeviceBuffer(n) { if (n) hip_check(hipMemcpy(p_, host, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy H2D"); }
  explicit DeviceBuffer(const std::vector<T>& v) : DeviceBuffer(v.data(), v.size()) {}
  ~DeviceBuffer() { (void)hipFree(p_); }
  DeviceBuffer(const DeviceBuffer&) = delete;  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  std::vector<T> to_host() const {
    std::vector<T> v(n_);
    if (n_) hip_check(hipMemcpy(v.data(), p_, n_ * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    return v;
  }
  T* get() { return p_; }  const T* get() const { return p_; }

 private:
  T* p_ = nullptr; size_t n_;
};

}  // namespace morb_adapter
