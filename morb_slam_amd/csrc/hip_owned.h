// Owners of the HIP resources of libmorb_hip.so: device blocks, pinned host blocks, streams and events.  Every handle holds its
// resources through these, so a handle is released by deleting it and a failed create releases what it had made.  This is the
// only file of csrc/ that allocates or releases such resources (tests/test_hip_resources_cpu.py checks it).
//
// Growth policy (GrowOnly): a buffer grows to half as much again as asked (exactly what is asked when that fails) and keeps the
// outgrown blocks until its owner dies.  A kernel or copy queued earlier, on the handle's stream or a caller's, may still use an
// outgrown block, and hipFree would wait for the whole device: a tracking-thread call must not wait for a LocalBundleAdjustment
// another thread has running.  The retired bytes stay below twice the final size.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "common.h"

namespace morb {

// One device block (hipMalloc).  alloc() releases what the owner held first: the block is replaced, not grown.
template <class T = void>
class DeviceArray {
 public:
  DeviceArray() = default;
  DeviceArray(DeviceArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  DeviceArray& operator=(DeviceArray&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
    return *this;
  }
  ~DeviceArray() { reset(); }
  hipError_t alloc(size_t bytes) {
    reset();
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) { p_ = static_cast<T*>(p); bytes_ = bytes; }
    return e;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr; bytes_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t bytes() const { return bytes_; }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

// One pinned host block (hipHostMalloc with `flags`); a mapped block also holds its device address.
template <class T = void>
class PinnedArray {
 public:
  PinnedArray() = default;
  PinnedArray(PinnedArray&& o) noexcept
      : p_(std::exchange(o.p_, nullptr)), dev_(std::exchange(o.dev_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  PinnedArray& operator=(PinnedArray&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr); dev_ = std::exchange(o.dev_, nullptr); bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~PinnedArray() { reset(); }
  hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
    reset();
    void *p = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, flags);
    if (e != hipSuccess) return e;
    if ((flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer(&d, p, 0)) != hipSuccess) {
      (void)hipHostFree(p);
      return e;
    }
    p_ = static_cast<T*>(p); dev_ = static_cast<T*>(d); bytes_ = bytes;
    return hipSuccess;
  }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = dev_ = nullptr; bytes_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* dev() const { return dev_; }   // (mapped blocks only)
  size_t bytes() const { return bytes_; }

 private:
  T *p_ = nullptr, *dev_ = nullptr;
  size_t bytes_ = 0;
};

// Grow-only buffer of device (DeviceArray<>) or pinned host (PinnedArray<>) memory: see the growth policy above.
template <class Block>
class GrowOnly {
 public:
  int ensure(size_t bytes, void** out) {
    if (cur_.bytes() < bytes) {
      Block fresh;
      if (fresh.alloc(bytes + bytes / 2) != hipSuccess) {
        (void)hipGetLastError();
        const hipError_t e = fresh.alloc(bytes);
        if (e != hipSuccess) {
          set_error("cannot allocate a %zu-byte workspace: %s", bytes, hipGetErrorString(e));
          return MORB_ERR_HIP;
        }
      }
      if (cur_.get()) retired_.push_back(std::move(cur_));
      cur_ = std::move(fresh);
    }
    *out = cur_.get();
    return MORB_OK;
  }

 private:
  Block cur_;
  std::vector<Block> retired_;
};
using DeviceGrow = GrowOnly<DeviceArray<>>;
using PinnedGrow = GrowOnly<PinnedArray<>>;

class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
  hipError_t create(unsigned flags) { return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, flags); }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&&) = delete;
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  hipError_t create(unsigned flags) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace morb
