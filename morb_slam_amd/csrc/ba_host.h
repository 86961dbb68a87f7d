// Host side shared by the three bundle adjusters (local_ba.hip: LocalBA and the welding BA of map merging; inertial_ba.hip: LocalInertialBA):
// the carve of one device block into arrays, the flattened graph's lists, and the host loop that queues Levenberg-Marquardt trials ahead of the
// device's decisions.  Host only (no HIP header), nothing here allocates: tests/native/ba_host_check.cc compiles it alone, with sanitizers.
#pragma once
#include <sched.h>
#include <time.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

namespace morb {

// Every array of a problem is carved from ONE device block: uploads first, gathered in a host mirror of that region and sent in ONE
// copy, device-only arrays behind them.  The caller runs one function of take() calls twice: dry (a fresh carver), which sizes the
// regions, and after bind(), which hands out the pointers.  Each array's size is therefore written once.
class ArenaCarver {
 public:
  // base: device block of uploadBytes() + deviceBytes(); stage: host mirror of its first uploadBytes().  Begins the real pass.
  void bind(char* base, char* stage) { base_ = base; stage_ = stage; real_ = true; next_ = 0; up_ = dev_ = 0; }
  // src != null: an array of the upload region, src copied to the mirror at the same offset; null: a device-only array.
  // Every array starts 256-aligned.  Dry pass: returns null.
  void* take(const void* src, size_t bytes) {
    const size_t sz = (std::max<size_t>(bytes, 8) + 255) / 256 * 256;
    if (!real_) { asked_.push_back({bytes, src != nullptr}); (src ? upCap_ : devCap_) += sz; return nullptr; }
    if (bad_ || next_ >= asked_.size() || asked_[next_].bytes != bytes || asked_[next_].upload != (src != nullptr)) { bad_ = true; return nullptr; }
    size_t& off = src ? up_ : dev_;
    const size_t at = off; off += sz; ++next_;
    if (!src) return base_ + upCap_ + at;
    memcpy(stage_ + at, src, bytes);
    return base_ + at;
  }
  size_t uploadBytes() const { return upCap_; }
  size_t deviceBytes() const { return devCap_; }
  // the real pass asked for exactly what the dry pass measured, request by request (a pure carve function cannot fail this)
  bool ok() const { return real_ && !bad_ && next_ == asked_.size(); }
 private:
  struct Asked { size_t bytes; bool upload; };
  std::vector<Asked> asked_;
  size_t upCap_ = 0, devCap_ = 0, up_ = 0, dev_ = 0, next_ = 0;
  char *base_ = nullptr, *stage_ = nullptr;
  bool real_ = false, bad_ = false;
};

// CSR lists of the items 0 .. n-1 by key, in item order: key k's items are items[start[k] .. start[k + 1]).  wanted != null: only
// the items of keys with wanted[key] >= 0 are listed (the other keys' lists are empty and `items` is compact).
inline void csr_by_key(const int* keys, int n, int nKeys, std::vector<int>& start, std::vector<int>& items, const int* wanted = nullptr) {
  start.assign(nKeys + 1, 0);
  for (int i = 0; i < n; ++i) if (!wanted || wanted[keys[i]] >= 0) ++start[keys[i] + 1];
  for (int k = 0; k < nKeys; ++k) start[k + 1] += start[k];
  items.resize(start[nKeys]);
  std::vector<int> fill(start.begin(), start.end() - 1);
  for (int i = 0; i < n; ++i) if (!wanted || wanted[keys[i]] >= 0) items[fill[keys[i]]++] = i;
}

// The lists of the wanted keys (wanted[k] >= 0) cut into chunks of at most `len` items, keys and chunks in ascending order: chunk c is
// positions [chunkStart[c], chunkEnd[c]) of chunkKey[c]'s list.  keyChunkStart != null: key k's chunks are [k], [k + 1]) of it.
inline void chunks_of(const std::vector<int>& start, const int* wanted, int len, std::vector<int>& chunkKey, std::vector<int>& chunkStart,
                      std::vector<int>& chunkEnd, std::vector<int>* keyChunkStart = nullptr) {
  const int nKeys = (int)start.size() - 1;
  chunkKey.clear(); chunkStart.clear(); chunkEnd.clear();
  if (keyChunkStart) keyChunkStart->assign(nKeys + 1, 0);
  for (int k = 0; k < nKeys; ++k) {
    if (keyChunkStart) (*keyChunkStart)[k] = (int)chunkKey.size();
    if (wanted[k] >= 0)
      for (int s = start[k]; s < start[k + 1]; s += len) { chunkKey.push_back(k); chunkStart.push_back(s); chunkEnd.push_back(std::min(s + len, start[k + 1])); }
  }
  if (keyChunkStart) (*keyChunkStart)[nKeys] = (int)chunkKey.size();
}

// The upper-triangle blocks (bi <= bj) of an nb x nb block matrix in row-major order, and index[bi * nb + bj] = position in `blocks`
// (schur_mfma.h).  I2: the caller's pair of ints (int2 on the device side).
template <class I2>
inline void schur_block_lists(int nb, std::vector<I2>& blocks, std::vector<int>& index) {
  blocks.clear();
  index.assign((size_t)nb * nb, 0);
  for (int bi = 0; bi < nb; ++bi)
    for (int bj = bi; bj < nb; ++bj) { index[(size_t)bi * nb + bj] = (int)blocks.size(); I2 b; b.x = bi; b.y = bj; blocks.push_back(b); }
}

// Levenberg-Marquardt with the control flow on the device, the host's part.  The device decides every trial and mirrors `decided` (trials
// decided so far) and `done` to mapped host memory; kernels queued behind the last decision return at once.  The host queues slot after slot
// (queueSlot(slot): one trial's launches; non-zero: a launch error), one ahead of the decisions: slot s + 1 once `decided` >= s, `done` is set,
// or look() — hipStreamQuery, asked at every 1024th look at the words — finds the stream idle.  tick() runs before every look at the words.
// Returns 1: `done` seen; 0: maxSlots queued without it (decisions may still be on their way: drain the stream before the words are reset);
// negative: queueSlot's error, or -1 when look() said Failed — nothing is queued behind either.  sleeps: counts the 50 us sleeps (tests).
enum class StreamLook { Busy, Idle, Failed };

template <class QueueSlot, class Look, class Tick>
int lm_slot_queue(int maxSlots, const int* decided, const int* done, QueueSlot&& queueSlot, Look&& look, Tick&& tick, int* sleeps = nullptr) {
  for (int slot = 0; slot < maxSlots; ++slot) {
    if (const int rc = queueSlot(slot)) return rc < 0 ? rc : -rc;
    // wait until all but the last queued trial are decided (or the solve is done) on the mapped host words, backing off in tiers: a
    // trial takes ~110 us, so the first ~30 us are `pause` spins (the decision of a short trial is picked up at once), then the thread yields
    // its core between looks (LocalMapping's thread no longer holds a core against Tracking's for the whole solve), and a wait that outlasts
    // 2 ms — a solve stuck behind other work on the device — sleeps 50 us at a time
    unsigned spins = 0;
    const auto tWait = std::chrono::steady_clock::now();
    while (!__atomic_load_n(done, __ATOMIC_ACQUIRE) && __atomic_load_n(decided, __ATOMIC_ACQUIRE) < slot) {
      tick();
      if ((++spins & 0x3FFu) == 0) {
        const StreamLook q = look();
        if (q == StreamLook::Idle) break;          // (everything queued has run: the words are final)
        if (q == StreamLook::Failed) return -1;    // a kernel fault: the words will never change
      }
      if (spins < 2048) __builtin_ia32_pause();
      else if ((spins & 0xFF) != 0 || std::chrono::steady_clock::now() - tWait < std::chrono::milliseconds(2)) sched_yield();
      else { struct timespec ts = {0, 50000}; nanosleep(&ts, nullptr); if (sleeps) ++*sleeps; }
    }
    if (__atomic_load_n(done, __ATOMIC_ACQUIRE)) return 1;
  }
  return 0;
}

}  // namespace morb
