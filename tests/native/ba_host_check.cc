// Host build of morb_slam_amd/csrc/ba_host.h (the bundle adjusters' shared host side) for tests/test_ba_host_cpu.py, a program of
// its own so that it can run under sanitizers.  The carver works on heap blocks of exactly the sizes it reports, so a write or a read
// outside them is AddressSanitizer's to find.  The graph lists are compared with a restatement, written here, of the loops the two
// adjusters had before the header: the vector-of-vectors form of LocalInertialBA and the full CSR with chunk offsets of LocalBA.
// The slot queue (lm_slot_queue) runs against a std::thread that plays the device: it "decides" the slots the host has queued by writing
// the two mirror words with release stores, so ThreadSanitizer (a second build of this program) sees the same accesses as the real words get.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "ba_host.h"

using namespace morb;

static long bad = 0, cases = 0;
#define CHECK(c) do { if (!(c)) { if (++bad <= 20) std::printf("FAILED %s  (line %d, case %ld)\n", #c, __LINE__, cases); } } while (0)

struct Req { size_t bytes; bool upload; };
struct I2 { int x, y; };

static size_t rounded(size_t bytes) { return (std::max<size_t>(bytes, 8) + 255) & ~(size_t)255; }

// one dry and one real pass over `reqs`, with request `grow` (if any) one byte larger in the real pass, `drop` (if any) left out of
// it and `flip` (if any) asked from the other region
static void carver_case(const std::vector<Req>& reqs, int grow = -1, int drop = -1, int flip = -1) {
  ++cases;
  const int n = (int)reqs.size();
  std::vector<std::unique_ptr<unsigned char[]>> src(n);   // exactly `bytes` (+ 1 for the grown request) each: ASan sees an over-read
  for (int i = 0; i < n; ++i) {
    const size_t len = reqs[i].bytes + (i == grow ? 1 : 0);
    src[i].reset(new unsigned char[len]);
    for (size_t b = 0; b < len; ++b) src[i][b] = (unsigned char)(31 * i + 7 * b + 1);
  }
  ArenaCarver A;
  size_t upWant = 0, devWant = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(A.take(reqs[i].upload ? src[i].get() : nullptr, reqs[i].bytes) == nullptr);
    (reqs[i].upload ? upWant : devWant) += rounded(reqs[i].bytes);
    CHECK(rounded(reqs[i].bytes) == ((std::max<size_t>(reqs[i].bytes, 16) + 255) & ~(size_t)255));   // LocalInertialBA's former rule
  }
  CHECK(!A.ok());   // (no real pass yet)
  CHECK(A.uploadBytes() == upWant && A.deviceBytes() == devWant);
  // the device block is only addressed, never touched; the mirror is written
  char* base = (char*)std::aligned_alloc(256, std::max<size_t>(upWant + devWant, 256));
  std::unique_ptr<char[]> stage(new char[upWant]);
  A.bind(base, stage.get());
  std::vector<char*> got(n, nullptr);
  for (int i = 0; i < n; ++i) {
    if (i == drop) continue;
    const bool upload = reqs[i].upload != (i == flip);
    got[i] = (char*)A.take(upload ? src[i].get() : nullptr, reqs[i].bytes + (i == grow ? 1 : 0));
  }
  const int firstBad = grow >= 0 ? grow : flip >= 0 ? flip : n;
  CHECK(A.ok() == (grow < 0 && drop < 0 && flip < 0));
  size_t upOff = 0, devOff = 0;
  std::vector<std::pair<size_t, size_t>> spans;
  for (int i = 0; i < n; ++i) {
    if (drop >= 0 && i >= drop) break;   // (a later request may or may not match the one measured at its new place: ok() is what counts)
    if (i >= firstBad) { CHECK(got[i] == nullptr); continue; }   // nothing is handed out behind a request that differs
    size_t& off = reqs[i].upload ? upOff : devOff;
    const size_t at = (size_t)(got[i] - base);
    CHECK(got[i] != nullptr && at == (reqs[i].upload ? 0 : upWant) + off);   // the offsets the dry pass's sizes give
    CHECK(((uintptr_t)got[i] & 255) == 0);
    if (reqs[i].upload) {
      CHECK(at + reqs[i].bytes <= upWant);
      CHECK(std::equal(src[i].get(), src[i].get() + reqs[i].bytes, (const unsigned char*)stage.get() + at));
    } else {
      CHECK(at >= upWant && at + reqs[i].bytes <= upWant + devWant);
    }
    spans.push_back({at, at + std::max<size_t>(reqs[i].bytes, 1)});
    off += rounded(reqs[i].bytes);
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i) CHECK(spans[i - 1].second <= spans[i].first);
  std::free(base);
}

static void carver_sweep(std::mt19937& rng) {
  const size_t edge[] = {0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 100000};
  std::vector<std::vector<Req>> lists;
  lists.push_back({});
  for (size_t b : edge) { lists.push_back({{b, true}}); lists.push_back({{b, false}}); }
  for (int pattern = 0; pattern < 4; ++pattern) {   // all edge sizes in one list: uploads first, device first, alternating both ways
    std::vector<Req> l;
    for (size_t k = 0; k < sizeof edge / sizeof *edge; ++k) l.push_back({edge[k], pattern == 0 ? k < 9 : pattern == 1 ? k >= 9 : (k + pattern) % 2 == 0});
    lists.push_back(l);
  }
  for (int t = 0; t < 120; ++t) {
    std::vector<Req> l(rng() % 40);
    for (Req& r : l) { r.bytes = rng() % 3 ? edge[rng() % 15] : rng() % 6000; r.upload = rng() % 2; }
    lists.push_back(l);
  }
  for (const auto& l : lists) {
    carver_case(l);
    for (int i = 0; i < (int)l.size(); ++i) { carver_case(l, i); carver_case(l, -1, i); carver_case(l, -1, -1, i); }
  }
  {   // one request more than the dry pass measured
    ++cases;
    ArenaCarver A;
    char s[4] = {1, 2, 3, 4}, stage[256], dev[512];
    A.take(s, 4);
    A.bind(dev, stage);
    CHECK(A.take(s, 4) == dev && A.ok());
    CHECK(A.take(nullptr, 4) == nullptr && !A.ok());
  }
}

// one graph: nKeys keyframes, key[e] of edge e, col[k] >= 0 for the optimizable ones
static void graph_case(const std::vector<int>& key, int nKeys, const std::vector<int>& col) {
  ++cases;
  const int n = (int)key.size();
  // LocalInertialBA as it was: the optimizable keyframes' edges, compact, cut into chunks of 64
  std::vector<std::vector<int>> byKF(nKeys);
  for (int e = 0; e < n; ++e) if (col[key[e]] >= 0) byKF[key[e]].push_back(e);
  std::vector<int> kfEdges, chunkKF, chunkStart, chunkEnd;
  for (int k = 0; k < nKeys; ++k)
    for (size_t s0 = 0; s0 < byKF[k].size(); s0 += 64) {
      chunkKF.push_back(k); chunkStart.push_back((int)kfEdges.size());
      const size_t s1 = std::min(byKF[k].size(), s0 + 64);
      for (size_t q = s0; q < s1; ++q) kfEdges.push_back(byKF[k][q]);
      chunkEnd.push_back((int)kfEdges.size());
    }
  std::vector<int> start, items, cK, cS, cE;
  csr_by_key(key.data(), n, nKeys, start, items, col.data());
  chunks_of(start, col.data(), 64, cK, cS, cE);
  CHECK(items == kfEdges && cK == chunkKF && cS == chunkStart && cE == chunkEnd);
  CHECK((int)start.size() == nKeys + 1 && start[0] == 0 && start[nKeys] == (int)kfEdges.size());
  for (int k = 0; k < nKeys; ++k) CHECK(std::equal(byKF[k].begin(), byKF[k].end(), items.begin() + start[k]) && start[k + 1] - start[k] == (int)byKF[k].size());
  std::vector<int> cat;
  for (size_t c = 0; c < cK.size(); ++c) { CHECK(cE[c] > cS[c] && cE[c] - cS[c] <= 64); cat.insert(cat.end(), items.begin() + cS[c], items.begin() + cE[c]); }
  CHECK(cat == kfEdges);
  // LocalBA as it was: every keyframe's edges, chunks of the free keyframes as offsets into that list, chunk ranges per keyframe
  std::vector<std::vector<int>> all(nKeys);
  for (int e = 0; e < n; ++e) all[key[e]].push_back(e);
  std::vector<int> fullStart(nKeys + 1, 0), fullEdges, bK, bS, bE, kfChunkStart(nKeys + 1, 0);
  for (int k = 0; k < nKeys; ++k) { fullEdges.insert(fullEdges.end(), all[k].begin(), all[k].end()); fullStart[k + 1] = (int)fullEdges.size(); }
  for (int k = 0; k < nKeys; ++k) {
    kfChunkStart[k] = (int)bK.size();
    if (col[k] >= 0)
      for (int s = fullStart[k]; s < fullStart[k + 1]; s += 64) { bK.push_back(k); bS.push_back(s); bE.push_back(std::min(s + 64, fullStart[k + 1])); }
  }
  kfChunkStart[nKeys] = (int)bK.size();
  std::vector<int> kcs;
  csr_by_key(key.data(), n, nKeys, start, items);
  chunks_of(start, col.data(), 64, cK, cS, cE, &kcs);
  CHECK(start == fullStart && items == fullEdges && cK == bK && cS == bS && cE == bE && kcs == kfChunkStart);
  cat.clear();
  for (size_t c = 0; c < cK.size(); ++c) cat.insert(cat.end(), items.begin() + cS[c], items.begin() + cE[c]);
  CHECK(cat == kfEdges);   // both adjusters walk the same edges in the same order
}

static void graph_sweep(std::mt19937& rng) {
  graph_case({}, 1, {0});   // n = 0
  graph_case({}, 5, {0, -1, 1, 2, -1});
  for (int len : {1, 63, 64, 65, 127, 128, 129}) {   // one keyframe with exactly `len` edges among others, optimizable and not
    for (int wanted = 0; wanted < 2; ++wanted) {
      std::vector<int> key;
      for (int e = 0; e < len; ++e) { key.push_back(2); if (e % 3 == 0) key.push_back(e % 2 ? 0 : 4); }
      graph_case(key, 6, {0, -1, wanted ? 1 : -1, 2, 3, -1});   // (keys 1, 3 and 5 have no items)
    }
  }
  for (int t = 0; t < 400; ++t) {
    const int nKeys = 1 + rng() % 12, n = t % 7 == 0 ? rng() % 8 : rng() % 400;
    std::vector<int> col(nKeys), key(n);
    int nOpt = 0;
    for (int& c : col) c = rng() % 3 ? nOpt++ : -1;
    const int hot = rng() % nKeys, empty = rng() % nKeys;   // one crowded keyframe, one without items (unless it is the only one)
    for (int& k : key) { k = rng() % 2 ? hot : (int)(rng() % nKeys); if (k == empty) k = hot; }
    graph_case(key, nKeys, col);
  }
}

static void block_list_sweep() {
  for (int nb = 1; nb <= 40; ++nb) {
    ++cases;
    std::vector<I2> blocks(3, I2{-1, -1});   // (stale content must go)
    std::vector<int> index(5, -1);
    schur_block_lists(nb, blocks, index);
    CHECK((int)blocks.size() == nb * (nb + 1) / 2 && (int)index.size() == nb * nb);
    size_t k = 0;
    for (int bi = 0; bi < nb; ++bi)
      for (int bj = bi; bj < nb; ++bj, ++k) {
        CHECK(k < blocks.size() && blocks[k].x == bi && blocks[k].y == bj);
        CHECK(index[(size_t)bi * nb + bj] == (int)k);
      }
    CHECK(k == blocks.size());
    for (int bi = 0; bi < nb; ++bi) for (int bj = 0; bj < bi; ++bj) CHECK(index[(size_t)bi * nb + bj] == 0);   // (below the diagonal: unused, zero)
  }
}

// ---- lm_slot_queue ----
struct Words {
  int decided = 0, done = 0, stop = 0;   // the mapped words: the device's two, and the stop flag the host forwards
  std::atomic<int> queued{0};            // slots the host has launched
  std::atomic<bool> quit{false};
};
static void put(int* w, int v) { __atomic_store_n(w, v, __ATOMIC_RELEASE); }
static int get(const int* w) { return __atomic_load_n(w, __ATOMIC_ACQUIRE); }

// The device: decides the queued slots in order, each after usPerSlot; the decision of slot doneAt (if it is ever queued) raises `done`,
// as the real decision kernels do: `done` first, then the count with release.  decides == false: it only watches the forwarded stop flag,
// which raises `done` in either mode.
static void device(Words& w, int doneAt, int usPerSlot, bool decides = true) {
  for (int ran = 0; !w.quit.load();) {
    if (get(&w.stop)) { put(&w.done, 1); return; }
    if (!decides || ran >= w.queued.load()) { std::this_thread::yield(); continue; }
    if (usPerSlot) std::this_thread::sleep_for(std::chrono::microseconds(usPerSlot));
    if (ran == doneAt) put(&w.done, 1);
    put(&w.decided, ++ran);
    if (ran - 1 == doneAt) return;
  }
}

struct QueueRun {
  int ret = 0, looks = 0, sleeps = 0, queuedAtFailedLook = -1;
  long ticks = 0;
  std::vector<int> decidedSeen, idleSeen;   // per queued slot: `decided` as queueSlot read it, and whether the last look() before it said Idle
};

// the host: lm_slot_queue over w with `look` (called with the number of looks so far) and `tick`; queueSlot reports -7 at slot failAt
template <class Look, class Tick>
static QueueRun run_queue(Words& w, int maxSlots, Look&& look, Tick&& tick, int failAt = -1) {
  QueueRun r;
  bool idle = false;
  r.ret = lm_slot_queue(maxSlots, &w.decided, &w.done, [&](int slot) {
    CHECK(slot == (int)r.decidedSeen.size());
    r.decidedSeen.push_back(get(&w.decided)); r.idleSeen.push_back(idle); idle = false;
    w.queued.store(slot + 1);
    return slot == failAt ? 7 : 0;   // (a positive code: the queue reports it negative)
  }, [&]() {
    const StreamLook q = look(r.looks++);
    idle = q == StreamLook::Idle;
    if (q == StreamLook::Failed) r.queuedAtFailedLook = w.queued.load();
    return q;
  }, [&]() { ++r.ticks; tick(); }, &r.sleeps);
  CHECK(r.ticks >= 1024L * r.looks);   // tick() before every look at the words, look() at every 1024th
  // no slot s + 1 was queued while decided < s, `done` was clear (the queue would have returned) and the stream was busy
  for (size_t s = 1; s < r.decidedSeen.size(); ++s) CHECK(r.decidedSeen[s] >= (int)s - 1 || r.idleSeen[s]);
  return r;
}

static void queue_sweep() {
  const int maxSlots = 6;
  const auto busy = [](int) { return StreamLook::Busy; };
  const auto noTick = []() {};
  // 1. the decision of slot k raises `done`, behind k decided slots, at three device speeds.  The host is one slot ahead, so slots k and
  // perhaps k + 1 are queued.  k = maxSlots - 1: the last slot's decision is not waited for (the host only waits for the one before it), so
  // the queue may end with 0 — then `done` is on its way, which is what the callers' drain is for.  k = maxSlots: that slot does not exist.
  for (int us : {0, 20, 300})
    for (int k = 0; k <= maxSlots; ++k) {
      ++cases;
      Words w;
      std::thread dev(device, std::ref(w), k, us, true);
      const QueueRun r = run_queue(w, maxSlots, busy, noTick);
      if (k < maxSlots - 1) CHECK(r.ret == 1);
      else CHECK(k == maxSlots ? r.ret == 0 : r.ret == 0 || r.ret == 1);
      CHECK((int)r.decidedSeen.size() >= std::min(k + 1, maxSlots) && (int)r.decidedSeen.size() <= std::min(k + 2, maxSlots));
      for (size_t s = 0; s < r.idleSeen.size(); ++s) CHECK(!r.idleSeen[s]);
      if (us == 300 && k >= 2) CHECK(r.ticks >= k - 1);   // every wait but the last had to look more than once
      if (k == maxSlots) w.quit.store(true);   // 2. `done` never set: exactly maxSlots slots
      dev.join();
      CHECK(get(&w.done) == (k < maxSlots));
    }
  {   // 3. the stream fails at the first look: the queue returns although the words never change, and queues nothing more
    ++cases;
    Words w;
    const QueueRun r = run_queue(w, maxSlots, [](int) { return StreamLook::Failed; }, noTick);
    CHECK(r.ret < 0 && r.looks == 1 && r.queuedAtFailedLook == 2 && w.queued.load() == 2);   // (slot 0 is not waited for: one ahead)
  }
  {   // 4. an idle stream without a decision: the queue goes on to the limit ...
    ++cases;
    Words w;
    const QueueRun r = run_queue(w, maxSlots, [](int) { return StreamLook::Idle; }, noTick);
    CHECK(r.ret == 0 && (int)r.decidedSeen.size() == maxSlots && r.looks == maxSlots - 1);
    for (size_t s = 2; s < r.idleSeen.size(); ++s) CHECK(r.idleSeen[s] && r.decidedSeen[s] == 0);
  }
  {   // ... or to `done`: the second look finds the stream idle, the device then decides what is queued and slot 3 is the last
    ++cases;
    Words w;
    std::thread dev;
    const QueueRun r = run_queue(w, maxSlots, [&](int looks) {
      if (looks == 1) dev = std::thread(device, std::ref(w), 3, 0, true);
      return looks < 2 ? StreamLook::Idle : StreamLook::Busy;
    }, noTick);
    dev.join();
    CHECK(r.ret == 1 && r.decidedSeen.size() >= 4 && r.decidedSeen.size() <= 5 && r.idleSeen[2] && r.idleSeen[3]);
  }
  {   // 5. a launch error at slot 2: three calls, its code negative
    ++cases;
    Words w;
    std::thread dev(device, std::ref(w), -1, 0, true);
    const QueueRun r = run_queue(w, maxSlots, busy, noTick, 2);
    w.quit.store(true);
    dev.join();
    CHECK(r.ret == -7 && r.decidedSeen.size() == 3);
  }
  {   // 6. a stop the caller raises during a wait reaches the device through tick() before the wait ends: nothing else can end it
    ++cases;
    Words w;
    std::atomic<int> callerStop{0};
    std::thread dev(device, std::ref(w), -1, 0, false);
    std::thread caller([&]() { std::this_thread::sleep_for(std::chrono::milliseconds(1)); callerStop.store(1); });
    const QueueRun r = run_queue(w, maxSlots, busy, [&]() { if (callerStop.load()) put(&w.stop, 1); });
    caller.join(); dev.join();
    CHECK(r.ret == 1 && r.decidedSeen.size() == 2 && get(&w.decided) == 0 && r.ticks >= 1);
  }
  {   // 7. a decision that takes 5 ms, past the 2 ms tier, is still picked up, from the sleeping tier
    ++cases;
    Words w;
    std::thread dev(device, std::ref(w), 1, 5000, true);
    const QueueRun r = run_queue(w, maxSlots, busy, noTick);
    dev.join();
    CHECK(r.ret == 1 && r.sleeps >= 1 && r.decidedSeen.size() >= 2 && r.decidedSeen.size() <= 3);
  }
}

// "queue" as the only argument: the slot queue's cases alone (the ThreadSanitizer build: the other sweeps have one thread)
int main(int argc, char** argv) {
  const bool all = !(argc == 2 && std::string(argv[1]) == "queue");
  std::mt19937 rng(20240611);
  if (all) carver_sweep(rng);
  const long carverCases = cases;
  if (all) graph_sweep(rng);
  const long graphCases = cases - carverCases;
  if (all) block_list_sweep();
  const long blockCases = cases - carverCases - graphCases;
  queue_sweep();
  std::printf("carver cases %ld, graph cases %ld, block-list cases %ld, queue cases %ld\n", carverCases, graphCases, blockCases,
              cases - carverCases - graphCases - blockCases);
  std::printf("cases %ld\nmismatches %ld\n", cases, bad);
  return bad ? 1 : 0;
}
