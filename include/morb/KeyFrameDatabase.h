// Drop-in adapter: ORB_SLAM3::KeyFrameDatabase (reference include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) over
// morb_detect_n_best_candidates_batch / morb_detect_relocalization_candidates_batch on a matcher handle of its own: the constructor
// from a vocabulary, add, erase, clear, clearMap, SetORBVocabulary, DetectNBestCandidates (the call of LoopClosing.cc:484) and
// DetectRelocalizationCandidates (Tracking.cc:3369).  The members are templates on the caller's KeyFrame / Frame / Map / vocabulary
// types, so this header includes none of them; one database is used with ONE KeyFrame type.  DetectLoopCandidates, DetectCandidates
// and DetectBestCandidates have no call site in the reference and are not provided.
//   * No inverted file: the class owns a device pool of BoW vectors, one row per keyframe ever added, and each row's add rank
//     (morb_hip.h explains why that reproduces the list order).  add / erase / clear / clearMap touch host state only; the rows that
//     changed are uploaded when the next detection opens, so they need no device.
//   * Each detection stages the query's vector into a spare row, flattens the connected set, the covisibility table
//     (GetBestCovisibilityKeyFrames(10)), map ids and flags, reads the stored scores from the keyframes (mPlaceRecognitionScore /
//     mRelocScore: the state the previous query left), runs a batch of one, and writes mnPlaceRecognitionQuery / Words / Score (or
//     mnRelocQuery / Words / Score) back as the reference leaves them, including the count of 1 it leaves on a connected keyframe
//     that shares a word.
//   * As the C entries, it takes as given that a query id (pKF->mnId, F->mnId) never equals a stamp an earlier query left, nor the
//     initial 0.  The reference's constructor leaves mRelocScore uninitialised; whoever constructs the keyframes sets it to 0.
//   * Only the L1 score is built: the vocabulary is kept for SetORBVocabulary's sake and never read.
//   * The reference locks mMutex around its walks; the methods here lock one mutex as a whole.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_buffer.h"
#include "keyframe_database_math.h"
#include "morb_hip.h"

namespace ORB_SLAM3 {

class KeyFrame;   // the caller's: the return type of DetectRelocalizationCandidates(Frame*, Map*)

// One query over plain arrays, the view-taking form.  Rows are rows of this database's pool (add_row's return values).
struct KeyFrameDatabaseView {
  // in
  std::vector<int> word;           // the query's BoW vector, words ascending
  std::vector<double> value;
  int queryMap = 0;
  std::vector<int> connected;      // rows of GetConnectedKeyFrames() (N best only)
  int ncovis = 0;
  std::vector<int> covis;          // [rows][ncovis], -1 padded
  std::vector<int> mapId;          // [rows]
  std::vector<uint8_t> flags;      // [rows]: morbkfdb::KFDB_BAD, KFDB_MAP_BAD
  std::vector<float> prevScore;    // [rows]
  int nNumCandidates = 3;
  // out
  std::vector<int> loop, merge, cand;   // rows
  std::vector<int> words;               // [rows] common words of a stamped row, -1 otherwise
  std::vector<float> score;             // [rows] the stored score after the query
};

class KeyFrameDatabase {
 public:
  // KeyFrameDatabase(const ORBVocabulary& voc)  (:33-35)
  template <class Voc>
  explicit KeyFrameDatabase(const Voc& voc, int device = 0) : voc_(&voc), device_(device) {}
  ~KeyFrameDatabase() { if (h_) morb_matcher_destroy(h_); }
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

  // void add(KeyFrame* pKF)  (:37-44)
  template <class KF>
  void add(KF* pKF) {
    std::lock_guard<std::mutex> lock(mu_);
    std::vector<int> w;
    std::vector<double> v;
    bow_of(pKF->mBowVec, w, v);
    auto it = rowOf_.find(pKF);
    const int row = it != rowOf_.end() ? it->second : new_row(pKF);
    set_row(row, w, v);
    rows_[row].map = pKF->GetMap();
    if (rows_[row].rank < 0) rows_[row].rank = nextRank_++;   // (a second add of a keyframe in the database would list it twice there)
  }
  // void erase(KeyFrame* pKF)  (:46-64)
  template <class KF>
  void erase(KF* pKF) {
    std::lock_guard<std::mutex> lock(mu_);
    auto it = rowOf_.find(pKF);
    if (it != rowOf_.end()) rows_[it->second].rank = -1;
  }
  // void clear()  (:66-69)
  void clear() {
    std::lock_guard<std::mutex> lock(mu_);
    for (Row& r : rows_) r.rank = -1;
  }
  // void clearMap(Map* pMap)  (:71-93): by the map each keyframe has NOW (GetMap()), as the reference's walk reads it
  template <class KF = KeyFrame, class MapT>
  void clearMap(MapT* pMap) {
    std::lock_guard<std::mutex> lock(mu_);
    for (Row& r : rows_) {
      if (r.rank < 0) continue;
      const void* m = r.kf ? static_cast<const void*>(static_cast<KF*>(r.kf)->GetMap()) : r.map;
      if (m == static_cast<const void*>(pMap)) r.rank = -1;
    }
  }
  // void SetORBVocabulary(ORBVocabulary* pORBVoc)  (:816-820)
  template <class Voc>
  void SetORBVocabulary(Voc* pORBVoc) { voc_ = pORBVoc; }

  // void DetectNBestCandidates(KeyFrame* pKF, vector<KeyFrame*>& vpLoopCand, vector<KeyFrame*>& vpMergeCand, int nNumCandidates)  (:579-705)
  template <class KF>
  void DetectNBestCandidates(KF* pKF, std::vector<KF*>& vpLoopCand, std::vector<KF*>& vpMergeCand, int nNumCandidates) {
    std::lock_guard<std::mutex> lock(mu_);
    KeyFrameDatabaseView v;
    std::vector<int> touched;
    flatten<KF>(pKF->mBowVec, pKF->GetMap(), false, v, &touched, pKF);
    v.nNumCandidates = nNumCandidates;   // (below 1 the reference still stamps and scores, and pushes nothing)
    run(v, false);
    for (size_t r = 0; r < rows_.size(); ++r) {
      if (v.words[r] < 0) continue;
      KF* k = static_cast<KF*>(rows_[r].kf);
      k->mnPlaceRecognitionQuery = pKF->mnId;
      k->mnPlaceRecognitionWords = v.words[r];
      k->mPlaceRecognitionScore = v.score[r];
    }
    for (int r : touched) static_cast<KF*>(rows_[r].kf)->mnPlaceRecognitionWords = 1;   // :602 + :608 on a keyframe :603 never stamps
    vpLoopCand.reserve(std::max(nNumCandidates, 0));
    vpMergeCand.reserve(std::max(nNumCandidates, 0));
    for (int r : v.loop) vpLoopCand.push_back(static_cast<KF*>(rows_[r].kf));
    for (int r : v.merge) vpMergeCand.push_back(static_cast<KF*>(rows_[r].kf));
  }

  // vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F, Map* pMap)  (:707-814)
  template <class KF = KeyFrame, class FrameT, class MapT>
  std::vector<KF*> DetectRelocalizationCandidates(FrameT* F, MapT* pMap) {
    std::lock_guard<std::mutex> lock(mu_);
    KeyFrameDatabaseView v;
    flatten<KF>(F->mBowVec, pMap, true, v, nullptr, static_cast<KF*>(nullptr));
    run(v, true);
    std::vector<KF*> out;
    for (size_t r = 0; r < rows_.size(); ++r) {
      if (v.words[r] < 0) continue;
      KF* k = static_cast<KF*>(rows_[r].kf);
      k->mnRelocQuery = F->mnId;
      k->mnRelocWords = v.words[r];
      k->mRelocScore = v.score[r];
    }
    for (int r : v.cand) out.push_back(static_cast<KF*>(rows_[r].kf));
    return out;
  }

  // ---- the view-taking form: plain arrays, pool rows ----
  // a keyframe's BoW vector as a new row in the database (add order = call order); returns the row
  int add_row(const int* word, const double* value, int n, const void* map = nullptr) {
    std::lock_guard<std::mutex> lock(mu_);
    const int row = new_row(nullptr);
    set_row(row, std::vector<int>(word, word + n), std::vector<double>(value, value + n));
    rows_[row].map = map;
    rows_[row].rank = nextRank_++;
    return row;
  }
  void erase_row(int row) {
    std::lock_guard<std::mutex> lock(mu_);
    rows_.at(row).rank = -1;
  }
  int rows() const { return (int)rows_.size(); }
  int add_rank(int row) const { return rows_.at(row).rank; }
  void DetectNBestCandidates(KeyFrameDatabaseView& v) {
    std::lock_guard<std::mutex> lock(mu_);
    run(v, false);
  }
  void DetectRelocalizationCandidates(KeyFrameDatabaseView& v) {
    std::lock_guard<std::mutex> lock(mu_);
    run(v, true);
  }

  // What a detection hands the device besides the pool, from the reference's objects (host only): the query's vector and map, the
  // covisibility table, map ids, flags and stored scores of every row, the connected rows, and (touched) the connected rows in the
  // database that share a word with the query.
  template <class KF, class Bow, class MapT>
  void flatten(const Bow& qbow, MapT* qmap, bool reloc, KeyFrameDatabaseView& v, std::vector<int>* touched, KF* pKF) {
    const int n = (int)rows_.size();
    bow_of(qbow, v.word, v.value);
    std::map<const void*, int> mapIds;
    auto map_id = [&](const void* m) { return mapIds.emplace(m, (int)mapIds.size()).first->second; };
    v.queryMap = map_id(qmap);
    v.ncovis = 10;
    v.covis.assign((size_t)n * v.ncovis, -1);
    v.mapId.assign(n, -1);
    v.flags.assign(n, 0);
    v.prevScore.assign(n, 0.f);
    for (int r = 0; r < n; ++r) {
      KF* k = static_cast<KF*>(rows_[r].kf);
      if (!k || rows_[r].rank < 0) continue;   // outside the database: never met, never read
      auto* m = k->GetMap();
      v.mapId[r] = map_id(m);
      v.flags[r] = (uint8_t)((k->isBad() ? morbkfdb::KFDB_BAD : 0) | (m && m->IsBad() ? morbkfdb::KFDB_MAP_BAD : 0));
      v.prevScore[r] = reloc ? k->mRelocScore : k->mPlaceRecognitionScore;
      const std::vector<KF*> nb = k->GetBestCovisibilityKeyFrames(10);
      for (int j = 0; j < (int)nb.size() && j < v.ncovis; ++j) {
        auto it = rowOf_.find(nb[j]);
        if (it != rowOf_.end()) v.covis[(size_t)r * v.ncovis + j] = it->second;
      }
    }
    if (pKF) {
      for (KF* c : pKF->GetConnectedKeyFrames()) {
        auto it = rowOf_.find(c);
        if (it == rowOf_.end()) continue;
        v.connected.push_back(it->second);
        const Row& row = rows_[it->second];
        if (touched && row.rank >= 0 && shares_word(v.word, row.word)) touched->push_back(it->second);
      }
    }
  }

 private:
  struct Row {
    void* kf = nullptr;
    const void* map = nullptr;
    std::vector<int> word;
    std::vector<double> value;
    int rank = -1;       // position in add order, -1 = not in the database
    bool dirty = true;   // the device row is older than the host's
  };
  using Call = morb_adapter::CallStaging;

  template <class Bow>
  static void bow_of(const Bow& bow, std::vector<int>& w, std::vector<double>& v) {
    w.clear();
    v.clear();
    for (auto it = bow.begin(); it != bow.end(); ++it) { w.push_back((int)it->first); v.push_back((double)it->second); }
  }
  static bool shares_word(const std::vector<int>& a, const std::vector<int>& b) {
    size_t i = 0, j = 0;
    while (i < a.size() && j < b.size()) {
      if (a[i] == b[j]) return true;
      if (a[i] < b[j]) ++i; else ++j;
    }
    return false;
  }
  int new_row(void* kf) {
    rows_.emplace_back();
    rows_.back().kf = kf;
    if (kf) rowOf_[kf] = (int)rows_.size() - 1;
    return (int)rows_.size() - 1;
  }
  void set_row(int row, std::vector<int> w, std::vector<double> v) {
    rows_[row].word = std::move(w);
    rows_[row].value = std::move(v);
    rows_[row].dirty = true;
  }
  static void check(int rc) { if (rc < 0) throw std::runtime_error(morb_last_error()); }

  // the device pool holds every row and one spare row for the query; it is rebuilt when either dimension is outgrown
  void sync_pool(const KeyFrameDatabaseView& v, hipStream_t st) {
    const int n = (int)rows_.size();
    size_t widest = std::max<size_t>(v.word.size(), 1);
    for (const Row& r : rows_) widest = std::max(widest, r.word.size());
    if (n + 1 > poolRows_ || (int)widest > cap_) {
      poolRows_ = std::max(2 * poolRows_, std::max(n + 1, 64));
      cap_ = std::max((int)widest, cap_ + cap_ / 2);
      dWord_.reset(new morb_adapter::DeviceBuffer<int>((size_t)poolRows_ * cap_));
      dValue_.reset(new morb_adapter::DeviceBuffer<double>((size_t)poolRows_ * cap_));
      dCount_.reset(new morb_adapter::DeviceBuffer<int>((size_t)poolRows_));
      for (Row& r : rows_) r.dirty = true;
    }
    count_.assign((size_t)n + 1, 0);
    for (int r = 0; r <= n; ++r) {   // row n: the query
      const std::vector<int>& w = r < n ? rows_[r].word : v.word;
      const std::vector<double>& val = r < n ? rows_[r].value : v.value;
      count_[r] = (int)w.size();
      if (r < n && !rows_[r].dirty) continue;
      if (!w.empty()) {
        morb_adapter::hip_check(hipMemcpyAsync(dWord_->get() + (size_t)r * cap_, w.data(), w.size() * sizeof(int), hipMemcpyHostToDevice, st), "hipMemcpy H2D");
        morb_adapter::hip_check(hipMemcpyAsync(dValue_->get() + (size_t)r * cap_, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy H2D");
      }
      if (r < n) rows_[r].dirty = false;
    }
    morb_adapter::hip_check(hipMemcpyAsync(dCount_->get(), count_.data(), count_.size() * sizeof(int), hipMemcpyHostToDevice, st), "hipMemcpy H2D");
  }

  // a batch of one; the query is the spare row behind the pool's rows
  void run(KeyFrameDatabaseView& v, bool reloc) {
    const int n = (int)rows_.size(), nimg = n + 1, N = std::max(v.nNumCandidates, 1), ncovis = std::max(v.ncovis, 0);
    if (v.word.size() != v.value.size() || (int)v.mapId.size() != n || (int)v.flags.size() != n || (int)v.prevScore.size() != n ||
        v.covis.size() != (size_t)n * ncovis)
      throw std::runtime_error("KeyFrameDatabase: a view array does not have one entry per row");
    if (!h_ && morb_matcher_create(&h_, device_) != MORB_OK) throw std::runtime_error(std::string("morb_matcher_create: ") + morb_last_error());
    Call c(device_, morb_matcher_stream(h_));
    sync_pool(v, reinterpret_cast<hipStream_t>(morb_matcher_stream(h_)));
    std::vector<int> rank(nimg, -1), mapId(v.mapId), covis(v.covis);
    for (int r = 0; r < n; ++r) rank[r] = rows_[r].rank;
    mapId.push_back(v.queryMap);
    covis.resize((size_t)nimg * ncovis, -1);
    std::vector<uint8_t> flags(v.flags);
    flags.push_back(0);
    std::vector<float> prev(v.prevScore);
    prev.push_back(0.f);
    const int q = n, connStart[2] = {0, (int)v.connected.size()};
    const int *d_q = c.in(&q, 1), *d_qMap = c.in(&v.queryMap, 1), *d_rank = c.in(rank.data(), rank.size()), *d_map = c.in(mapId.data(), mapId.size());
    const int *d_covis = c.in(covis.data(), covis.size()), *d_cs = c.in(connStart, 2), *d_conn = c.in(v.connected.data(), v.connected.size());
    const uint8_t* d_flags = c.in(flags.data(), flags.size());
    const float* d_prev = c.in(prev.data(), prev.size());
    int *d_words = c.out<int>(nimg), *d_nA = c.out<int>(1), *d_nB = c.out<int>(1);
    int *d_A = c.out<int>(reloc ? nimg : N), *d_B = c.out<int>(N);
    float* d_score = c.out<float>(nimg);
    if (reloc)
      check(morb_detect_relocalization_candidates_batch(h_, 1, d_q, d_qMap, nimg, cap_, dWord_->get(), dValue_->get(), dCount_->get(), d_rank,
                                                        d_covis, ncovis, d_map, d_prev, d_A, d_nA, d_words, d_score, nullptr));
    else
      check(morb_detect_n_best_candidates_batch(h_, 1, d_q, nimg, cap_, dWord_->get(), dValue_->get(), dCount_->get(), d_rank, d_cs, d_conn,
                                                d_covis, ncovis, d_map, d_flags, d_prev, N, d_A, d_nA, d_B, d_nB, d_words, d_score, nullptr));
    c.wait();
    int nA = 0, nB = 0;
    c.fetch(d_nA, &nA, 1);
    if (!reloc) c.fetch(d_nB, &nB, 1);
    std::vector<int> A = c.fetch(d_A, (size_t)nA), B = c.fetch(d_B, (size_t)nB);
    v.words = c.fetch(d_words, (size_t)nimg);
    v.score = c.fetch(d_score, (size_t)nimg);
    v.words.resize(n);
    v.score.resize(n);
    v.loop.clear(); v.merge.clear(); v.cand.clear();
    if (reloc) v.cand = A;
    else if (v.nNumCandidates >= 1) { v.loop = A; v.merge = B; }
  }

  const void* voc_ = nullptr;
  int device_ = 0;
  morb_matcher* h_ = nullptr;
  std::mutex mu_;
  std::vector<Row> rows_;
  std::map<const void*, int> rowOf_;
  int nextRank_ = 0;
  // the device pool
  int poolRows_ = 0, cap_ = 0;
  std::unique_ptr<morb_adapter::DeviceBuffer<int>> dWord_, dCount_;
  std::unique_ptr<morb_adapter::DeviceBuffer<double>> dValue_;
  std::vector<int> count_;
};

}  // namespace ORB_SLAM3
