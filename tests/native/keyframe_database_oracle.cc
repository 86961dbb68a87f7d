// CPU oracle of KeyFrameDatabase place recognition for tests/keyframe_database_oracle.py: a restatement, from the documented behaviour,
// of add / erase / clear / clearMap, DetectNBestCandidates and DetectRelocalizationCandidates with DBoW2's L1 score, in the
// reference's own data structures: std::map<int, double> BoW vectors, a std::list inverted file per word, per-keyframe stamp /
// words / score fields, std::set for the connected and the already-added keyframes, list::sort for the order by accumulated score.
// It is stateful across queries, as the database is.  The scalar pieces are include/morb/keyframe_database_math.h's, which the
// kernels share.
#include <list>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "morb/keyframe_database_math.h"

namespace {

typedef std::map<int, double> BowVector;

struct Map {
  bool bad = false;
};

struct KeyFrame {
  long id = 0;
  BowVector bow;
  Map* map = nullptr;
  bool bad = false;
  std::vector<KeyFrame*> covis;       // GetBestCovisibilityKeyFrames(10), in its order
  std::set<KeyFrame*> connected;      // GetConnectedKeyFrames()
  long placeQuery = 0, relocQuery = 0;
  int placeWords = 0, relocWords = 0;
  float placeScore = 0.f, relocScore = 0.f;
};

struct Database {
  std::vector<std::list<KeyFrame*>> inverted;
  std::vector<KeyFrame*> kfs;
  std::vector<Map*> maps;
  std::vector<KeyFrame*> lastSharing;   // lKFsSharingWords of the last query
  ~Database() {
    for (KeyFrame* k : kfs) delete k;
    for (Map* m : maps) delete m;
  }
  int index(const KeyFrame* k) const { return (int)k->id - 1; }
};

double score_l1(const BowVector& v1, const BowVector& v2) {
  BowVector::const_iterator a = v1.begin(), b = v2.begin();
  double score = 0;
  while (a != v1.end() && b != v2.end()) {
    if (a->first == b->first) {
      score += morbkfdb::l1_term(a->second, b->second);
      ++a;
      ++b;
    } else if (a->first < b->first) {
      a = v1.lower_bound(b->first);
    } else {
      b = v2.lower_bound(a->first);
    }
  }
  return -score / 2.0;
}

bool comp_first(const std::pair<float, KeyFrame*>& a, const std::pair<float, KeyFrame*>& b) { return a.first > b.first; }

// the part both detections share but for the field names: stamp, count, threshold, score, accumulate.  RELOC picks the fields.
template <bool RELOC>
bool accumulate(Database& db, const BowVector& qbow, long qid, const std::set<KeyFrame*>* connected,
                std::list<std::pair<float, KeyFrame*>>& lAcc, float& bestAccScore) {
  auto Q = [](KeyFrame* k) -> long& { return RELOC ? k->relocQuery : k->placeQuery; };
  auto W = [](KeyFrame* k) -> int& { return RELOC ? k->relocWords : k->placeWords; };
  auto S = [](KeyFrame* k) -> float& { return RELOC ? k->relocScore : k->placeScore; };
  std::list<KeyFrame*> lSharing;
  for (BowVector::const_iterator vit = qbow.begin(); vit != qbow.end(); ++vit) {
    if (vit->first < 0 || vit->first >= (int)db.inverted.size()) continue;
    std::list<KeyFrame*>& lKFs = db.inverted[vit->first];
    for (std::list<KeyFrame*>::iterator lit = lKFs.begin(); lit != lKFs.end(); ++lit) {
      KeyFrame* k = *lit;
      if (Q(k) != qid) {
        W(k) = 0;
        if (!connected || !connected->count(k)) {
          Q(k) = qid;
          lSharing.push_back(k);
        }
      }
      W(k)++;
    }
  }
  db.lastSharing.assign(lSharing.begin(), lSharing.end());
  if (lSharing.empty()) return false;
  int maxCommonWords = 0;
  for (KeyFrame* k : lSharing)
    if (W(k) > maxCommonWords) maxCommonWords = W(k);
  const int minCommonWords = morbkfdb::min_common_words(maxCommonWords);
  std::list<std::pair<float, KeyFrame*>> lScore;
  for (KeyFrame* k : lSharing) {
    if (W(k) > minCommonWords) {
      const float si = (float)score_l1(qbow, k->bow);
      S(k) = si;
      lScore.push_back(std::make_pair(si, k));
    }
  }
  if (lScore.empty()) return false;
  bestAccScore = 0;
  for (std::list<std::pair<float, KeyFrame*>>::iterator it = lScore.begin(); it != lScore.end(); ++it) {
    KeyFrame* k = it->second;
    float bestScore = it->first;
    float accScore = bestScore;
    KeyFrame* pBest = k;
    for (KeyFrame* k2 : k->covis) {
      if (Q(k2) != qid) continue;
      accScore += S(k2);
      if (S(k2) > bestScore) {
        pBest = k2;
        bestScore = S(k2);
      }
    }
    lAcc.push_back(std::make_pair(accScore, pBest));
    if (accScore > bestAccScore) bestAccScore = accScore;
  }
  return true;
}

}  // namespace

extern "C" {

void* kfdb_oracle_create(int nwords) {
  Database* db = new Database;
  db->inverted.resize(nwords);
  return db;
}
void kfdb_oracle_destroy(void* h) { delete static_cast<Database*>(h); }

int kfdb_oracle_new_map(void* h) {
  Database& db = *static_cast<Database*>(h);
  db.maps.push_back(new Map);
  return (int)db.maps.size() - 1;
}
void kfdb_oracle_set_map_bad(void* h, int map, int bad) { static_cast<Database*>(h)->maps[map]->bad = bad != 0; }

// a keyframe outside the database; its id is its index + 1 (nonzero, as a stamp must be)
int kfdb_oracle_new_keyframe(void* h, int n, const int* word, const double* value, int map) {
  Database& db = *static_cast<Database*>(h);
  KeyFrame* k = new KeyFrame;
  for (int i = 0; i < n; ++i) k->bow[word[i]] = value[i];
  k->map = db.maps[map];
  db.kfs.push_back(k);
  k->id = (long)db.kfs.size();
  return (int)db.kfs.size() - 1;
}
void kfdb_oracle_set_bad(void* h, int kf, int bad) { static_cast<Database*>(h)->kfs[kf]->bad = bad != 0; }
void kfdb_oracle_set_covis(void* h, int kf, int n, const int* nb) {
  Database& db = *static_cast<Database*>(h);
  db.kfs[kf]->covis.clear();
  for (int i = 0; i < n; ++i)
    if (nb[i] >= 0) db.kfs[kf]->covis.push_back(db.kfs[nb[i]]);
}
void kfdb_oracle_set_connected(void* h, int kf, int n, const int* nb) {
  Database& db = *static_cast<Database*>(h);
  db.kfs[kf]->connected.clear();
  for (int i = 0; i < n; ++i) db.kfs[kf]->connected.insert(db.kfs[nb[i]]);
}

void kfdb_oracle_add(void* h, int kf) {
  Database& db = *static_cast<Database*>(h);
  KeyFrame* k = db.kfs[kf];
  for (BowVector::const_iterator vit = k->bow.begin(); vit != k->bow.end(); ++vit) db.inverted[vit->first].push_back(k);
}
void kfdb_oracle_erase(void* h, int kf) {
  Database& db = *static_cast<Database*>(h);
  KeyFrame* k = db.kfs[kf];
  for (BowVector::const_iterator vit = k->bow.begin(); vit != k->bow.end(); ++vit) {
    std::list<KeyFrame*>& l = db.inverted[vit->first];
    for (std::list<KeyFrame*>::iterator lit = l.begin(); lit != l.end(); ++lit)
      if (*lit == k) {
        l.erase(lit);
        break;
      }
  }
}
void kfdb_oracle_clear(void* h) {
  Database& db = *static_cast<Database*>(h);
  const size_t n = db.inverted.size();
  db.inverted.clear();
  db.inverted.resize(n);
}
void kfdb_oracle_clear_map(void* h, int map) {
  Database& db = *static_cast<Database*>(h);
  for (std::list<KeyFrame*>& l : db.inverted)
    for (std::list<KeyFrame*>::iterator lit = l.begin(); lit != l.end();) {
      if ((*lit)->map == db.maps[map]) lit = l.erase(lit);
      else ++lit;
    }
}

double kfdb_oracle_score(int n1, const int* w1, const double* v1, int n2, const int* w2, const double* v2) {
  BowVector a, b;
  for (int i = 0; i < n1; ++i) a[w1[i]] = v1[i];
  for (int i = 0; i < n2; ++i) b[w2[i]] = v2[i];
  return score_l1(a, b);
}

// DetectNBestCandidates(pKF = keyframe `query`, .., nNumCandidates) with pKF->mnId = qid; the lists as keyframe indices
void kfdb_oracle_detect_n_best(void* h, int query, long qid, int nNumCandidates, int* loopCand, int* nLoop, int* mergeCand, int* nMerge) {
  Database& db = *static_cast<Database*>(h);
  KeyFrame* pKF = db.kfs[query];
  *nLoop = *nMerge = 0;
  std::set<KeyFrame*> spConnectedKF = pKF->connected;
  std::list<std::pair<float, KeyFrame*>> lAcc;
  float bestAccScore = 0;
  if (!accumulate<false>(db, pKF->bow, qid, &spConnectedKF, lAcc, bestAccScore)) return;
  lAcc.sort(comp_first);
  std::set<KeyFrame*> spAlreadyAddedKF;
  for (std::list<std::pair<float, KeyFrame*>>::iterator it = lAcc.begin(); it != lAcc.end(); ++it) {   // the whole list is walked
    KeyFrame* k = it->second;
    if (k->bad) continue;
    if (!spAlreadyAddedKF.count(k)) {
      if (pKF->map == k->map && *nLoop < nNumCandidates) loopCand[(*nLoop)++] = db.index(k);
      else if (pKF->map != k->map && *nMerge < nNumCandidates && !k->map->bad) mergeCand[(*nMerge)++] = db.index(k);
      spAlreadyAddedKF.insert(k);
    }
  }
}

// DetectRelocalizationCandidates(F, pMap): F->mBowVec = keyframe `frame`'s vector, F->mnId = qid; returns the candidates' count
int kfdb_oracle_detect_reloc(void* h, int frame, long qid, int map, int* cand) {
  Database& db = *static_cast<Database*>(h);
  std::list<std::pair<float, KeyFrame*>> lAcc;
  float bestAccScore = 0;
  if (!accumulate<true>(db, db.kfs[frame]->bow, qid, nullptr, lAcc, bestAccScore)) return 0;
  std::set<KeyFrame*> spAlreadyAddedKF;
  int n = 0;
  for (std::list<std::pair<float, KeyFrame*>>::iterator it = lAcc.begin(); it != lAcc.end(); ++it) {
    if (morbkfdb::retained(it->first, bestAccScore)) {
      KeyFrame* k = it->second;
      if (k->map != db.maps[map]) continue;
      if (!spAlreadyAddedKF.count(k)) {
        cand[n++] = db.index(k);
        spAlreadyAddedKF.insert(k);
      }
    }
  }
  return n;
}

int kfdb_oracle_last_sharing(void* h, int* out) {
  Database& db = *static_cast<Database*>(h);
  for (size_t i = 0; i < db.lastSharing.size(); ++i) out[i] = db.index(db.lastSharing[i]);
  return (int)db.lastSharing.size();
}

// the fields of every keyframe: which = 0 place recognition, 1 relocalisation
void kfdb_oracle_get_state(void* h, int which, long* query, int* words, float* score) {
  Database& db = *static_cast<Database*>(h);
  for (size_t i = 0; i < db.kfs.size(); ++i) {
    const KeyFrame* k = db.kfs[i];
    query[i] = which ? k->relocQuery : k->placeQuery;
    words[i] = which ? k->relocWords : k->placeWords;
    score[i] = which ? k->relocScore : k->placeScore;
  }
}
void kfdb_oracle_set_scores(void* h, int which, const float* score) {
  Database& db = *static_cast<Database*>(h);
  for (size_t i = 0; i < db.kfs.size(); ++i) (which ? db.kfs[i]->relocScore : db.kfs[i]->placeScore) = score[i];
}

}  // extern "C"
