// MOCKS — NOT DBoW2, NOT the reference.  What KeyFrameDatabase.cc, LoopClosing.cc:484 and Tracking.cc:3369 touch around the
// database, as the reference headers declare it: DBoW2::BowVector, ORBVocabulary, and a KeyFrame / Frame / Map with the members the
// adapter reads and writes.  The basic types come from tests/native/mock_ref/mock_types.h; mock_ref's own KeyFrame.h / Frame.h /
// Map.h lack these members and are not included.
#pragma once
#include <map>
#include <set>
#include <vector>

#include "mock_types.h"   // tests/native/mock_ref

namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
class BowVector : public std::map<WordId, WordValue> {};
}  // namespace DBoW2

namespace ORB_SLAM3 {
using std::vector;   // the reference headers bring std into scope (`using namespace std`)

struct ORBVocabulary { unsigned int size() const { return 1000; } };

class Map {
 public:
  bool IsBad() { return mbBad; }
  bool mbBad = false;
};

class KeyFrame {
 public:
  std::set<KeyFrame*> GetConnectedKeyFrames() { return mspConnected; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    return (int)mvpOrdered.size() < N ? mvpOrdered : std::vector<KeyFrame*>(mvpOrdered.begin(), mvpOrdered.begin() + N);
  }
  bool isBad() { return mbBad; }
  Map* GetMap() { return mpMap; }
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
  long unsigned int mnPlaceRecognitionQuery = 0, mnRelocQuery = 0;
  int mnPlaceRecognitionWords = 0, mnRelocWords = 0;
  float mPlaceRecognitionScore = 0, mRelocScore = 0;
  // (mock state)
  std::set<KeyFrame*> mspConnected; std::vector<KeyFrame*> mvpOrdered; bool mbBad = false; Map* mpMap = nullptr;
};

class Frame {
 public:
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
};

struct AtlasMock { Map* GetCurrentMap() { return mpCurrentMap; } Map* mpCurrentMap = nullptr; };
}  // namespace ORB_SLAM3
