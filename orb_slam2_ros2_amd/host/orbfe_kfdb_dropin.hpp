// orbfe_kfdb_dropin.hpp -- ORB_SLAM2_ROS2::KeyFrameDB (include/ORB_SLAM2/KeyFrameDB.h) on the device keyframe database (orbfe_kfdb,
// include/orbfe.h).  INTEGRATION.md section 8: include/ORB_SLAM2/KeyFrameDB.h becomes `#include <orbfe_kfdb_dropin.hpp>` and
// src/KeyFrameDB.cc becomes `#include <orbfe_kfdb_dropin_impl.hpp>`.  The public interface is the reference's: the constructor
// (std::size_t nWordNum), addKeyFrame, eraseKeyFrame, findRelocKfs, findLoopCloseKfs and struct Group.
#pragma once

#include <cstdint>
#include <memory>
#include <mutex>
#include <set>
#include <unordered_map>
#include <vector>

#include <DBoW3/DBoW3.h>

#include "orbfe.h"

namespace ORB_SLAM2_ROS2 {

class KeyFrame;
class VirtualFrame;
class Frame;

struct Group {
  typedef std::shared_ptr<KeyFrame> KeyFramePtr;
  KeyFramePtr mpBestKf;
  double mfAccScore = 0;  // the reference leaves it uninitialised and adds to it
  std::vector<KeyFramePtr> mvpKfs;
};

class KeyFrameDB {
 public:
  typedef std::shared_ptr<KeyFrame> KeyFramePtr;
  typedef std::shared_ptr<Frame> FramePtr;
  typedef std::shared_ptr<VirtualFrame> VirtualFramePtr;
  typedef std::shared_ptr<DBoW3::Vocabulary> VocabPtr;
  typedef std::shared_ptr<KeyFrameDB> SharedPtr;

  KeyFrameDB(std::size_t nWordNum);
  ~KeyFrameDB();
  KeyFrameDB(const KeyFrameDB&) = delete;
  KeyFrameDB& operator=(const KeyFrameDB&) = delete;

  /// adds the keyframe (computeBow() first, as the reference does); an id already present is left as it is
  void addKeyFrame(KeyFramePtr pKf);

  /// removes the keyframe
  void eraseKeyFrame(KeyFramePtr pKf);

  /// relocalisation candidates: count -> minWordFilter -> groupFilter
  void findRelocKfs(FramePtr pFrame, std::vector<KeyFramePtr>& candidateKfs);

  /// loop candidates (appended, as the reference appends): count without the connected keyframes -> minWordFilter -> minScoreFilter ->
  /// groupFilter
  void findLoopCloseKfs(KeyFramePtr pFrame, std::vector<KeyFramePtr>& candidateKfs);

 private:
  struct Survivor {
    KeyFramePtr kf;
    double score;
  };
  // the query on the device, with every keyframe's bad flag brought up to date first; survivors in ascending id order
  std::vector<Survivor> query(const DBoW3::BowVector& bow, const std::vector<uint64_t>& ignore, const double* minScore);
  // groupFilter over the survivors with their own getOrderedConnectedKfs(10)
  static void groupFilter(const std::vector<Survivor>& survivors, std::vector<KeyFramePtr>& candidateKfs);
  // minScoreFilter's floor: 0 without connected keyframes, else 1 lowered to the smallest similarity of a good one
  double minScore(KeyFramePtr pFrame);

  orbfe_kfdb* mpDb = nullptr;
  std::mutex mMutex;                                     ///< guards the maps (the database has its own lock)
  std::unordered_map<uint64_t, KeyFramePtr> mKfs;        ///< id -> keyframe, to map results back
  std::unordered_map<uint64_t, bool> mBad;               ///< the bad flag the database holds
};

}  // namespace ORB_SLAM2_ROS2
