// The drop-in KeyFrameDB (orb_slam2_ros2_amd/host/orbfe_kfdb_dropin.hpp + _impl.hpp) over minimal shared_ptr keyframe and frame types with
// the members KeyFrameDB.cc touches; tests/test_gpu_kfdb.py writes the input and the restatement's candidates.
//   test_kfdb_dropin <in.txt>
// in.txt: `n_words n_vectors`, then per vector `n (word value_hex)*`; keyframe ids (vector i is keyframe i); bad ids; per keyframe its
// ordered covisible ids; then cases `reloc f 0 0 n want..` (a Frame with vector f) or `loop id n_all all.. n15 c15.. n want..` (a new
// KeyFrame `id` with vector id - 200, its connected keyframes given).  Prints KFDB_DROPIN_OK <cases> when every candidate list matches.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <vector>

#include <DBoW3/DBoW3.h>

#include "orbfe_kfdb_dropin.hpp"

namespace ORB_SLAM2_ROS2 {

class KeyFrame;

class VirtualFrame {
 public:
  typedef std::shared_ptr<VirtualFrame> SharedPtr;
  DBoW3::BowVector mBowVec, mGiven;
  int mnBowCalls = 0;
  void computeBow() {  // VirtualFrame::computeBow: only when empty (the transform itself is tests/test_gpu_bow.py's)
    ++mnBowCalls;
    if (mBowVec.empty()) mBowVec = mGiven;
  }
  const DBoW3::BowVector& getBowVec() const { return mBowVec; }
};

class Frame : public VirtualFrame {
 public:
  typedef std::shared_ptr<Frame> SharedPtr;
};

class KeyFrame : public VirtualFrame {
 public:
  typedef std::shared_ptr<KeyFrame> SharedPtr;
  typedef std::weak_ptr<KeyFrame> WeakPtr;
  struct WeakCompareFunc {
    bool operator()(const WeakPtr& a, const WeakPtr& b) const { return a.owner_before(b); }
  };
  typedef std::map<WeakPtr, std::size_t, WeakCompareFunc> ConnectedType;
  std::size_t mnId = 0;
  bool mbBad = false;
  std::vector<SharedPtr> mvOrdered, mvConnected15;
  ConnectedType mmAll;
  std::size_t getID() const { return mnId; }
  bool isBad() const { return mbBad; }
  std::vector<SharedPtr> getOrderedConnectedKfs(int n) {  // bad ones included: the drop-in skips them as groupFilter does
    return std::vector<SharedPtr>(mvOrdered.begin(), mvOrdered.begin() + std::min<std::size_t>(n, mvOrdered.size()));
  }
  std::vector<SharedPtr> getConnectedKfs(int) { return mvConnected15; }
  ConnectedType getAllConnected() { return mmAll; }
};

}  // namespace ORB_SLAM2_ROS2

#define ORBFE_KFDB_OWN_TYPES
#include "orbfe_kfdb_dropin_impl.hpp"

using namespace ORB_SLAM2_ROS2;

static double from_hex(const std::string& s) {
  uint64_t u = std::stoull(s, nullptr, 16);
  double v;
  std::memcpy(&v, &u, 8);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::size_t nWords, nVec;
  in >> nWords >> nVec;
  std::vector<DBoW3::BowVector> vec(nVec);
  for (auto& v : vec) {
    int n;
    in >> n;
    for (int i = 0; i < n; ++i) {
      unsigned w;
      std::string h;
      in >> w >> h;
      v.emplace(w, from_hex(h));
    }
  }
  auto readIds = [&]() {
    int n;
    in >> n;
    std::vector<std::size_t> ids((std::size_t)n);
    for (auto& x : ids) in >> x;
    return ids;
  };
  const auto kfIds = readIds();
  const auto badIds = readIds();
  std::map<std::size_t, KeyFrame::SharedPtr> kfs;
  for (auto id : kfIds) {
    auto kf = std::make_shared<KeyFrame>();
    kf->mnId = id;
    kf->mGiven = vec[id];
    kfs[id] = kf;
  }
  for (auto id : kfIds)
    for (auto c : readIds()) kfs[id]->mvOrdered.push_back(kfs.at(c));
  // System.cc:104-109: the database sized by the vocabulary, every keyframe of the map added
  auto mpKfDB = std::make_shared<KeyFrameDB>(nWords);
  for (auto id : kfIds) mpKfDB->addKeyFrame(kfs[id]);
  mpKfDB->addKeyFrame(kfs[kfIds[0]]);  // twice: nothing changes
  for (auto id : badIds) kfs[id]->mbBad = true;  // bad after being added: the query refreshes the flags
  int nCases;
  in >> nCases;
  int ok = 0;
  for (int c = 0; c < nCases; ++c) {
    std::string mode;
    std::size_t f;
    in >> mode >> f;
    const auto all = readIds(), c15 = readIds(), want = readIds();
    std::vector<KeyFrame::SharedPtr> cands;
    if (mode == "reloc") {  // Tracking.cc:418
      auto frame = std::make_shared<Frame>();
      frame->mGiven = vec[f];
      mpKfDB->findRelocKfs(frame, cands);
    } else {  // LoopClosing.cc:224 on a keyframe that is not in the database yet, then LoopClosing.cc:59 / LocalMapping.cc:731 add it
      auto kf = std::make_shared<KeyFrame>();
      kf->mnId = f;
      kf->mGiven = vec[f - 200];
      for (auto a : all) kf->mmAll.emplace(kfs.at(a), 20);
      for (auto a : c15) kf->mvConnected15.push_back(kfs.at(a));
      mpKfDB->findLoopCloseKfs(kf, cands);
      if (kf->mnBowCalls != 1) {
        std::printf("loop %zu: computeBow called %d times\n", f, kf->mnBowCalls);
        return 1;
      }
      mpKfDB->addKeyFrame(kf);
      mpKfDB->eraseKeyFrame(kf);  // and out again: the next case sees the same database
    }
    std::vector<std::size_t> got;
    for (auto& k : cands) got.push_back(k->getID());
    if (got != std::vector<std::size_t>(want.begin(), want.end())) {
      std::printf("%s %zu: got", mode.c_str(), f);
      for (auto g : got) std::printf(" %zu", g);
      std::printf(", want");
      for (auto w : want) std::printf(" %zu", w);
      std::printf("\n");
      return 1;
    }
    ++ok;
  }
  std::printf("KFDB_DROPIN_OK %d\n", ok);
  return 0;
}
