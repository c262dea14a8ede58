// The batched searchByBow of orbfe_reloc_dropin.hpp over minimal frame / map-point types, linked to liborbfe_hip.so.  Input (written by
// tests/test_gpu_bow_search.py): the query frame, then the candidate keyframes -- per feature its angle, its flag (1: a good map point,
// 3: one that is in the map too) and its descriptor, then the FeatureVector.  The same small map is loaded twice: copy A goes through the
// per-candidate orbfe::dropin::searchByBow loop (Tracking::filterKFByBow's shape: setMapPointsNull() before every candidate), copy B
// through the overload that takes a store.  Equal: the match vectors, every map point's addMatchInTrack count, the frame's final map
// points -- in tracking mode; the match vectors in loop mode (the query named by id) and with bAddMPs.
// Exit code 0 and one line "OK <tracking matches> <loop matches> <bAddMPs matches> <addMatchInTrack calls>" when the two agree.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>

#include <opencv2/opencv.hpp>

namespace ORB_SLAM2_ROS2 {
struct MapPoint {
  typedef std::shared_ptr<MapPoint> SharedPtr;
  bool inMap = false;
  int nMatchInTrack = 0, owner = -1, feature = -1;
  bool isBad() const { return false; }
  bool isInMap() const { return inMap; }
  void addMatchInTrack() { ++nMatchInTrack; }
};
struct VFrame {  // a Frame and a KeyFrame at once: what the bodies read of either
  typedef std::shared_ptr<VFrame> SharedPtr;
  uint64_t id = 0;
  std::vector<cv::KeyPoint> mvFeatsLeft;
  std::vector<cv::Mat> mvLeftDescriptor;
  std::vector<MapPoint::SharedPtr> mvpMapPoints;
  std::vector<double> depth, ru;
  std::map<unsigned, std::vector<unsigned>> mFeatVec;
  int nBowCalls = 0;
  bool isBad() const { return false; }
  void computeBow() { ++nBowCalls; }
  const std::vector<cv::KeyPoint>& getLeftKeyPoints() const { return mvFeatsLeft; }
  const std::vector<cv::Mat>& getDescriptor() const { return mvLeftDescriptor; }
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mvpMapPoints; }
  const std::vector<double>& getDepth() const { return depth; }
  const std::vector<double>& getRightU() const { return ru; }
  void setMapPointsNull() { mvpMapPoints.assign(mvpMapPoints.size(), nullptr); }
};
}  // namespace ORB_SLAM2_ROS2

#include "orbfe_reloc_dropin.hpp"

using namespace ORB_SLAM2_ROS2;

struct Access {  // the minimal frame has no bounds: the image
  static uint64_t id(const VFrame::SharedPtr& k) { return k->id; }
  static void bounds(const VFrame::SharedPtr&, float b[4]) { b[0] = 0, b[1] = 640, b[2] = 0, b[3] = 480; }
};

struct World {
  VFrame::SharedPtr frame;
  std::vector<VFrame::SharedPtr> kfs;
};

static World load(const char* path) {
  std::ifstream in(path);
  World w;
  int nkf = 0;
  in >> nkf;
  for (int k = 0; k < nkf; ++k) {
    auto f = std::make_shared<VFrame>();
    f->id = k == 0 ? ((uint64_t)1 << 40) : (uint64_t)k;
    int n = 0;
    in >> n;
    for (int i = 0; i < n; ++i) {
      cv::KeyPoint kp;
      double x, y, a;
      int fl;
      in >> x >> y >> a >> fl;
      kp.pt.x = (float)x, kp.pt.y = (float)y, kp.angle = (float)a, kp.octave = 0;
      cv::Mat ds(1, 32, CV_8U);
      for (int b = 0; b < 32; ++b) {
        int v;
        in >> v;
        ds.data[b] = (uint8_t)v;
      }
      MapPoint::SharedPtr mp;
      if (fl & 1) {
        mp = std::make_shared<MapPoint>();
        mp->inMap = (fl & 2) != 0, mp->owner = k, mp->feature = i;
      }
      f->mvFeatsLeft.push_back(kp), f->mvLeftDescriptor.push_back(ds), f->mvpMapPoints.push_back(mp);
    }
    int nn = 0;
    in >> nn;
    for (int j = 0; j < nn; ++j) {
      unsigned node;
      int c;
      in >> node >> c;
      auto& v = f->mFeatVec[node];
      for (int q = 0; q < c; ++q) {
        unsigned id;
        in >> id;
        v.push_back(id);
      }
    }
    if (k == 0) w.frame = f;
    else w.kfs.push_back(f);
  }
  return w;
}

static bool same(const std::vector<cv::DMatch>& a, const std::vector<cv::DMatch>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].queryIdx != b[i].queryIdx || a[i].trainIdx != b[i].trainIdx || a[i].distance != b[i].distance) return false;
  return true;
}

// one pass of a mode over both worlds: the per-candidate loop on A, the stored overload on B
static long pass(World& A, World& B, orbfe::dropin::KeyframeStore<Access>& store, bool bAddMPs, bool bLoop, bool byId) {
  std::vector<std::vector<cv::DMatch>> a(A.kfs.size()), b;
  const std::vector<MapPoint::SharedPtr> stateA = A.frame->mvpMapPoints, stateB = B.frame->mvpMapPoints;
  for (size_t k = 0; k < A.kfs.size(); ++k) {
    if (!bAddMPs && !bLoop) A.frame->setMapPointsNull();  // Tracking.cc:460
    orbfe::dropin::searchByBow(A.frame, A.kfs[k], a[k], bAddMPs, bLoop, 0.75f, true);
  }
  orbfe::dropin::searchByBow(store, B.frame, B.kfs, b, bAddMPs, bLoop, 0.75f, true, byId);
  long total = 0;
  for (size_t k = 0; k < a.size(); ++k) {
    if (!same(a[k], b[k])) {
      std::fprintf(stderr, "candidate %zu: %zu vs %zu matches (bAddMPs %d, bLoop %d)\n", k, a[k].size(), b[k].size(), (int)bAddMPs, (int)bLoop);
      return -1;
    }
    total += (long)a[k].size();
  }
  if (!bAddMPs && !bLoop) {  // the side effects: every candidate's counts, the frame's final points
    for (size_t k = 0; k < A.kfs.size(); ++k)
      for (size_t i = 0; i < A.kfs[k]->mvpMapPoints.size(); ++i) {
        const auto &pa = A.kfs[k]->mvpMapPoints[i], &pb = B.kfs[k]->mvpMapPoints[i];
        if ((pa == nullptr) != (pb == nullptr) || (pa && pa->nMatchInTrack != pb->nMatchInTrack)) return -2;
      }
    for (size_t i = 0; i < A.frame->mvpMapPoints.size(); ++i) {
      const auto &pa = A.frame->mvpMapPoints[i], &pb = B.frame->mvpMapPoints[i];
      if ((pa == nullptr) != (pb == nullptr) || (pa && (pa->owner != pb->owner || pa->feature != pb->feature))) return -3;
    }
    A.frame->mvpMapPoints = stateA, B.frame->mvpMapPoints = stateB;  // the later modes start from the loaded state
  }
  return total;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  World A = load(argv[1]), B = load(argv[1]);
  orbfe::dropin::KeyframeStore<Access> store(640, 480, 8);
  const long nTrack = pass(A, B, store, false, false, false);
  if (nTrack < 0) return 1;
  long bumps = 0;
  for (const auto& kf : B.kfs)
    for (const auto& p : kf->mvpMapPoints) bumps += p ? p->nMatchInTrack : 0;
  if (store.size() != B.kfs.size()) return 3;  // the candidates were inserted on first use, the frame went up as arrays
  const long nLoop = pass(A, B, store, false, true, true);  // LoopClosing's shape: the current keyframe by id
  if (nLoop < 0 || store.size() != B.kfs.size() + 1) return 4;
  const long nAdd = pass(A, B, store, true, false, false);
  if (nAdd < 0) return 5;
  std::printf("OK %ld %ld %ld %ld\n", nTrack, nLoop, nAdd, bumps);
  return 0;
}
