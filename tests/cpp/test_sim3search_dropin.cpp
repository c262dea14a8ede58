// Both ORBMatcher::searchBySim3 overloads of orbfe_reloc_dropin.hpp (over a keyframe store) against the overloads of orbfe_dropin.hpp
// (keyframe uploaded per call) on minimal keyframe / map-point types, linked to liborbfe_hip.so.  Input (written by
// tests/test_gpu_sim3_search.py): the camera, the two similarities, the input matches, two keyframes (pose, then per feature position,
// octave, flag -- 1: a good map point, 3: one in the map too --, the point's position and distance range, the descriptor) and the loop
// group.  The same small map is loaded twice; copy A goes through the overloads without a store, copy B through those with one.  Equal:
// the match vectors, vMatchedMps (by the loop point's index) and both return values.  The image is 160 x 120: the geometry of the
// context the plain overloads search with (orbfe::dropin::matcherContext), whose grid the pair overload without a store uses.
// Exit code 0 and one line "OK <matches after the pair call> <new pairs> <nMatches of the points call> <slots filled>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>

#include <opencv2/opencv.hpp>

namespace ORB_SLAM2_ROS2 {
struct Camera {
  static inline float mfFx = 0, mfFy = 0, mfCx = 0, mfCy = 0;
};
struct MapPoint {
  typedef std::shared_ptr<MapPoint> SharedPtr;
  bool inMap = false;
  int index = -1;
  cv::Mat pos = cv::Mat(3, 1, CV_32F), view = cv::Mat(3, 1, CV_32F), desc = cv::Mat(1, 32, CV_8U);
  float mx = 0, mn = 0;
  bool isBad() const { return false; }
  bool isInMap() const { return inMap; }
  cv::Mat getPos() const { return pos.clone(); }
  cv::Mat getViewDirection() const { return view.clone(); }
  cv::Mat getDesc() const { return desc; }
  void getDistance(float& a, float& b) const { a = mx, b = mn; }
};
struct KeyFrame {
  typedef std::shared_ptr<KeyFrame> SharedPtr;
  uint64_t id = 0;
  std::vector<cv::KeyPoint> mvFeatsLeft;
  std::vector<cv::Mat> mvLeftDescriptor;
  std::vector<MapPoint::SharedPtr> mvpMapPoints;
  cv::Mat mRcw = cv::Mat(3, 3, CV_32F), mtcw = cv::Mat(3, 1, CV_32F);
  float mfMinU = 0, mfMaxU = 160, mfMinV = 0, mfMaxV = 120;
  static inline std::vector<float> mvfScaledFactors;
  const std::vector<cv::Mat>& getLeftDescriptor() const { return mvLeftDescriptor; }
  std::vector<MapPoint::SharedPtr> getMapPoints() { return mvpMapPoints; }
  void getPose(cv::Mat& R, cv::Mat& t) const { R = mRcw.clone(), t = mtcw.clone(); }
  float getScaledFactor2(int o) const { return mvfScaledFactors[(size_t)o] * mvfScaledFactors[(size_t)o]; }
};
struct Sim3Ret {  // include/ORB_SLAM2/Sim3Solver.h:14-48
  cv::Mat mRqp = cv::Mat(3, 3, CV_32F), mtqp = cv::Mat(3, 1, CV_32F);
  float mfS = 1.f;
};
}  // namespace ORB_SLAM2_ROS2

#include "orbfe_reloc_dropin.hpp"

using namespace ORB_SLAM2_ROS2;

struct Access {
  static uint64_t id(const KeyFrame::SharedPtr& k) { return k->id; }
  static void bounds(const KeyFrame::SharedPtr& k, float b[4]) { orbfe::dropin::Bodies::bounds(k, b); }
};

struct World {
  KeyFrame::SharedPtr C, M;
  Sim3Ret Scm, Scw;
  float thPair = 0, thPoints = 0, ratio = 0;
  std::vector<cv::DMatch> matches;
  std::vector<MapPoint::SharedPtr> loop;
};

static float num(std::ifstream& in) {
  double v = 0;
  in >> v;
  return (float)v;
}
static void mat(std::ifstream& in, cv::Mat& m, int rows, int cols) {
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) m.at<float>(r, c) = num(in);
}
static void descriptor(std::ifstream& in, cv::Mat& d) {
  for (int b = 0; b < 32; ++b) {
    int v = 0;
    in >> v;
    d.data[b] = (uint8_t)v;
  }
}

static World load(const char* path) {
  std::ifstream in(path);
  World w;
  Camera::mfFx = num(in), Camera::mfFy = num(in), Camera::mfCx = num(in), Camera::mfCy = num(in);
  int nLevels = 0;
  in >> nLevels;
  KeyFrame::mvfScaledFactors.resize((size_t)nLevels);
  for (auto& s : KeyFrame::mvfScaledFactors) s = num(in);
  w.thPair = num(in), w.thPoints = num(in), w.ratio = num(in);
  for (Sim3Ret* S : {&w.Scm, &w.Scw}) {
    S->mfS = num(in);
    mat(in, S->mRqp, 3, 3), mat(in, S->mtqp, 3, 1);
  }
  int nm = 0;
  in >> nm;
  for (int k = 0; k < nm; ++k) {
    cv::DMatch m;
    in >> m.queryIdx >> m.trainIdx;
    w.matches.push_back(m);
  }
  for (int k = 0; k < 2; ++k) {
    auto kf = std::make_shared<KeyFrame>();
    kf->id = k == 0 ? ((uint64_t)1 << 40) : 5;
    mat(in, kf->mRcw, 3, 3), mat(in, kf->mtcw, 3, 1);
    int n = 0;
    in >> n;
    for (int i = 0; i < n; ++i) {
      cv::KeyPoint kp;
      kp.pt.x = num(in), kp.pt.y = num(in);
      int fl = 0;
      in >> kp.octave >> fl;
      MapPoint::SharedPtr mp;
      cv::Mat pos(3, 1, CV_32F);
      mat(in, pos, 3, 1);
      const float mx = num(in), mn = num(in);
      if (fl & 1) {
        mp = std::make_shared<MapPoint>();
        mp->inMap = (fl & 2) != 0, mp->pos = pos, mp->mx = mx, mp->mn = mn;
      }
      cv::Mat ds(1, 32, CV_8U);
      descriptor(in, ds);
      kf->mvFeatsLeft.push_back(kp), kf->mvLeftDescriptor.push_back(ds), kf->mvpMapPoints.push_back(mp);
    }
    (k == 0 ? w.C : w.M) = kf;
  }
  int m = 0;
  in >> m;
  for (int j = 0; j < m; ++j) {
    int usable = 0;
    in >> usable;
    auto mp = std::make_shared<MapPoint>();
    mp->index = j, mp->inMap = true;
    mat(in, mp->pos, 3, 1), mat(in, mp->view, 3, 1);
    mp->mx = num(in), mp->mn = num(in);
    descriptor(in, mp->desc);
    w.loop.push_back(usable ? mp : nullptr);
  }
  return w;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  World A = load(argv[1]), B = load(argv[1]);
  orbfe::dropin::KeyframeStore<Access> store(160, 120, (int)KeyFrame::mvfScaledFactors.size());
  // the pair
  const size_t had = A.matches.size();
  const int ra = orbfe::dropin::searchBySim3<Camera>(A.C, A.M, A.matches, A.Scm, A.thPair, A.ratio);
  const int rb = orbfe::dropin::searchBySim3<Camera>(store, B.C, B.M, B.matches, B.Scm, B.thPair, B.ratio);
  if (store.size() != 2) return 3;  // both keyframes inserted on first use
  if (ra != rb || A.matches.size() != B.matches.size() || ra != (int)A.matches.size()) {
    std::fprintf(stderr, "pair: %d (%zu matches) without the store, %d (%zu) with it\n", ra, A.matches.size(), rb, B.matches.size());
    return 1;
  }
  for (size_t k = 0; k < A.matches.size(); ++k)
    if (A.matches[k].queryIdx != B.matches[k].queryIdx || A.matches[k].trainIdx != B.matches[k].trainIdx) {
      std::fprintf(stderr, "pair: match %zu is (%d, %d) without the store, (%d, %d) with it\n", k, A.matches[k].queryIdx, A.matches[k].trainIdx,
                   B.matches[k].queryIdx, B.matches[k].trainIdx);
      return 1;
    }
  // the loop group into C: two slots of vMatchedMps are taken by loop points already
  std::vector<MapPoint::SharedPtr> va(A.C->mvFeatsLeft.size()), vb(va.size());
  int taken = 0;
  for (size_t j = 0; j < A.loop.size() && taken < 2; ++j)
    if (A.loop[j]) va[(size_t)(3 + 4 * taken)] = A.loop[j], vb[(size_t)(3 + 4 * taken)] = B.loop[j], ++taken;
  const int na = orbfe::dropin::searchBySim3<Camera>(A.C, A.loop, va, A.Scw, A.thPoints, A.ratio);
  const int nb = orbfe::dropin::searchBySim3<Camera>(store, B.C, B.loop, vb, B.Scw, B.thPoints, B.ratio);
  if (na != nb || store.size() != 2) {
    std::fprintf(stderr, "points: %d without the store, %d with it\n", na, nb);
    return 4;
  }
  int filled = 0;
  for (size_t i = 0; i < va.size(); ++i) {
    if ((va[i] == nullptr) != (vb[i] == nullptr) || (va[i] && va[i]->index != vb[i]->index)) {
      std::fprintf(stderr, "points: slot %zu differs\n", i);
      return 5;
    }
    filled += va[i] != nullptr;
  }
  std::printf("OK %d %zu %d %d\n", ra, A.matches.size() - had, na, filled);
  return 0;
}
