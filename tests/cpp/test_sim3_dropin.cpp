// The Sim3Solver drop-in (orbfe_sim3_dropin.hpp) over minimal KeyFrame / MapPoint / Sim3Ret / Camera types, driven by the second loop of
// LoopClosing::computeSim3 (n = 5, no candidate accepted): one line per iterate call -- problem, ret, bNoMore, the model as float bits
// (or '-'), the inliers -- which tests/test_gpu_sim3.py compares with the Python binding's.  On the way it checks what the drop-in adds
// to the C API: the vbChoose filter (a null and a bad map point are added to every problem), creation order as problem order, the set
// uploaded lazily at the first iterate, and a solver created after that starting a set of its own.
// Input: the problem count, then per problem its size, a line with pose p and pose q (12 floats each) and lines "P.xyz Q.xyz octP octQ".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>

#include <opencv2/opencv.hpp>

#include "orbfe_sim3_dropin.hpp"

namespace {

struct MapPoint {
  cv::Mat pos;
  bool bad = false;
  bool isBad() const { return bad; }
  cv::Mat getPos() const { return pos; }
};

struct KeyFrame {
  cv::Mat R, t;
  std::vector<std::shared_ptr<MapPoint>> mps;
  std::vector<cv::KeyPoint> kps;
  void getPose(cv::Mat& Rcw, cv::Mat& tcw) const {
    Rcw = R;
    tcw = t;
  }
  std::shared_ptr<MapPoint> getMapPoint(int i) const { return mps[(std::size_t)i]; }
  const cv::KeyPoint& getLeftKeyPoint(int i) const { return kps[(std::size_t)i]; }
  static float getScaledFactor2(const int& nLevel) { return (float)std::pow(1.2, 2 * nLevel); }
};

struct Sim3Ret {
  bool error() const { return mRqp.empty() || mtqp.empty() || mfS <= 0.0f; }
  cv::Mat mRqp, mtqp;
  float mfS = 0.f;
};

struct Camera {
  static float mfFx, mfFy, mfCx, mfCy;
};
float Camera::mfFx = 517.3f, Camera::mfFy = 516.5f, Camera::mfCx = 318.6f, Camera::mfCy = 255.3f;

using Solver = orbfe::Sim3Solver<KeyFrame, Sim3Ret, Camera>;

unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}

cv::Mat vec3(const double* v) {
  cv::Mat m(3, 1, CV_32F);
  for (int r = 0; r < 3; ++r) m.at<float>(r) = (float)v[r];
  return m;
}

void read_pose(std::ifstream& in, KeyFrame& kf) {
  double v[12];
  for (double& x : v) in >> x;
  kf.R = cv::Mat(3, 3, CV_32F);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) kf.R.at<float>(r, c) = (float)v[3 * r + c];
  kf.t = vec3(v + 9);
}

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                               \
    }                                                         \
  } while (0)

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  int K = 0;
  in >> K;
  std::vector<Solver::SharedPtr> solvers;
  std::vector<std::shared_ptr<KeyFrame>> keep;
  for (int k = 0; k < K; ++k) {
    int n = 0;
    in >> n;
    auto kfp = std::make_shared<KeyFrame>(), kfq = std::make_shared<KeyFrame>();
    read_pose(in, *kfp);
    read_pose(in, *kfq);
    std::vector<cv::DMatch> matches;
    // match 0: p's map point is null; the last match: q's map point is bad (both must leave through vbChoose)
    kfp->mps.push_back(nullptr);
    kfq->mps.push_back(std::make_shared<MapPoint>());
    kfp->kps.emplace_back(0.f, 0.f, 31.f, -1.f, 0.f, 0);
    kfq->kps.emplace_back(0.f, 0.f, 31.f, -1.f, 0.f, 0);
    matches.emplace_back(0, 0, 0.f);
    for (int i = 0; i <= n; ++i) {
      double v[6] = {0, 0, 1, 0, 0, 1};
      int op = 0, oq = 0;
      if (i < n) in >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5] >> op >> oq;
      auto mp = std::make_shared<MapPoint>(), mq = std::make_shared<MapPoint>();
      mp->pos = vec3(v);
      mq->pos = vec3(v + 3);
      mq->bad = i == n;
      kfp->mps.push_back(mp);
      kfq->mps.push_back(mq);
      kfp->kps.emplace_back(0.f, 0.f, 31.f, -1.f, 0.f, op);
      kfq->kps.emplace_back(0.f, 0.f, 31.f, -1.f, 0.f, oq);
      matches.emplace_back(i + 1, i + 1, 0.f);  // queryIdx: q's feature, trainIdx: p's
    }
    std::vector<bool> vbChoose(matches.size(), true);
    solvers.push_back(Solver::create(kfp, kfq, matches, vbChoose, false, 7));  // S1: bFixScale and nMinSet are ignored
    CHECK(!vbChoose.front() && !vbChoose.back());
    for (int i = 1; i <= n; ++i) CHECK(vbChoose[(std::size_t)i]);
    CHECK(solvers.back()->problem() == k && solvers.back()->size() == n);  // creation order
    keep.push_back(kfp);
    keep.push_back(kfq);
  }
  // nothing has been uploaded yet: no device call can have failed, and the engine is untouched
  uint32_t eng = 0;
  CHECK(orbfe_sim3_engine(&eng, nullptr) == ORBFE_OK && eng == 1);
  if (argc > 2 && !std::strcmp(argv[2], "create-only")) {  // the part that needs no device (tests/test_sim3_host.py)
    std::printf("created %d\n", K);
    return 0;
  }
  std::vector<bool> vbDiscard(K, false);
  int nCandidates = K;
  std::vector<std::size_t> vInliers;
  bool first = true;
  while (nCandidates) {
    for (int idx = 0; idx < K; ++idx) {
      if (vbDiscard[idx]) continue;
      bool bNoMore = false;
      Sim3Ret model;
      vInliers.clear();
      bool ret = solvers[idx]->iterate(5, model, bNoMore, vInliers);
      if (first && K > 0) {  // the set exists now: a new solver starts a set of its own
        std::vector<bool> choose(1, true);
        std::vector<cv::DMatch> one(1, cv::DMatch(1, 1, 0.f));
        Solver::SharedPtr late = Solver::create(keep[0], keep[1], one, choose);
        CHECK(late->problem() == 0);
        first = false;
      }
      std::printf("%d %d %d ", idx, ret ? 1 : 0, bNoMore ? 1 : 0);
      if (model.error()) {
        std::printf("-");
      } else {
        CHECK(model.mfS == 1.0f);
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) std::printf("%s%08x", r + c ? " " : "", bits(model.mRqp.at<float>(r, c)));
        for (int r = 0; r < 3; ++r) std::printf(" %08x", bits(model.mtqp.at<float>(r)));
      }
      std::printf(" |");
      for (std::size_t i = 0; i < vInliers.size(); ++i) std::printf(" %zu", vInliers[i]);
      std::printf("\n");
      if (bNoMore) {
        vbDiscard[idx] = true;
        --nCandidates;
      }
    }
  }
  return 0;
}
