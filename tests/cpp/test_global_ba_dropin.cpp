// dropin::globalOptimization (orbfe_global_ba_dropin.hpp) over minimal KeyFrame / MapPoint / Camera types: the whole body of
// Optimizer::globalOptimization -- which keyframes and map points become vertices, the fixed flag, the edges with their measurements,
// information and Huber deltas, the device call, mTcwGBA / mPGBA written back -- on the scene tests/global_ba_dropin_scene.py writes.
//   test_global_ba_dropin IN build   everything up to the device call (no device needed): prints the graph
//   test_global_ba_dropin IN full    the whole function: prints the graph, then mTcwGBA / mPGBA of every keyframe and map point
// IN: nLevels invSigma2.. | nkf | per keyframe: id bad R[9] t[3] nkp (x y octave rightU).. | nmp | per map point: bad pos[3] nobs
//     (keyframe index, -1: an observer that no longer exists; feature index).. | n vpKfs indices (-1: null) | n vpMps indices (-1: null) |
//     useRk nIteration stop
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <opencv2/opencv.hpp>

#include "orbfe_global_ba_dropin.hpp"

namespace {

std::vector<float> g_inv_sigma2;

struct KeyFrame {
  std::size_t id = 0;
  bool bad = false;
  cv::Mat R, t, mTcwGBA;
  std::vector<cv::KeyPoint> kps;
  std::vector<double> rightU;
  bool isBad() const { return bad; }
  std::size_t getID() const { return id; }
  void getPose(cv::Mat& Rcw, cv::Mat& tcw) const {
    Rcw = R;
    tcw = t;
  }
  const cv::KeyPoint& getLeftKeyPoint(std::size_t i) const { return kps.at(i); }
  const double& getRightU(std::size_t i) const { return rightU.at(i); }
  float getScaledFactorInv2(int octave) const { return g_inv_sigma2.at((size_t)octave); }
  float getScaledFactorInv(int) const { return -1e30f; }  // (the local BA's mono edges use this one; globalOptimization must not)
};
using KeyFramePtr = std::shared_ptr<KeyFrame>;

struct MapPoint {
  typedef std::map<std::weak_ptr<KeyFrame>, std::size_t, std::owner_less<std::weak_ptr<KeyFrame>>> Observations;
  bool bad = false;
  cv::Mat pos, mPGBA;
  Observations obs;
  bool isBad() const { return bad; }
  cv::Mat getPos() const { return pos; }
  Observations getObservation() const { return obs; }
};
using MapPointPtr = std::shared_ptr<MapPoint>;

struct Camera {
  static inline float mfFx = 520.908620f, mfFy = 521.007327f, mfCx = 325.141442f, mfCy = 249.701764f, mfBf = 40.0f;
};

unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}
unsigned long long bits(double f) {
  unsigned long long u;
  std::memcpy(&u, &f, 8);
  return u;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN build|full\n", argv[0]), 2;
  const bool full = std::string(argv[2]) == "full";
  std::ifstream in(argv[1]);
  int nLevels = 0, nkf = 0, nmp = 0;
  in >> nLevels;
  g_inv_sigma2.resize((size_t)nLevels);
  for (auto& v : g_inv_sigma2) in >> v;
  in >> nkf;
  std::vector<KeyFramePtr> kfs;
  for (int k = 0; k < nkf; ++k) {
    auto kf = std::make_shared<KeyFrame>();
    int bad = 0, nkp = 0;
    in >> kf->id >> bad;
    kf->bad = bad != 0;
    kf->R = cv::Mat(3, 3, CV_32F), kf->t = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) in >> kf->R.at<float>(r, c);
    for (int r = 0; r < 3; ++r) in >> kf->t.at<float>(r);
    in >> nkp;
    kf->kps.resize((size_t)nkp), kf->rightU.resize((size_t)nkp);
    for (int i = 0; i < nkp; ++i) in >> kf->kps[(size_t)i].pt.x >> kf->kps[(size_t)i].pt.y >> kf->kps[(size_t)i].octave >> kf->rightU[(size_t)i];
    kfs.push_back(kf);
  }
  in >> nmp;
  std::vector<MapPointPtr> mps;
  for (int m = 0; m < nmp; ++m) {
    auto mp = std::make_shared<MapPoint>();
    int bad = 0, nobs = 0;
    mp->pos = cv::Mat(3, 1, CV_32F);
    in >> bad >> mp->pos.at<float>(0) >> mp->pos.at<float>(1) >> mp->pos.at<float>(2) >> nobs;
    mp->bad = bad != 0;
    for (int i = 0; i < nobs; ++i) {
      int k;
      std::size_t idx;
      in >> k >> idx;
      if (k >= 0) {
        mp->obs[kfs.at((size_t)k)] = idx;
      } else {
        auto gone = std::make_shared<KeyFrame>();  // an observer that is destroyed before the function runs
        mp->obs[gone] = idx;
      }
    }
    mps.push_back(mp);
  }
  std::vector<KeyFramePtr> vpKfs;
  std::vector<MapPointPtr> vpMps;
  int n = 0;
  in >> n;
  for (int i = 0; i < n; ++i) {
    int k;
    in >> k;
    vpKfs.push_back(k < 0 ? nullptr : kfs.at((size_t)k));
  }
  in >> n;
  for (int i = 0; i < n; ++i) {
    int k;
    in >> k;
    vpMps.push_back(k < 0 ? nullptr : mps.at((size_t)k));
  }
  int useRk = 0, nIteration = 0, stop = 0;
  in >> useRk >> nIteration >> stop;
  if (!in) return fprintf(stderr, "input ends early\n"), 2;

  using namespace orbfe::dropin;
  {
    const auto G = buildGlobalGraph(vpKfs, vpMps, useRk != 0);
    const orbfe_ba_problem prob = G.problem<Camera>();
    printf("c %016llx %016llx %016llx %016llx %016llx\n", bits(prob.fx), bits(prob.fy), bits(prob.cx), bits(prob.cy), bits(prob.bf));
    for (size_t v = 0; v < G.frames.size(); ++v) {
      printf("p %zu %d", G.frames[v]->id, (int)G.fixed[v]);
      for (int k = 0; k < 7; ++k) printf(" %016llx", bits(G.poses[7 * v + (size_t)k]));
      printf("\n");
    }
    for (size_t p = 0; p < G.landmarks.size(); ++p) {
      size_t index = 0;
      while (mps[index] != G.landmarks[p]) ++index;
      printf("l %zu %016llx %016llx %016llx\n", index, bits(G.points[3 * p]), bits(G.points[3 * p + 1]), bits(G.points[3 * p + 2]));
    }
    for (size_t e = 0; e < G.edgePose.size(); ++e)
      printf("e %d %d %d %016llx %016llx %016llx %016llx %016llx\n", G.edgePose[e], G.edgePoint[e], (int)G.isStereo[e], bits(G.meas[3 * e]),
             bits(G.meas[3 * e + 1]), bits(G.meas[3 * e + 2]), bits(G.info[e]), bits(G.huber[e]));
  }
  if (!full) return 0;
  bool bStop = stop != 0;
  globalOptimization<Camera>(vpKfs, vpMps, nIteration, &bStop, useRk != 0);
  for (size_t k = 0; k < kfs.size(); ++k) {
    printf("kf %zu", kfs[k]->id);
    if (kfs[k]->mTcwGBA.empty()) {
      printf(" none\n");
      continue;
    }
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) printf(" %08x", bits(kfs[k]->mTcwGBA.at<float>(r, c)));
    printf("\n");
  }
  for (size_t m = 0; m < mps.size(); ++m) {
    if (mps[m]->mPGBA.empty())
      printf("mp %zu none\n", m);
    else
      printf("mp %zu %08x %08x %08x\n", m, bits(mps[m]->mPGBA.at<float>(0)), bits(mps[m]->mPGBA.at<float>(1)), bits(mps[m]->mPGBA.at<float>(2)));
  }
  // nothing but mTcwGBA / mPGBA is written: poses and positions are as they came
  return 0;
}
