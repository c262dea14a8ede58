// dropin::OptimizeSim3 (orbfe_dropin.hpp) over minimal KeyFrame / MapPoint / Sim3Ret / Camera types: the whole body of
// Optimizer::OptimizeSim3 -- the vbIsInlier filter, the camera-frame points, the octave's information, the device call, the list and the
// model written back -- on the problems tests/test_gpu_sim3_opt.py writes, which compares the output with the Python binding's.
// Input: the case count, then per case: pose c and pose m (12 floats each), the start model (12 floats), the match count, and per match
//   cPw.xyz mPw.xyz  ckp.x ckp.y ckp.octave  mkp.x mkp.y mkp.octave  cState mState     (state 0 good, 1 null, 2 bad, 3 not in the map)
// Output per case: "ret | kept queryIdx ... | the model as float bits, mfS".  Then a line "fixed-scale only: ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>

#include <opencv2/opencv.hpp>

#include "orbfe_dropin.hpp"

namespace {

struct MapPoint {
  cv::Mat pos;
  bool bad = false, inMap = true;
  bool isBad() const { return bad; }
  bool isInMap() const { return inMap; }
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
  static float getScaledFactorInv2(const int& nLevel) { return 1.0f / (float)std::pow(1.2, 2 * nLevel); }
};

struct Sim3Ret {
  Sim3Ret() = default;
  Sim3Ret(const cv::Mat& Rqp, const cv::Mat& tqp, const float& s) : mfS(s) {
    Rqp.copyTo(mRqp);
    tqp.copyTo(mtqp);
  }
  void copyTo(Sim3Ret& other) {
    mRqp.copyTo(other.mRqp);
    mtqp.copyTo(other.mtqp);
    other.mfS = mfS;
  }
  cv::Mat mRqp, mtqp;
  float mfS = 0.f;
};

struct Camera {
  static float mfFx, mfFy, mfCx, mfCy;
};
float Camera::mfFx = 520.908620f, Camera::mfFy = 521.007327f, Camera::mfCx = 325.141442f, Camera::mfCy = 249.701764f;

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

void read_rt(std::ifstream& in, cv::Mat& R, cv::Mat& t) {
  double v[12];
  for (double& x : v) in >> x;
  R = cv::Mat(3, 3, CV_32F);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R.at<float>(r, c) = (float)v[3 * r + c];
  t = vec3(v + 9);
}

std::shared_ptr<MapPoint> make_point(const double* xyz, int state) {
  if (state == 1) return nullptr;
  auto p = std::make_shared<MapPoint>();
  p->pos = vec3(xyz);
  p->bad = state == 2;
  p->inMap = state != 3;
  return p;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  int cases = 0;
  in >> cases;
  for (int k = 0; k < cases; ++k) {
    auto kfc = std::make_shared<KeyFrame>(), kfm = std::make_shared<KeyFrame>();
    read_rt(in, kfc->R, kfc->t);
    read_rt(in, kfm->R, kfm->t);
    Sim3Ret scm;
    read_rt(in, scm.mRqp, scm.mtqp);
    scm.mfS = 1.0f;
    int n = 0;
    in >> n;
    std::vector<cv::DMatch> matches;
    for (int i = 0; i < n; ++i) {
      double c[3], m[3], ck[2], mk[2];
      int co = 0, mo = 0, cs = 0, ms = 0;
      in >> c[0] >> c[1] >> c[2] >> m[0] >> m[1] >> m[2] >> ck[0] >> ck[1] >> co >> mk[0] >> mk[1] >> mo >> cs >> ms;
      kfc->mps.push_back(make_point(c, cs));
      kfm->mps.push_back(make_point(m, ms));
      kfc->kps.emplace_back((float)ck[0], (float)ck[1], 31.f, -1.f, 0.f, co);
      kfm->kps.emplace_back((float)mk[0], (float)mk[1], 31.f, -1.f, 0.f, mo);
      matches.emplace_back(i, i, 0.f);
    }
    if (k == 0) {  // O1: a free scale is refused before anything is read, and nothing changes
      bool threw = false;
      try {
        orbfe::dropin::OptimizeSim3<Camera>(kfc, kfm, matches, scm, false);
      } catch (const std::invalid_argument&) {
        threw = true;
      }
      if (!threw || (int)matches.size() != n) return std::fprintf(stderr, "bFixedScale == false was not refused\n"), 1;
    }
    const int ret = orbfe::dropin::OptimizeSim3<Camera>(kfc, kfm, matches, scm);
    std::printf("%d |", ret);
    for (const auto& m : matches) std::printf(" %d", m.queryIdx);
    std::printf(" |");
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) std::printf(" %08x", bits(scm.mRqp.at<float>(r, c)));
    for (int r = 0; r < 3; ++r) std::printf(" %08x", bits(scm.mtqp.at<float>(r)));
    std::printf(" %08x\n", bits(scm.mfS));
  }
  std::printf("fixed-scale only: ok\n");
  return 0;
}
