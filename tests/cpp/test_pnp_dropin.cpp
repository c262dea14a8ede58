// The PnPSolver drop-in (orbfe_pnp_dropin.hpp) over minimal Camera / Frame types, driven by Tracking::trackReLocalize's step-3 loop
// (n = 5, no candidate accepted): one line per iterate call -- problem, ret, bNoMore, the pose as float bits (or '-'), the inliers --
// which tests/test_gpu_pnp.py compares with the Python binding's.  Input: the problem count, then per problem its point count and
// lines "x y z u v octave".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>

#define ORBFE_PNP_MINIMAL_TYPES
#include <opencv2/opencv.hpp>

namespace ORB_SLAM2_ROS2 {
struct Camera {
  static float mfFx, mfFy, mfCx, mfCy;
};
float Camera::mfFx = 517.3f, Camera::mfFy = 516.5f, Camera::mfCx = 318.6f, Camera::mfCy = 255.3f;
struct Frame {
  static float getScaledFactor2(const int& nLevel) { return (float)std::pow(1.2, 2 * nLevel); }
};
}  // namespace ORB_SLAM2_ROS2

#include "orbfe_pnp_dropin_impl.hpp"

using namespace ORB_SLAM2_ROS2;

static unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  int K = 0;
  in >> K;
  std::vector<PnPSolver::SharedPtr> solvers;
  for (int k = 0; k < K; ++k) {
    int n = 0;
    in >> n;
    std::vector<cv::Mat> mapPoints;
    std::vector<cv::KeyPoint> ORBPoints;
    for (int i = 0; i < n; ++i) {
      double x, y, z, u, v;
      int o;
      in >> x >> y >> z >> u >> v >> o;
      cv::Mat p(3, 1, CV_32F);
      p.at<float>(0) = (float)x;
      p.at<float>(1) = (float)y;
      p.at<float>(2) = (float)z;
      mapPoints.push_back(p);
      ORBPoints.push_back(cv::KeyPoint((float)u, (float)v, 31.f, -1.f, 0.f, o));
    }
    solvers.push_back(PnPSolver::create(mapPoints, ORBPoints));
  }
  std::vector<bool> vbDiscard(K, false);
  int nCandidates = K;
  std::vector<std::size_t> vInliers;
  while (nCandidates) {
    for (int idx = 0; idx < K; ++idx) {
      if (vbDiscard[idx]) continue;
      bool bNoMore = false;
      PnPRet modelReti;
      vInliers.clear();
      bool ret = solvers[idx]->iterate(5, modelReti, bNoMore, vInliers);
      std::printf("%d %d %d ", idx, ret ? 1 : 0, bNoMore ? 1 : 0);
      if (modelReti.error()) {
        std::printf("-");
      } else {
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) std::printf("%s%08x", r + c ? " " : "", bits(modelReti.mRcw.at<float>(r, c)));
        for (int r = 0; r < 3; ++r) std::printf(" %08x", bits(modelReti.mtcw.at<float>(r)));
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
