// orbfe_pnp_dropin_impl.hpp -- the bodies of orbfe_pnp_dropin.hpp (src/PnPSolver.cc becomes `#include <orbfe_pnp_dropin_impl.hpp>`).
// Intrinsics come from Camera::mfFx .. mfCy and thresholds from Frame::getScaledFactor2, through PnpBodies<Camera, Frame>: the
// reference's classes by default; a translation unit that defines ORBFE_PNP_MINIMAL_TYPES declares its own Camera / Frame first.
#pragma once

#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>

#include "orbfe_pnp_dropin.hpp"

#ifndef ORBFE_PNP_MINIMAL_TYPES
#include "ORB_SLAM2/Camera.h"
#include "ORB_SLAM2/Frame.h"
#endif

namespace ORB_SLAM2_ROS2 {
namespace orbfe_pnp_detail {

struct Batch {
  std::vector<int64_t> offsets{0};
  std::vector<float> xyz, uv;
  std::vector<int32_t> octave;
  orbfe_pnp* set = nullptr;
  std::mutex mu;

  ~Batch() {
    if (set) orbfe_pnp_destroy(set);
  }
};

// the batch solvers created on this thread join until one of them iterates
inline std::weak_ptr<Batch>& open_batch() {
  static thread_local std::weak_ptr<Batch> b;
  return b;
}

inline void check(orbfe_status st) {
  if (st != ORBFE_OK) throw std::runtime_error(std::string("orbfe_pnp: ") + orbfe_last_error(nullptr));
}

template <class CameraT, class FrameT>
struct PnpBodies {
  static void upload(Batch& b) {
    if (b.set) return;
    int max_oct = 0;
    for (int32_t o : b.octave) max_oct = o > max_oct ? o : max_oct;
    std::vector<float> sigma2((size_t)max_oct + 1);
    for (int l = 0; l <= max_oct; ++l) sigma2[(size_t)l] = FrameT::getScaledFactor2(l);
    orbfe_camera cam{};
    cam.fx = CameraT::mfFx;
    cam.fy = CameraT::mfFy;
    cam.cx = CameraT::mfCx;
    cam.cy = CameraT::mfCy;
    check(orbfe_pnp_create(0, (int32_t)b.offsets.size() - 1, b.offsets.data(), b.xyz.data(), b.uv.data(), b.octave.data(), sigma2.data(),
                           (int32_t)sigma2.size(), &cam, nullptr, &b.set));
  }
};

}  // namespace orbfe_pnp_detail

inline PnPSolver::SharedPtr PnPSolver::create(std::vector<cv::Mat>& vMapPoints, std::vector<cv::KeyPoint>& vORBPoints) {
  std::shared_ptr<orbfe_pnp_detail::Batch> b = orbfe_pnp_detail::open_batch().lock();
  if (!b || b->set) {
    b = std::make_shared<orbfe_pnp_detail::Batch>();
    orbfe_pnp_detail::open_batch() = b;
  }
  SharedPtr s(new PnPSolver());
  s->mpBatch = b;
  s->mnProblem = (int)b->offsets.size() - 1;
  s->mnN = (int)vMapPoints.size();
  for (std::size_t i = 0; i < vMapPoints.size(); ++i) {
    const cv::Mat& p = vMapPoints[i];
    const cv::KeyPoint& kp = vORBPoints[i];
    b->xyz.push_back(p.at<float>(0));
    b->xyz.push_back(p.at<float>(1));
    b->xyz.push_back(p.at<float>(2));
    b->uv.push_back(kp.pt.x);
    b->uv.push_back(kp.pt.y);
    b->octave.push_back(kp.octave);
  }
  b->offsets.push_back(b->offsets.back() + (int64_t)vMapPoints.size());
  return s;
}

inline bool PnPSolver::iterate(int nIterations, PnPRet& modelRet, bool& bNoMore, std::vector<std::size_t>& vnInlierIndices) {
  orbfe_pnp_detail::Batch& b = *mpBatch;
  std::lock_guard<std::mutex> lk(b.mu);
  orbfe_pnp_detail::PnpBodies<Camera, Frame>::upload(b);
  float pose[12] = {};
  int32_t has = modelRet.error() ? 0 : 1;
  if (has) {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) pose[3 * r + c] = modelRet.mRcw.at<float>(r, c);
      pose[9 + r] = modelRet.mtcw.at<float>(r);
    }
  }
  const int64_t cap = (int64_t)vnInlierIndices.size() + (int64_t)(nIterations > 0 ? nIterations + 2 : 2) * mnN + 1;
  std::vector<int32_t> buf((size_t)cap);
  for (std::size_t i = 0; i < vnInlierIndices.size(); ++i) buf[i] = (int32_t)vnInlierIndices[i];
  int64_t k = (int64_t)vnInlierIndices.size();
  int32_t ret = 0, no_more = 0;
  orbfe_pnp_detail::check(orbfe_pnp_iterate(b.set, mnProblem, nIterations, pose, &has, buf.data(), &k, cap, &ret, &no_more));
  if (no_more) bNoMore = true;
  if (has) {
    modelRet.mRcw = cv::Mat(3, 3, CV_32F);
    modelRet.mtcw = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) modelRet.mRcw.at<float>(r, c) = pose[3 * r + c];
      modelRet.mtcw.at<float>(r) = pose[9 + r];
    }
  }
  vnInlierIndices.assign(buf.begin(), buf.begin() + k);
  return ret != 0;
}

}  // namespace ORB_SLAM2_ROS2
