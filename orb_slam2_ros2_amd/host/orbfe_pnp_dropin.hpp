// orbfe_pnp_dropin.hpp -- ORB_SLAM2_ROS2::PnPSolver and PnPRet (include/ORB_SLAM2/PnPSolver.h) on the device EPnP RANSAC sets
// (orbfe_pnp, include/orbfe.h).  INTEGRATION.md section 9: include/ORB_SLAM2/PnPSolver.h becomes `#include <orbfe_pnp_dropin.hpp>` and
// src/PnPSolver.cc becomes `#include <orbfe_pnp_dropin_impl.hpp>`.  The public interface is the reference's: PnPRet (mRcw, mtcw,
// error(), copyTo()), PnPSolver::create(vector<cv::Mat>&, vector<cv::KeyPoint>&) and iterate(int, PnPRet&, bool&, vector<size_t>&).
// Solvers created one after another on a thread before the first iterate of any of them form one orbfe_pnp set, in creation order
// (Tracking::filterKFByBow's order); the set is uploaded at that first iterate.  A failed library call throws std::runtime_error.
#pragma once

#include <cstddef>
#include <memory>
#include <vector>

#include <opencv2/opencv.hpp>

#include "orbfe.h"

namespace ORB_SLAM2_ROS2 {

/// the result of PnP: empty Mats until a pose is found
struct PnPRet {
  bool error() const { return mRcw.empty() || mtcw.empty(); }

  void copyTo(PnPRet& other) {
    mRcw.copyTo(other.mRcw);
    mtcw.copyTo(other.mtcw);
  }

  cv::Mat mRcw;
  cv::Mat mtcw;
};

namespace orbfe_pnp_detail {
struct Batch;
}

/// RANSAC + EPnP (Ransac<PnPRet>::iterate exactly)
class PnPSolver {
 public:
  typedef std::shared_ptr<PnPSolver> SharedPtr;

  static SharedPtr create(std::vector<cv::Mat>& vMapPoints, std::vector<cv::KeyPoint>& vORBPoints);

  bool iterate(int nIterations, PnPRet& modelRet, bool& bNoMore, std::vector<std::size_t>& vnInlierIndices);

  PnPSolver(const PnPSolver&) = delete;
  PnPSolver& operator=(const PnPSolver&) = delete;

 private:
  PnPSolver() = default;

  std::shared_ptr<orbfe_pnp_detail::Batch> mpBatch;  ///< the set this solver belongs to
  int mnProblem = 0;                                 ///< its problem in the set
  int mnN = 0;                                       ///< its number of points
};

}  // namespace ORB_SLAM2_ROS2
