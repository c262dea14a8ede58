// What INTEGRATION.md section 18 writes, against the reference's real Optimizer / KeyFrame / MapPoint / Camera declarations: compiled
// with -fsyntax-only by tests/test_global_ba_host.py.  Optimizer::globalOptimization with the drop-in as its whole body.
#include <string>

#include <opencv2/opencv.hpp>
namespace cv {
inline void destroyWindow(const std::string&) {}
}  // namespace cv
#include "ORB_SLAM2/Camera.h"
#include "ORB_SLAM2/Frame.h"
#include "ORB_SLAM2/KeyFrame.h"
#include "ORB_SLAM2/Map.h"
#include "ORB_SLAM2/MapPoint.h"
#include "ORB_SLAM2/Optimizer.h"
#include "orbfe_global_ba_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
void Optimizer::globalOptimization(const std::vector<KeyFramePtr>& vpKfs, const std::vector<MapPointPtr>& vpMps, int nIteration, bool* bStopFlag,
                                   bool bUseRk) {
  orbfe::dropin::globalOptimization<Camera>(vpKfs, vpMps, nIteration, bStopFlag, bUseRk);
}
}  // namespace ORB_SLAM2_ROS2
