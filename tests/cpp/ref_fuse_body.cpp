// LocalMapping::fuseMapPoints (src/LocalMapping.cc:352-405) as its one-line body, against the reference's real
// LocalMapping / KeyFrame / MapPoint / Map / Camera / Frame declarations: compiled with -fsyntax-only by tests/test_fuse_host.py.
#include <string>

#include <opencv2/opencv.hpp>
namespace cv {
inline void destroyWindow(const std::string&) {}
}  // namespace cv
#include "ORB_SLAM2/Camera.h"
#include "ORB_SLAM2/Frame.h"
#include "ORB_SLAM2/KeyFrame.h"
#include "ORB_SLAM2/LocalMapping.h"
#include "ORB_SLAM2/Map.h"
#include "ORB_SLAM2/MapPoint.h"
#include "orbfe_fuse_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
void LocalMapping::fuseMapPoints() { orbfe::dropin::fuseMapPoints<Camera, Frame>(mpCurrKeyFrame, mpMap); }
}  // namespace ORB_SLAM2_ROS2
