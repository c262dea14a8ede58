// The whole body of Tracking::trackMotionModel over two frame slots and a device-resident map-point store,
// against the reference's real Tracking / Frame / MapPoint / Camera declarations: compiled with -fsyntax-only by
// tests/test_track_motion_host.py.
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
#include "ORB_SLAM2/Tracking.h"
#include "orbfe_motion_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
static orbfe::dropin::MapPointStore<>& mapPointStore() {
  static orbfe::dropin::MapPointStore<> store;
  return store;
}
// the body that stands for src/Tracking.cc:383-405 and processLastFrame (:685-694)
bool Tracking::trackMotionModel() {
  mpLastFrame->setPose(mTlr * mpLastFrame->getRefKF()->getPose());
  mpCurrFrame->setPose(mVelocity * mpLastFrame->getPose());
  return orbfe::dropin::trackMotionModel<Camera>(mpCurrFrame, mpLastFrame, mapPointStore(), mvpTempMappoints);
}
}  // namespace ORB_SLAM2_ROS2
