// The forward fuses over a device-resident keyframe store where the reference has them -- the loop of
// LoopClosing::correctLoop (src/LoopClosing.cc:515-517) and the first fuse of LocalMapping::fuseMapPoints (src/LocalMapping.cc:399) --
// against the reference's real LoopClosing / LocalMapping / KeyFrame / MapPoint / Map / Camera / Frame declarations: compiled with
// -fsyntax-only by tests/test_fuse_points_host.py.  (Of correctLoop only the lines around the loop are here.)
#include <string>

#include <opencv2/opencv.hpp>
namespace cv {
inline void destroyWindow(const std::string&) {}
}  // namespace cv
#include "ORB_SLAM2/Camera.h"
#include "ORB_SLAM2/Frame.h"
#include "ORB_SLAM2/KeyFrame.h"
#include "ORB_SLAM2/LocalMapping.h"
#include "ORB_SLAM2/LoopClosing.h"
#include "ORB_SLAM2/Map.h"
#include "ORB_SLAM2/MapPoint.h"
#include "orbfe_loopfuse_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
static orbfe::dropin::KeyframeStore<>& keyframeStore() {
  static orbfe::dropin::KeyframeStore<> store(1241, 376, ORBExtractor::mnLevels);
  return store;
}
void LoopClosing::correctLoop(const Sim3Ret&, const KeyFramePtr&) {
  auto vConnectedKfs = mpCurrKeyFrame->getConnectedKfs(0);
  orbfe::dropin::fuseLoopPoints<Camera, Frame>(vConnectedKfs, mvLoopGroupMps, mpMap, keyframeStore());
}
void LocalMapping::fuseMapPoints() {
  std::vector<MapPoint::SharedPtr> vTargetMps;
  orbfe::dropin::fuse<Camera, Frame>(keyframeStore(), mpCurrKeyFrame, vTargetMps, mpMap, false, 3.0f, 0.6f);
}
}  // namespace ORB_SLAM2_ROS2
