// The two ORBMatcher::searchBySim3 bodies over a device-resident keyframe store, against the reference's
// real ORBMatcher / KeyFrame / MapPoint / Sim3Solver declarations: compiled with -fsyntax-only by tests/test_sim3_search_host.py.
#include <string>

#include <opencv2/opencv.hpp>
namespace cv {
inline void destroyWindow(const std::string&) {}
}  // namespace cv
#include "ORB_SLAM2/Camera.h"
#include "ORB_SLAM2/Frame.h"
#include "ORB_SLAM2/KeyFrame.h"
#include "ORB_SLAM2/LoopClosing.h"
#include "ORB_SLAM2/Map.h"
#include "ORB_SLAM2/MapPoint.h"
#include "ORB_SLAM2/ORBMatcher.h"
#include "ORB_SLAM2/Sim3Solver.h"
#include "orbfe_reloc_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
static orbfe::dropin::KeyframeStore<>& keyframeStore() {
  static orbfe::dropin::KeyframeStore<> store(1241, 376, ORBExtractor::mnLevels);
  return store;
}
int ORBMatcher::searchBySim3(KeyFramePtr mpCurr, KeyFramePtr mpMatch, std::vector<cv::DMatch> &matches, Sim3Ret &g2oScm, float th) {
  return orbfe::dropin::searchBySim3<Camera>(keyframeStore(), mpCurr, mpMatch, matches, g2oScm, th, mfRatio);
}
int ORBMatcher::searchBySim3(KeyFramePtr pCurr, const std::vector<MapPointPtr> &vLoopGroupMps, std::vector<MapPointPtr> &vMatchedMps, Sim3Ret &g2oScw,
                             float th) {
  return orbfe::dropin::searchBySim3<Camera>(keyframeStore(), pCurr, vLoopGroupMps, vMatchedMps, g2oScw, th, mfRatio);
}
}  // namespace ORB_SLAM2_ROS2
