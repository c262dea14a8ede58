// The whole body of Tracking::trackReference over a device-resident keyframe store, against the reference's
// real Tracking / KeyFrame / Frame / MapPoint declarations and host/compat's DBoW3::Vocabulary: compiled with -fsyntax-only by
// tests/test_track_reference_host.py.
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
#include "ORB_SLAM2/PnPSolver.h"
#include "ORB_SLAM2/Sim3Solver.h"
#include "ORB_SLAM2/Tracking.h"
#include "orbfe_reloc_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
static orbfe::dropin::KeyframeStore<>& keyframeStore() {
  static orbfe::dropin::KeyframeStore<> store(1241, 376, ORBExtractor::mnLevels);
  return store;
}
// the one line that stands for src/Tracking.cc:362-370
bool Tracking::trackReference() { return orbfe::dropin::trackReference<Camera>(keyframeStore(), mpVoc, mpCurrFrame, mpRefKf); }
}  // namespace ORB_SLAM2_ROS2
