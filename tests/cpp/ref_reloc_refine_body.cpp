// What follows a successful iterate in Tracking::trackReLocalize over a device-resident keyframe store,
// against the reference's real Tracking / KeyFrame / Frame / MapPoint / PnPSolver declarations: compiled with -fsyntax-only by
// tests/test_reloc_refine_host.py.
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
// the one call that stands for src/Tracking.cc:565-584, with the types the loop around it has there (the loop itself, the reference's
// head and its tail stay as they are and are left out: this file checks the new line against the real declarations)
bool Tracking::trackReLocalize() {
  std::vector<KeyFrame::SharedPtr> vpCandidateKFs(1);
  RelocBowParam relocBowParam(1);
  std::vector<std::size_t> vInliers;
  PnPRet modelReti;
  const std::size_t idx = 0;
  return orbfe::dropin::relocRefine<Camera>(keyframeStore(), mpCurrFrame, vpCandidateKFs[idx], relocBowParam, idx, vInliers, modelReti.mRcw,
                                            modelReti.mtcw);
}
}  // namespace ORB_SLAM2_ROS2
