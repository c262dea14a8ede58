// What INTEGRATION.md section 14 adds to LoopClosing::computeSim3, against the reference's real LoopClosing / KeyFrame / MapPoint / Camera /
// Sim3Ret / ORBMatcher declarations: compiled with -fsyntax-only by tests/test_sim3_host.py.  Only the new lines are here -- the solver
// alias, sim3Candidates with it, one iterate on a solver it made and one searchBySim3 on the Sim3Ret that iterate fills; the reference's
// RANSAC loop and tail (src/LoopClosing.cc:343-414) are left out: they stay as they are.
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
#include "orbfe_sim3_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
using DeviceSim3Solver = orbfe::Sim3Solver<KeyFrame, Sim3Ret, Camera>;

static orbfe::dropin::KeyframeStore<>& keyframeStore() {
  static orbfe::dropin::KeyframeStore<> store(1241, 376, ORBExtractor::mnLevels);
  return store;
}

bool LoopClosing::computeSim3(Sim3Ret& g2oScm, Sim3Ret& g2oScw, KeyFramePtr& pLoopKf) {
  const std::size_t count = mvEnoughKfs.size();
  std::vector<bool> discarded(count, false);
  std::vector<DeviceSim3Solver::SharedPtr> solvers(count, nullptr);
  std::vector<std::vector<cv::DMatch>> kept(count);
  if (orbfe::dropin::sim3Candidates<DeviceSim3Solver>(keyframeStore(), mpCurrKeyFrame, mvEnoughKfs, discarded, solvers, kept) == 0 || !solvers[0])
    return false;
  // one call of each kind the unchanged loop makes on the new type
  bool exhausted = false;
  std::vector<std::size_t> inlierIdx;
  const bool found = solvers[0]->iterate(5, g2oScm, exhausted, inlierIdx);
  ORBMatcher matcher(0.75, true);
  std::vector<cv::DMatch> guided;
  const int nGuided = found ? matcher.searchBySim3(mpCurrKeyFrame, mvEnoughKfs[0], guided, g2oScm, 7.5) : 0;
  (void)g2oScw;
  (void)pLoopKf;
  return nGuided > 0 && !exhausted;
}

// create's own call shape, with every defaulted argument given
DeviceSim3Solver::SharedPtr anyCreate(KeyFrame::SharedPtr pKfp, KeyFrame::SharedPtr pKfq, const std::vector<cv::DMatch>& matches,
                                      std::vector<bool>& vbChoose) {
  return DeviceSim3Solver::create(pKfp, pKfq, matches, vbChoose, true, 3, 100, 0.4f, 0.99f);
}
}  // namespace ORB_SLAM2_ROS2
