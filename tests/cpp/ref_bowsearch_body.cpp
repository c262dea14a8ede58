// Tracking::filterKFByBow and the first loop of LoopClosing::computeSim3 over a device-resident keyframe store (INTEGRATION.md section
// 13), against the reference's real Tracking / LoopClosing / KeyFrame / Frame / MapPoint / PnPSolver / Sim3Solver declarations: compiled
// with -fsyntax-only by tests/test_bow_search_host.py.
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
int Tracking::filterKFByBow(RelocBowParam& relocBowParam, std::vector<bool>& vbDiscard, const int& candidateNum,
                            std::vector<KeyFrame::SharedPtr>& vpCandidateKFs) {
  return orbfe::dropin::filterKFByBow<PnPSolver>(keyframeStore(), mpCurrFrame, relocBowParam, vbDiscard, candidateNum, vpCandidateKFs);
}
// the head of LoopClosing::computeSim3, up to `bool bComplete = false;` (src/LoopClosing.cc:300-342); the reference's RANSAC loop and
// its tail follow unchanged (left out here: this file checks the new lines against the real declarations)
bool LoopClosing::computeSim3(Sim3Ret& g2oScm, Sim3Ret& g2oScw, KeyFramePtr& pLoopKf) {
  int n = mvEnoughKfs.size();
  std::vector<bool> vbDiscard(n, false);
  std::vector<Sim3Solver::SharedPtr> vpSolvers(n, nullptr);
  std::vector<std::vector<cv::DMatch>> vvMatches(n);
  int nCandidates = orbfe::dropin::sim3Candidates<Sim3Solver>(keyframeStore(), mpCurrKeyFrame, mvEnoughKfs, vbDiscard, vpSolvers, vvMatches);
  return nCandidates > 0;
}
// the general call: a keyframe against candidates with bAddMPs, as arrays and by id
void anySearch(KeyFrame::SharedPtr pKf, Frame::SharedPtr pFrame, std::vector<KeyFrame::SharedPtr>& cands, std::vector<std::vector<cv::DMatch>>& all) {
  orbfe::dropin::searchByBow(keyframeStore(), pKf, cands, all, true, false, 0.6f, false, true);
  orbfe::dropin::searchByBow(keyframeStore(), pFrame, cands, all, false, false);
}
}  // namespace ORB_SLAM2_ROS2
