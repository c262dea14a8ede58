// What INTEGRATION.md section 15 writes, against the reference's real Optimizer / LoopClosing / KeyFrame / MapPoint / Camera / Sim3Ret /
// ORBMatcher declarations: compiled with -fsyntax-only by tests/test_sim3_opt_host.py.  Optimizer::OptimizeSim3 with the drop-in as its
// whole body, and the second loop of LoopClosing::computeSim3 (src/LoopClosing.cc:343-380) with all four steps bound: the device solver's
// iterate, searchBySim3, OptimizeSim3.
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
#include "ORB_SLAM2/Optimizer.h"
#include "ORB_SLAM2/Sim3Solver.h"
#include "orbfe_dropin.hpp"
#include "orbfe_reloc_dropin.hpp"
#include "orbfe_sim3_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
int Optimizer::OptimizeSim3(KeyFramePtr pCurr, KeyFramePtr pMatch, Matches& inLier, Sim3Ret& g2oScm, bool bFixedScale) {
  return orbfe::dropin::OptimizeSim3<Camera>(pCurr, pMatch, inLier, g2oScm, bFixedScale);
}

using DeviceSim3Solver = orbfe::Sim3Solver<KeyFrame, Sim3Ret, Camera>;

static orbfe::dropin::KeyframeStore<>& keyframeStore() {
  static orbfe::dropin::KeyframeStore<> store(1241, 376, ORBExtractor::mnLevels);
  return store;
}

bool LoopClosing::computeSim3(Sim3Ret& g2oScm, Sim3Ret& g2oScw, KeyFramePtr& pLoopKf) {
  const std::size_t n = mvEnoughKfs.size();
  std::vector<bool> vbDiscard(n, false);
  std::vector<DeviceSim3Solver::SharedPtr> vpSolvers(n, nullptr);
  std::vector<std::vector<cv::DMatch>> kept(n);
  int nCandidates = orbfe::dropin::sim3Candidates<DeviceSim3Solver>(keyframeStore(), mpCurrKeyFrame, mvEnoughKfs, vbDiscard, vpSolvers, kept);
  ORBMatcher matcher(0.75, true);
  bool bComplete = false;
  KeyFrame::SharedPtr pkfCandidate;
  std::vector<cv::DMatch> vMatches;
  while (!bComplete && nCandidates > 0) {
    for (std::size_t idx = 0; idx < n; ++idx) {
      pkfCandidate = mvEnoughKfs[idx];
      if (vbDiscard[idx]) continue;
      bool bNoMore = false;
      std::vector<std::size_t> vIndices;
      const bool ret = vpSolvers[idx]->iterate(5, g2oScm, bNoMore, vIndices);
      if (bNoMore) {
        vbDiscard[idx] = true;
        --nCandidates;
      }
      if (ret) {
        vMatches.clear();
        const int nMatches = matcher.searchBySim3(mpCurrKeyFrame, pkfCandidate, vMatches, g2oScm, 7.5);
        if (nMatches < 50) continue;
        const int nInlier = Optimizer::OptimizeSim3(mpCurrKeyFrame, pkfCandidate, vMatches, g2oScm);
        if (nInlier > 50) {
          bComplete = true;
          break;
        }
      }
    }
  }
  (void)g2oScw;
  (void)pLoopKf;
  return bComplete;
}
}  // namespace ORB_SLAM2_ROS2
