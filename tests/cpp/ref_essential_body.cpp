// What INTEGRATION.md section 17 writes, against the reference's real Optimizer / LoopClosing / KeyFrame / MapPoint / Map / Sim3Ret
// declarations: compiled with -fsyntax-only by tests/test_essential_graph_host.py.  Optimizer::optimizeEssentialGraph with the drop-in as
// its whole body.
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
#include "ORB_SLAM2/Optimizer.h"
#include "ORB_SLAM2/Sim3Solver.h"
#include "orbfe_essential_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
void Optimizer::optimizeEssentialGraph(const LoopConnection& mLoopConnections, MapPtr mpMap, KeyFramePtr pLoopKf, KeyFramePtr pCurrKf,
                                       const int& graphTh, const KeyFrameAndSim3& mCorrectedG2oScw, const KeyFrameAndSim3& mNoCorrectedG2oScw,
                                       bool bFixScale) {
  orbfe::dropin::optimizeEssentialGraph<Sim3Ret>(mLoopConnections, mpMap, pLoopKf, pCurrKf, graphTh, mCorrectedG2oScw, mNoCorrectedG2oScw,
                                                 bFixScale);
}
}  // namespace ORB_SLAM2_ROS2
