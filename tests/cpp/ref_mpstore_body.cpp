// Tracking::trackLocalMap's middle over a device-resident map-point store, against the reference's real
// Tracking / Frame / MapPoint / Camera declarations: compiled with -fsyntax-only by tests/test_mpstore_host.py.  Also the three hooks of
// the coherence contract as they would stand in MapPoint.cc, and the store's maintenance calls on the reference's types.
#include <string>

#include <opencv2/opencv.hpp>
namespace cv {
inline void destroyWindow(const std::string&) {}
}  // namespace cv
#include "ORB_SLAM2/Camera.h"
#include "ORB_SLAM2/Frame.h"
#include "ORB_SLAM2/Map.h"
#include "ORB_SLAM2/MapPoint.h"
#include "ORB_SLAM2/Tracking.h"
#include "orbfe_mpstore_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
static orbfe::dropin::MapPointStore<>& mapPointStore() {
  static orbfe::dropin::MapPointStore<> store;
  return store;
}
// the one line that stands for src/Tracking.cc:650-658 (next to INTEGRATION section 3b's)
int trackLocalMapStored(Frame::SharedPtr mpCurrFrame, std::vector<MapPoint::SharedPtr>& mvpLocalMps, float th) {
  int nGood = 0;
  const int nMatches = orbfe::dropin::trackLocalMap<Camera>(mapPointStore(), mpCurrFrame, mvpLocalMps, th, nGood);
  if (nMatches < 30) return -1;
  return nGood;
}
int trackLocalMapStoredAllArguments(Frame::SharedPtr mpCurrFrame, std::vector<MapPoint::SharedPtr>& mvpLocalMps, float th) {
  int nGood = 0;
  orbfe::dropin::trackLocalMap<Camera>(mapPointStore(), mpCurrFrame, mvpLocalMps, th, /*mfRatio=*/0.8f, ORBExtractor::mnLevels, nGood);
  return nGood;
}
// the hook: one line at the end of MapPoint::setPos, MapPoint::setDesc and MapPoint::updateNormalAndDepth
void touched(MapPoint::SharedPtr pMp) { mapPointStore().touch(pMp->getID()); }
// maintenance on the reference's types
std::vector<uint64_t> maintenance(std::vector<MapPoint::SharedPtr>& points) {
  mapPointStore().ensure(points);
  mapPointStore().flush([&](uint64_t id) { return id < points.size() ? points[id] : MapPoint::SharedPtr(); });
  mapPointStore().erase({(uint64_t)points.front()->getID()});
  return mapPointStore().verify(points);
}
}  // namespace ORB_SLAM2_ROS2
