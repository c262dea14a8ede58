// LocalMapping::fuseMapPoints, createNewMapPoints and deleteKeyFrame over a device-resident keyframe store,
// and the insertion KeyFrame::create makes, against the reference's real LocalMapping / KeyFrame / MapPoint / Map / Camera / Frame
// declarations: compiled with -fsyntax-only by tests/test_kfstore_abi.py.
#include <string>

#include <opencv2/opencv.hpp>
namespace cv {
inline void destroyWindow(const std::string&) {}
}  // namespace cv
#include "ORB_SLAM2/Camera.h"
#include "ORB_SLAM2/Frame.h"
#include "ORB_SLAM2/KeyFrame.h"
#include "ORB_SLAM2/LocalMapping.h"
#include "ORB_SLAM2/Map.h"
#include "ORB_SLAM2/MapPoint.h"
#include "orbfe_kfstore_dropin.hpp"

namespace ORB_SLAM2_ROS2 {
static orbfe::dropin::KeyframeStore<>& keyframeStore() {
  static orbfe::dropin::KeyframeStore<> store(1241, 376, ORBExtractor::mnLevels);
  return store;
}
void LocalMapping::fuseMapPoints() { orbfe::dropin::fuseMapPoints<Camera, Frame>(mpCurrKeyFrame, mpMap, keyframeStore()); }
void LocalMapping::createNewMapPoints() {
  orbfe::dropin::createNewMapPoints<Camera, Frame>(mpCurrKeyFrame, mmUnprocessMps, mpMap, mlpAddedMPs, keyframeStore());
}
// what KeyFrame::create(const VirtualFrame&) adds after building pKf from a frame extracted into slots 0 / 1 of ctx, and deleteKeyFrame
int onKeyFrameCreated(orbfe_ctx* ctx, KeyFrame::SharedPtr pKf) { return keyframeStore().addFromSlot(ctx, pKf, 0, 0); }
void onKeyFrameDeleted(KeyFrame::SharedPtr pKf) { keyframeStore().erase(pKf); }
void onMapLoaded(KeyFrame::SharedPtr pKf) { keyframeStore().ensureMapping(pKf); }
}  // namespace ORB_SLAM2_ROS2
