// orbfe_motion_dropin.hpp -- Tracking::trackMotionModel over two frame slots and a map-point store (orbfe_track_motion_model_slots,
// include/orbfe.h).  INTEGRATION.md section 23: with the orbfe::dropin::MapPointStore<> of section 22,
//     bool Tracking::trackMotionModel() {
//       mpLastFrame->setPose(mTlr * mpLastFrame->getRefKF()->getPose());          // processLastFrame, src/Tracking.cc:689
//       mpCurrFrame->setPose(mVelocity * mpLastFrame->getPose());                  // :385
//       return orbfe::dropin::trackMotionModel<Camera>(mpCurrFrame, mpLastFrame, store, mvpTempMappoints);
//     }
// The call stands for Frame::unProject of the last frame (the temporary points end in mvpTempMappoints and in the last frame, as
// processLastFrame leaves them), the two searchByProjection, OptimizePoseOnly and the isInMap count, with every side effect on the
// reference's objects replayed in the reference's order (Bodies::trackMotionModelSlots, orbfe_dropin.hpp).
#pragma once

#include "orbfe_mpstore_dropin.hpp"

namespace orbfe {
namespace dropin {

template <class CameraT, class Access, class FramePtr1, class FramePtr2, class MapPointPtr>
bool trackMotionModel(FramePtr1 mpCurrFrame, FramePtr2 mpLastFrame, MapPointStore<Access>& store, std::vector<MapPointPtr>& mvpTempMappoints,
                      float mfRatio = 0.9f) {
  return Bodies::template trackMotionModelSlots<CameraT>(store, mpCurrFrame, mpLastFrame, mvpTempMappoints, mfRatio);
}

}  // namespace dropin
}  // namespace orbfe
