// orbfe_loopfuse_dropin.hpp -- the forward fuse ORBMatcher::fuse(pkf, mapPoints, map, bLoop, th) (src/ORBMatcher.cc:682-707) over keyframes
// RESIDENT on the device, every target keyframe in ONE device call (orbfe_fuse_points_into_keyframes_stored, include/orbfe.h).
// with the orbfe::dropin::KeyframeStore<> of section 12,
//     orbfe::dropin::fuseLoopPoints<Camera, Frame>(vConnectedKfs, mvLoopGroupMps, mpMap, store);
// is the whole of `ORBMatcher matcher(0.8, true); for (auto& pKf : vConnectedKfs) matcher.fuse(pKf, mvLoopGroupMps, mpMap, true, 4.0f);`
// in LoopClosing::correctLoop (src/LoopClosing.cc:515-517), and
//     orbfe::dropin::fuse<Camera, Frame>(store, pkf, mapPoints, map, bLoop, th, mfRatio)
// is one ORBMatcher::fuse(pkf, mapPoints, map, bLoop, th), the same call with one keyframe (the forward fuse of
// LocalMapping::fuseMapPoints, src/LocalMapping.cc:399).  Both run on the calling thread's matcherContext(); a failed call throws
// std::runtime_error; a keyframe the store does not hold is inserted on first use.
//
// Why one call is exact: entry (k, j) is a function of point j's position, view direction, distance range and descriptor and of keyframe
// k's pose, bounds and features.  During the loop the poses do not change (correctLoop sets them before), addObservation changes none of
// the point's fields, and MapPoint::replace(keep, drop) recomputes only keep's descriptor, normal and depth (src/MapPoint.cc:229-230).  So
// an entry is used iff point j has not been on either side of a replace since the call (the side that was dropped is bad and is skipped
// anyway); such a point is searched again, with its live arrays, in one further call for that keyframe alone.  Which points a keyframe
// already holds (:687-701) and processFuseMps (:623-663) read the live map, as the reference does.
#pragma once

#include <algorithm>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

#include "orbfe_kfstore_dropin.hpp"

namespace orbfe {
namespace dropin {

namespace loopfuse_detail {

struct Counters {
  long long deviceEntries = 0, reevaluated = 0, extraCalls = 0;
  int nFuse = 0;
};
inline Counters& counters() {
  thread_local Counters c;
  return c;
}

// the arrays of orbfe_sim3_points for the points as they are now; usable: non-null, not bad, in the map (src/ORBMatcher.cc:576)
template <class MapPointPtr>
void pointArrays(const std::vector<MapPointPtr>& mps, orbfe::ORBMatcher::LoopPoints& pts) {
  const size_t m = mps.size();
  pts.usable.assign(m, 0), pts.pos.assign(3 * m, 0.f), pts.viewDir.assign(3 * m, 0.f), pts.maxDist.assign(m, 0.f), pts.minDist.assign(m, 0.f);
  pts.desc.assign(m, orbfe::Descriptor());
  for (size_t i = 0; i < m; ++i) {
    const auto& pMp = mps[i];
    if (!pMp || pMp->isBad() || !pMp->isInMap()) continue;
    pts.usable[i] = 1;
    const cv::Mat Xw = pMp->getPos(), vd = pMp->getViewDirection(), d = pMp->getDesc();
    for (int a = 0; a < 3; ++a) pts.pos[3 * i + a] = Xw.template at<float>(a), pts.viewDir[3 * i + a] = vd.template at<float>(a);
    pMp->getDistance(pts.maxDist[i], pts.minDist[i]);
    std::memcpy(pts.desc[i].data(), d.data, 32);
  }
}

}  // namespace loopfuse_detail

// what the last fuseLoopPoints / fuse(store, ..) of the calling thread did per (keyframe, live point of its vMapPoints): took the entry of
// the one call, or searched the point again; and how many further calls that took (for tests)
inline long long fuseLoopDeviceEntries() { return loopfuse_detail::counters().deviceEntries; }
inline long long fuseLoopReevaluations() { return loopfuse_detail::counters().reevaluated; }
inline long long fuseLoopExtraCalls() { return loopfuse_detail::counters().extraCalls; }
inline int fuseLoopLastCount() { return loopfuse_detail::counters().nFuse; }

// `for (auto& pKf : vConnectedKfs) matcher.fuse(pKf, mvLoopGroupMps, mpMap, bLoop, th);` in the given order -> the sum of the fuses' counts
template <class CameraT, class FrameT, class KeyFramePtr, class MapPointPtr, class MapPtr, class Access>
int fuseLoopPoints(const std::vector<KeyFramePtr>& vConnectedKfs, const std::vector<MapPointPtr>& mvLoopGroupMps, MapPtr mpMap,
                   KeyframeStore<Access>& store, float th = 4.0f, float mfRatio = 0.8f, bool bLoop = true) {
  auto& cnt = loopfuse_detail::counters();
  cnt = loopfuse_detail::Counters();
  const size_t K = vConnectedKfs.size(), m = mvLoopGroupMps.size();
  if (!K || !m) return 0;
  orbfe_ctx* ctx = matcherContext();
  const orbfe::ORBMatcher matcher(mfRatio);
  const orbfe::ORBMatcher::Intrinsics intr = {CameraT::mfFx, CameraT::mfFy, CameraT::mfCx, CameraT::mfCy, 0.f, 0.f, 0.f, 0.f};
  std::vector<float> sf((size_t)store.levels());
  for (size_t l = 0; l < sf.size(); ++l) sf[l] = FrameT::getScaledFactor((int)l);
  auto poseOf = [](const KeyFramePtr& pkf) {
    orbfe_fuse_pose p;
    cv::Mat Rcw, tcw;
    pkf->getPose(Rcw, tcw);
    Bodies::poseFloats(Rcw, tcw, p.Rcw, p.tcw);
    return p;
  };
  // the calls: all of them before the replay starts (more than ORBFE_FUSE_MAX_KF keyframes or ORBFE_FUSE_POINTS_MAX_PAIRS pairs: several)
  orbfe::ORBMatcher::LoopPoints atCall;
  loopfuse_detail::pointArrays(mvLoopGroupMps, atCall);
  const size_t perCall = std::max<size_t>(1, std::min<size_t>(ORBFE_FUSE_MAX_KF, (size_t)ORBFE_FUSE_POINTS_MAX_PAIRS / m));
  std::vector<int32_t> bestIdx(K * m), bestDist(K * m);
  for (size_t k0 = 0; k0 < K; k0 += perCall) {
    const size_t n = std::min(perCall, K - k0);
    std::vector<uint64_t> ids(n);
    std::vector<orbfe_fuse_pose> poses(n);
    for (size_t k = 0; k < n; ++k) {
      store.ensureFeatures(vConnectedKfs[k0 + k]);
      ids[k] = store.id(vConnectedKfs[k0 + k]);
      poses[k] = poseOf(vConnectedKfs[k0 + k]);
    }
    std::vector<int32_t> bi, bd;
    matcher.fusePointsStored(ctx, store.get(), ids, poses, atCall, th, intr, sf, bi, bd);
    std::copy(bi.begin(), bi.end(), bestIdx.begin() + (std::ptrdiff_t)(k0 * m));
    std::copy(bd.begin(), bd.end(), bestDist.begin() + (std::ptrdiff_t)(k0 * m));
  }
  // the replay: per keyframe in order, ORBMatcher::fuse's own steps on the reference's objects
  std::unordered_set<MapPointPtr> changed;  // on either side of a replace since the call
  int nFuse = 0;
  for (size_t k = 0; k < K; ++k) {
    KeyFramePtr pkf1 = vConnectedKfs[k];
    std::set<MapPointPtr> sMapPoints;
    std::vector<MapPointPtr> vMapPoints;
    std::vector<size_t> from;  // vMapPoints[p] = mvLoopGroupMps[from[p]]
    auto fMapPoints = pkf1->getMapPoints();
    for (auto& p : fMapPoints)
      if (p && !p->isBad()) sMapPoints.insert(p);
    for (size_t j = 0; j < m; ++j) {
      if (sMapPoints.find(mvLoopGroupMps[j]) != sMapPoints.end()) continue;
      vMapPoints.push_back(mvLoopGroupMps[j]);
      from.push_back(j);
    }
    auto live = [](const MapPointPtr& p) { return p && !p->isBad() && p->isInMap(); };
    std::vector<MapPointPtr> again;
    std::vector<size_t> againAt;
    for (size_t p = 0; p < vMapPoints.size(); ++p)
      if (live(vMapPoints[p]) && changed.count(vMapPoints[p])) again.push_back(vMapPoints[p]), againAt.push_back(p);
    std::vector<int32_t> freshIdx, freshDist, freshOf(vMapPoints.size(), -1);
    if (!again.empty()) {
      orbfe::ORBMatcher::LoopPoints now;
      loopfuse_detail::pointArrays(again, now);
      matcher.fusePointsStored(ctx, store.get(), std::vector<uint64_t>(1, store.id(pkf1)), std::vector<orbfe_fuse_pose>(1, poseOf(pkf1)), now, th, intr, sf,
                               freshIdx, freshDist);
      for (size_t q = 0; q < againAt.size(); ++q) freshOf[againAt[q]] = (int32_t)q;
      ++cnt.extraCalls;
      cnt.reevaluated += (long long)again.size();
    }
    std::vector<cv::DMatch> matches;
    for (size_t p = 0; p < vMapPoints.size(); ++p) {
      if (!live(vMapPoints[p])) continue;
      int32_t idx, dist;
      if (freshOf[p] >= 0)
        idx = freshIdx[(size_t)freshOf[p]], dist = freshDist[(size_t)freshOf[p]];
      else
        idx = bestIdx[k * m + from[p]], dist = bestDist[k * m + from[p]], ++cnt.deviceEntries;
      if (idx >= 0) matches.push_back(cv::DMatch(idx, (int)p, (float)dist));
    }
    fMapPoints = pkf1->getMapPoints();
    for (const auto& match : matches) {  // a match of two different good points ends in a replace: both count as changed (the dropped one is bad)
      const auto& pMp1 = fMapPoints[(size_t)match.queryIdx];
      const auto& pMp2 = vMapPoints[(size_t)match.trainIdx];
      if (pMp1 && !pMp1->isBad() && pMp2 && !pMp2->isBad() && pMp1 != pMp2) changed.insert(pMp1), changed.insert(pMp2);
    }
    nFuse += Bodies::processFuseMps(matches, fMapPoints, vMapPoints, pkf1, mpMap, bLoop);
  }
  cnt.nFuse = nFuse;
  return nFuse;
}

// int ORBMatcher::fuse(KeyFramePtr pkf1, const std::vector<MapPointPtr>& mapPoints, MapPtr map, bool bLoop, float th) over a stored keyframe
template <class CameraT, class FrameT, class KeyFramePtr, class MapPointPtr, class MapPtr, class Access>
int fuse(KeyframeStore<Access>& store, KeyFramePtr pkf1, const std::vector<MapPointPtr>& mapPoints, MapPtr map, bool bLoop = false, float th = 3.0f,
         float mfRatio = 0.6f) {
  return fuseLoopPoints<CameraT, FrameT>(std::vector<KeyFramePtr>(1, pkf1), mapPoints, map, store, th, mfRatio, bLoop);
}

}  // namespace dropin
}  // namespace orbfe
