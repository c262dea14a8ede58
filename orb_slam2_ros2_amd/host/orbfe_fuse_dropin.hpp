// orbfe_fuse_dropin.hpp -- LocalMapping::fuseMapPoints (src/LocalMapping.cc:352-405) with its inverse fuses as ONE device call
// (orbfe_fuse_into_keyframes, include/orbfe.h).  INTEGRATION.md section 11: the body of LocalMapping::fuseMapPoints becomes
//     orbfe::dropin::fuseMapPoints<Camera, Frame>(mpCurrKeyFrame, mpMap);
// The template selects the target keyframes and map points with the reference's containers (same types, same insertion sequence, so the
// same iteration order), runs the forward fuse through the existing body (orbfe_dropin.hpp: fuse(pkf1, mapPoints, ..)), then replaces the
// loop `for (pkf : sTargetKfs) matcher.fuse(pkf, mpCurrKeyFrame, mpMap)` (ORBMatcher::fuse, searchByProjection with bFuse and
// processFuseMps, src/ORBMatcher.cc:265-347, 623-724) by one batch call on the calling thread's matcherContext() and a sequential replay
// with the reference's own objects, and ends with KeyFrame::updateConnections.  A failed call throws std::runtime_error.
//
// Why the batch is exact: with bFuse the search of (target k, feature i of cur) uses cur's feature position and descriptor only
// (ORBMatcher.cc:297-313), so no MapPoint::replace of an earlier fuse changes it.  Only MapPoint::isInVision reads the map; the batch's
// flag of (k, i) is used iff slot i still holds the point it held at call time and that point has not survived a replace since (its view
// direction is recomputed there, src/MapPoint.cc:229-230); otherwise pMp->isInVision(pkf, ..) is asked, as the reference does.
#pragma once

#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

#include "orbfe_dropin.hpp"

namespace orbfe {
namespace dropin {

namespace fuse_detail {

struct Counters {
  long long deviceFlags = 0, reevaluated = 0;
  int nFuse = 0;  // the fuses of the call: nFuseInv, plus the forward fuse's count after fuseMapPoints
};
inline Counters& counters() {
  thread_local Counters c;
  return c;
}

// tlc.z of searchByProjection(pFrame1, pFrame2, ..) (src/ORBMatcher.cc:270-276), the expression of Bodies::motionDirection:
// twc1 = -Rcw1.t() * tcw1;  tlc = Rcw2 * twc1 + tcw2   (products summed in float, alpha / beta in double)
template <class FramePtr1, class FramePtr2>
float tlcZ(FramePtr1 pFrame1, FramePtr2 pFrame2) {
  cv::Mat Rcw1, tcw1, Rcw2, tcw2;
  pFrame1->getPose(Rcw1, tcw1);
  pFrame2->getPose(Rcw2, tcw2);
  float twc1[3];
  for (int r = 0; r < 3; ++r) {
    const float sm = Rcw1.template at<float>(0, r) * tcw1.template at<float>(0, 0) + Rcw1.template at<float>(1, r) * tcw1.template at<float>(1, 0) +
                     Rcw1.template at<float>(2, r) * tcw1.template at<float>(2, 0);
    twc1[r] = (float)(-1.0 * (double)sm);
  }
  const float sm = Rcw2.template at<float>(2, 0) * twc1[0] + Rcw2.template at<float>(2, 1) * twc1[1] + Rcw2.template at<float>(2, 2) * twc1[2];
  return (float)((double)sm + (double)tcw2.template at<float>(2, 0));
}

struct FlatKf {  // one keyframe's arrays behind an orbfe_fuse_kf
  Bodies::Target t;
  orbfe_fuse_kf kf{};
};
template <class FramePtr>
void flatten(FramePtr f, FlatKf& o, int& n_levels) {
  Bodies::target(f, o.t);
  cv::Mat Rcw, tcw;
  f->getPose(Rcw, tcw);
  Bodies::poseFloats(Rcw, tcw, o.kf.Rcw, o.kf.tcw);
  std::memcpy(o.kf.bounds, o.t.bounds, sizeof o.kf.bounds);
  o.kf.n = (int32_t)o.t.kps.size();
  o.kf.kps = o.t.kps.data();
  o.kf.desc = o.t.desc.empty() ? nullptr : o.t.desc[0].data();
  for (const auto& kp : o.t.kps) n_levels = std::max(n_levels, kp.octave + 1);
}

// The batch call behind fuseIntoKeyframes as an object: prepare() takes the keyframes of one batch and returns the number of pyramid
// levels the scale factors must cover, run() makes the device call.  This one uploads every keyframe's features with the call
// (orbfe_fuse_into_keyframes); orbfe_kfstore_dropin.hpp has the one over keyframes resident in a store.
struct UploadSearch {
  FlatKf fc;
  std::vector<FlatKf> ft;
  std::vector<orbfe_fuse_kf> tk;
  template <class KeyFramePtr>
  int prepare(KeyFramePtr cur, const KeyFramePtr* targets, size_t K) {
    int n_levels = 1;
    ft.assign(K, FlatKf());
    tk.resize(K);
    flatten(cur, fc, n_levels);
    for (size_t k = 0; k < K; ++k) {
      flatten(targets[k], ft[k], n_levels);
      tk[k] = ft[k].kf;
    }
    return n_levels;
  }
  orbfe_status run(orbfe_ctx* ctx, const orbfe_fuse_points* pts, const float* z, const orbfe_camera* cam, float bl, const float* sf, int n_levels,
                   float ratio, int32_t* bestIdx, int32_t* bestDist, uint8_t* visible) {
    return orbfe_fuse_into_keyframes(ctx, &fc.kf, pts, (int32_t)tk.size(), tk.data(), z, cam, bl, sf, n_levels, 3.0f, ratio,
                                     orbfe::ORBMatcher::mnMinThreshold, bestIdx, bestDist, visible);
  }
  static const char* name() { return "orbfe_fuse_into_keyframes"; }
};

}  // namespace fuse_detail

// what the last fuseIntoKeyframes / fuseMapPoints of the calling thread did per (target, live slot): took the batch's visibility flag, or
// asked the live point (for tests)
inline long long fuseDeviceFlagUses() { return fuse_detail::counters().deviceFlags; }
inline long long fuseReevaluations() { return fuse_detail::counters().reevaluated; }
inline int fuseLastCount() { return fuse_detail::counters().nFuse; }

// `for (auto& pkf : targets) nFuseInv += matcher.fuse(pkf, cur, map);` (src/LocalMapping.cc:401-402) in the given order -> nFuseInv
// (search: fuse_detail::UploadSearch or an object of its shape)
template <class CameraT, class FrameT, class KeyFramePtr, class MapPtr, class Search>
int fuseIntoKeyframes(KeyFramePtr cur, const std::vector<KeyFramePtr>& targets, MapPtr map, float mfRatio, Search& search) {
  typedef typename std::decay<decltype(cur->getMapPoints())>::type MapPoints;
  typedef typename MapPoints::value_type MapPointPtr;
  typedef typename std::decay<decltype(*std::declval<MapPointPtr>())>::type MapPointT;
  auto& cnt = fuse_detail::counters();
  cnt = fuse_detail::Counters();
  int nFuseInv = 0;
  for (size_t k0 = 0; k0 < targets.size(); k0 += ORBFE_FUSE_MAX_KF) {  // (the reference collects at most 61; more go in several batches)
    const size_t K = std::min<size_t>(ORBFE_FUSE_MAX_KF, targets.size() - k0);
    const MapPoints atCall = cur->getMapPoints();
    const size_t n = atCall.size();
    if (!n) break;
    const int n_levels = search.prepare(cur, targets.data() + k0, K);
    std::vector<float> z(K);
    for (size_t k = 0; k < K; ++k) z[k] = fuse_detail::tlcZ(targets[k0 + k], cur);
    std::vector<uint8_t> has(n, 0);
    std::vector<float> pos(3 * n, 0.f), view(3 * n, 0.f), mx(n, 0.f), mn(n, 0.f);
    for (size_t i = 0; i < n; ++i) {
      const auto& p = atCall[i];
      if (!p || p->isBad()) continue;
      has[i] = 1;
      const cv::Mat X = p->getPos(), D = p->getViewDirection();
      for (int a = 0; a < 3; ++a) pos[3 * i + a] = X.template at<float>(a), view[3 * i + a] = D.template at<float>(a);
      p->getDistance(mx[i], mn[i]);
    }
    const orbfe_fuse_points pts = {has.data(), pos.data(), view.data(), mx.data(), mn.data()};
    std::vector<float> sf((size_t)n_levels);
    for (int l = 0; l < n_levels; ++l) sf[(size_t)l] = FrameT::getScaledFactor(l);
    orbfe_camera cam{};
    cam.fx = CameraT::mfFx, cam.fy = CameraT::mfFy, cam.cx = CameraT::mfCx, cam.cy = CameraT::mfCy;
    std::vector<int32_t> bestIdx(K * n), bestDist(K * n);
    std::vector<uint8_t> visible(K * n);
    orbfe_ctx* ctx = matcherContext();
    const orbfe_status st = search.run(ctx, &pts, z.data(), &cam, CameraT::mfBl, sf.data(), n_levels, mfRatio, bestIdx.data(), bestDist.data(), visible.data());
    if (st != ORBFE_OK) throw std::runtime_error(std::string(Search::name()) + ": " + orbfe_last_error(ctx));
    // the replay: per target in order, the match list from the live slots, then processFuseMps' policy (src/ORBMatcher.cc:623-663, bLoop
    // false) on the reference's own objects, remembering which point survived a replace
    std::unordered_set<MapPointPtr> survived;
    for (size_t k = 0; k < K; ++k) {
      KeyFramePtr pkf1 = targets[k0 + k];
      auto vMapPoints = cur->getMapPoints();
      std::vector<cv::DMatch> matches;
      for (size_t i = 0; i < n && i < vMapPoints.size(); ++i) {
        const auto& pMp2 = vMapPoints[i];
        if (!pMp2 || pMp2->isBad()) continue;
        bool inVision;
        if (pMp2 == atCall[i] && !survived.count(pMp2)) {
          inVision = visible[k * n + i] != 0;
          ++cnt.deviceFlags;
        } else {
          float vecDistance, cosTheta;
          cv::Point2f uv;
          inVision = pMp2->isInVision(pkf1, vecDistance, uv, cosTheta);
          ++cnt.reevaluated;
        }
        if (inVision && bestIdx[k * n + i] >= 0) matches.emplace_back(bestIdx[k * n + i], (int)i, (float)bestDist[k * n + i]);
      }
      auto fMapPoints = pkf1->getMapPoints();
      for (const auto& match : matches) {
        auto& pMp1 = fMapPoints[(size_t)match.queryIdx];
        auto pMp2 = vMapPoints[(size_t)match.trainIdx];
        if (!pMp2 || pMp2->isBad()) continue;
        if (!pMp1 || pMp1->isBad()) {
          pkf1->setMapPoint(match.queryIdx, pMp2);
          pMp2->addObservation(pkf1, match.queryIdx);
          ++nFuseInv;
        } else {
          if (pMp1 == pMp2) continue;
          const int obs1 = pMp1->getObsNum(), obs2 = pMp2->getObsNum();
          if (obs1 >= obs2) {
            MapPointT::replace(pMp1, pMp2, map);
            survived.insert(pMp1);
          } else {
            MapPointT::replace(pMp2, pMp1, map);
            survived.insert(pMp2);
          }
          ++nFuseInv;
        }
      }
    }
  }
  cnt.nFuse = nFuseInv;
  return nFuseInv;
}

template <class CameraT, class FrameT, class KeyFramePtr, class MapPtr>
int fuseIntoKeyframes(KeyFramePtr cur, const std::vector<KeyFramePtr>& targets, MapPtr map, float mfRatio = 0.6f) {
  fuse_detail::UploadSearch search;
  return fuseIntoKeyframes<CameraT, FrameT>(cur, targets, map, mfRatio, search);
}

// void LocalMapping::fuseMapPoints()  (src/LocalMapping.cc:352-405); search: the batch call of its inverse fuses (see above)
template <class CameraT, class FrameT, class KeyFramePtr, class MapPtr, class Search>
void fuseMapPoints(KeyFramePtr mpCurrKeyFrame, MapPtr mpMap, Search& search) {
  typedef typename std::decay<decltype(mpCurrKeyFrame->getMapPoints())>::type::value_type MapPointPtr;
  typedef typename std::decay<decltype(*mpCurrKeyFrame)>::type KeyFrameT;
  std::unordered_set<KeyFramePtr> sTargetKfs;
  std::unordered_set<MapPointPtr> sTargetMps;
  std::vector<MapPointPtr> vTargetMps;
  sTargetKfs.insert(mpCurrKeyFrame);
  auto connectedKfs = mpCurrKeyFrame->getOrderedConnectedKfs(10);
  for (auto item : connectedKfs) {
    int nNum = 0;
    auto connectedKfs2 = item->getOrderedConnectedKfs(100);
    sTargetKfs.insert(item);
    for (auto pkf : connectedKfs2) {
      if (sTargetKfs.find(pkf) == sTargetKfs.end()) {
        sTargetKfs.insert(pkf);
        ++nNum;
        if (nNum == 5) break;
      }
    }
  }
  for (auto& pkf : sTargetKfs) {
    auto mps = pkf->getMapPoints();
    for (auto& pMp : mps) {
      if (!pMp || pMp->isBad()) continue;
      sTargetMps.insert(pMp);
    }
  }
  std::unordered_set<MapPointPtr> sNoMps;
  auto mps = mpCurrKeyFrame->getMapPoints();
  for (auto& pMp : mps) {
    if (!pMp || pMp->isBad()) continue;
    sNoMps.insert(pMp);
  }
  for (auto& pMp : sTargetMps)
    if (sNoMps.find(pMp) == sNoMps.end()) vTargetMps.push_back(pMp);
  // ORBMatcher matcher(0.6, true);  matcher.fuse(mpCurrKeyFrame, vTargetMps, mpMap): the existing body, unchanged
  const float mfRatio = 0.6f;
  const int nFuse = fuse(mpCurrKeyFrame, vTargetMps, mpMap, false, 3.0f, mfRatio, ORB_SLAM2_ROS2::ORBExtractor::mnLevels);
  const std::vector<KeyFramePtr> targets(sTargetKfs.begin(), sTargetKfs.end());
  fuseIntoKeyframes<CameraT, FrameT>(mpCurrKeyFrame, targets, mpMap, mfRatio, search);
  fuse_detail::counters().nFuse += nFuse;
  KeyFrameT::updateConnections(mpCurrKeyFrame);
}
template <class CameraT, class FrameT, class KeyFramePtr, class MapPtr>
void fuseMapPoints(KeyFramePtr mpCurrKeyFrame, MapPtr mpMap) {
  fuse_detail::UploadSearch search;
  fuseMapPoints<CameraT, FrameT>(mpCurrKeyFrame, mpMap, search);
}

}  // namespace dropin
}  // namespace orbfe
