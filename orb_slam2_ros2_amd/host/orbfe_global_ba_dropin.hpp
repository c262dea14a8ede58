// orbfe_global_ba_dropin.hpp -- Optimizer::globalOptimization (src/Optimizer.cc:934-1043) with the device global bundle adjustment
// (orbfe_ba_global_optimize) in the place of g2o: the function's whole body.
//
//   void Optimizer::globalOptimization(const std::vector<KeyFramePtr>& vpKfs, const std::vector<MapPointPtr>& vpMps, int nIteration,
//                                      bool* bStopFlag, bool bUseRk) {
//     orbfe::dropin::globalOptimization<Camera>(vpKfs, vpMps, nIteration, bStopFlag, bUseRk);
//   }
//
// What stays on the host is map state: which keyframes and map points become vertices (:946-976; null and bad ones are skipped, a
// keyframe vertex is fixed iff its id is 0), the edges in vpMps order and, within a map point, getObservation() order (:977-1028;
// observers that are gone, bad or no vertex are skipped; stereo iff rightU > 0; information getScaledFactorInv2(octave) for BOTH edge
// kinds -- the local BA's mono edges use getScaledFactorInv, this function does not; Huber deltas only with bUseRk), and the write-back
// into mTcwGBA / mPGBA of every vertex and nowhere else (:1031-1043).  A map point none of whose observations is usable is still a
// vertex: it comes back where it was.  buildGlobalGraph is everything up to the optimisation; the device call runs on solverContext(2)
// (the LoopClosing thread's, which is where the reference starts the global BA).
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#include <opencv2/core.hpp>

#include "orbfe_dropin.hpp"

namespace orbfe {
namespace dropin {

// the graph as orbfe_ba_global_optimize takes it, with the vertices' owners for the write-back
template <class KeyFramePtr, class MapPointPtr>
struct GlobalGraph {
  std::vector<KeyFramePtr> frames;      // [n_poses] vertex order: vpKfs order
  std::vector<MapPointPtr> landmarks;   // [n_points] vpMps order
  std::vector<uint8_t> fixed;           // [n_poses]
  std::vector<double> poses, points;    // [n_poses][7], [n_points][3]
  std::vector<int32_t> edgePose, edgePoint;
  std::vector<double> meas, info, huber;  // [n_edges][3], [n_edges], [n_edges] (-1: no kernel)
  std::vector<uint8_t> isStereo;
  template <class CameraT>
  orbfe_ba_problem problem() const {
    orbfe_ba_problem prob{};
    prob.n_poses = (int32_t)frames.size(), prob.n_points = (int32_t)landmarks.size(), prob.n_edges = (int32_t)edgePose.size();
    prob.poses = poses.data(), prob.points = points.data(), prob.edge_pose = edgePose.data(), prob.edge_point = edgePoint.data();
    prob.meas = meas.data(), prob.is_stereo = isStereo.data(), prob.info = info.data(), prob.huber_delta = huber.data();
    prob.fx = CameraT::mfFx, prob.fy = CameraT::mfFy, prob.cx = CameraT::mfCx, prob.cy = CameraT::mfCy, prob.bf = CameraT::mfBf;
    return prob;
  }
};

// :946-1028: the vertices and the edges
template <class KeyFramePtr, class MapPointPtr>
GlobalGraph<KeyFramePtr, MapPointPtr> buildGlobalGraph(const std::vector<KeyFramePtr>& vpKfs, const std::vector<MapPointPtr>& vpMps, bool bUseRk) {
  using KeyFrameT = typename KeyFramePtr::element_type;
  using MapPointT = typename MapPointPtr::element_type;
  GlobalGraph<KeyFramePtr, MapPointPtr> G;
  std::map<const KeyFrameT*, int32_t> vertexOf;
  for (const auto& pkf : vpKfs) {
    if (!pkf || pkf->isBad() || vertexOf.count(pkf.get())) continue;
    cv::Mat Rcw, tcw;
    pkf->getPose(Rcw, tcw);
    double p[7];
    matToPose(Rcw, tcw, p);  // Converter::ConvertTcw2SE3
    G.poses.insert(G.poses.end(), p, p + 7);
    G.fixed.push_back(pkf->getID() == 0 ? 1 : 0);
    vertexOf[pkf.get()] = (int32_t)G.frames.size();
    G.frames.push_back(pkf);
  }
  std::map<const MapPointT*, int32_t> landmarkOf;
  for (const auto& pMp : vpMps) {
    if (!pMp || pMp->isBad() || landmarkOf.count(pMp.get())) continue;
    const int32_t pv = (int32_t)G.landmarks.size();
    landmarkOf[pMp.get()] = pv;
    G.landmarks.push_back(pMp);
    const cv::Mat pos = pMp->getPos();
    for (int a = 0; a < 3; ++a) G.points.push_back((double)pos.template at<float>(a));  // Converter::ConvertPw2Vector3
    auto mObservations = pMp->getObservation();
    for (auto& obs : mObservations) {
      auto pKf = obs.first.lock();
      if (!pKf || pKf->isBad()) continue;
      auto it = vertexOf.find(pKf.get());
      if (it == vertexOf.end()) continue;
      const auto& kp = pKf->getLeftKeyPoint(obs.second);
      const double rightU = pKf->getRightU(obs.second);
      const bool stereo = rightU > 0;
      G.edgePose.push_back(it->second), G.edgePoint.push_back(pv);
      G.meas.push_back((double)kp.pt.x), G.meas.push_back((double)kp.pt.y), G.meas.push_back(stereo ? rightU : 0.0);
      G.isStereo.push_back(stereo ? 1 : 0);
      G.info.push_back((double)pKf->getScaledFactorInv2(kp.octave));  // both edge kinds (:994, :1013)
      G.huber.push_back(bUseRk ? (double)(stereo ? Optimizer::deltaStereo : Optimizer::deltaMono) : -1.0);
    }
  }
  return G;
}

// the whole body of Optimizer::globalOptimization
template <class CameraT, class KeyFramePtr, class MapPointPtr>
void globalOptimization(const std::vector<KeyFramePtr>& vpKfs, const std::vector<MapPointPtr>& vpMps, int nIteration, bool* bStopFlag,
                        bool bUseRk = false) {
  const auto G = buildGlobalGraph(vpKfs, vpMps, bUseRk);
  const orbfe_ba_problem prob = G.template problem<CameraT>();
  const Optimizer::GlobalResult r = Optimizer::globalOptimization(solverContext(2), prob, G.fixed, nIteration, (const volatile bool*)bStopFlag);
  for (std::size_t v = 0; v < G.frames.size(); ++v) G.frames[v]->mTcwGBA = poseToMat(r.poses.data() + v * 7);  // Converter::ConvertSE32Tcw
  for (std::size_t p = 0; p < G.landmarks.size(); ++p) {
    cv::Mat pos(3, 1, CV_32F);  // Converter::ConvertVector32Pw
    for (int a = 0; a < 3; ++a) pos.template at<float>(a) = (float)r.points[p * 3 + a];
    G.landmarks[p]->mPGBA = pos;
  }
}

}  // namespace dropin
}  // namespace orbfe
