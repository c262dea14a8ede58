// orbfe_essential_dropin.hpp -- Optimizer::optimizeEssentialGraph (src/Optimizer.cc:746-920) with the device pose-graph optimiser
// (orbfe_pose_graph_optimize) in the place of g2o: the function's whole body in the reference's own order and arithmetic
// (rule G9).
//
//   void Optimizer::optimizeEssentialGraph(const LoopConnection& mLoopConnections, MapPtr mpMap, KeyFramePtr pLoopKf, KeyFramePtr pCurrKf,
//                                          const int& graphTh, const KeyFrameAndSim3& mCorrectedG2oScw,
//                                          const KeyFrameAndSim3& mNoCorrectedG2oScw, bool bFixScale) {
//     orbfe::dropin::optimizeEssentialGraph<Sim3Ret>(mLoopConnections, mpMap, pLoopKf, pCurrKf, graphTh, mCorrectedG2oScw, mNoCorrectedG2oScw,
//                                                    bFixScale);
//   }
//
// What stays on the host is map state: which keyframes become vertices and with which Sim3 (:767-797), the three edge sources with the
// graphTh and sAlreadyConnected rules and the measurements S2w * Sw1 in double (:804-877), the normalisation by vertex 0's inverse and
// setPose(R, t / s) (:882-894), the map-point correction with the reference's own Sim3Ret arithmetic, setPos, updateDescriptor and
// updateNormalAndDepth (:897-918).  buildEssentialGraph is everything up to the optimisation, applyEssentialGraph everything after it;
// the device call sits between them, on solverContext(2) (the LoopClosing thread's).
// A free scale is not on the device: bFixScale == false throws std::invalid_argument, and so does any Sim3 whose mfS is not 1.  The
// reference dereferences vpSim3Vertexes[0]; with no good keyframe of id 0 this throws std::runtime_error instead.
// Needs the project's csrc directory on the include path for the group arithmetic (sim3_edge_dev.h: host + device, no HIP needed).
#pragma once

#include <cstddef>
#include <cstdint>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include <opencv2/core.hpp>

#include "../csrc/sim3_edge_dev.h"
#include "orbfe_dropin.hpp"

namespace orbfe {
namespace dropin {

// the graph as orbfe_pose_graph_optimize takes it, with what the write-back needs; vertex v is the keyframe of id ids[v]
template <class KeyFramePtr, class Sim3RetT>
struct EssentialGraph {
  std::vector<std::size_t> ids;       // [nv] keyframe id of every vertex, ascending order of getAllKeyFrames()
  std::vector<int32_t> vertexOfId;    // [nMaxID + 1] vertex of a keyframe id, -1: none
  std::vector<KeyFramePtr> keyFrames; // [nMaxID + 1] vKeyFrames
  std::vector<Sim3RetT> vScw;         // [nMaxID + 1] the Sim3 before the optimisation (:770)
  std::vector<double> estimates;      // [nv][8]
  std::vector<uint8_t> fixed;         // [nv]
  std::vector<int32_t> v0, v1;        // [ne]
  std::vector<double> meas;           // [ne][8]
};

// Converter::ConvertSim3G2o (rule G2 = O2 of DESIGN 4.22)
template <class Sim3RetT>
inline Sim3Dev essentialSim3(const Sim3RetT& S) {
  if (S.mfS != 1.0f) throw std::invalid_argument("optimizeEssentialGraph: only fixed-scale Sim3 (mfS == 1) are on the device");
  float model[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) model[3 * r + c] = S.mRqp.template at<float>(r, c);
    model[9 + r] = S.mtqp.template at<float>(r);
  }
  Sim3Dev out;
  sim3_from_model(model, out);
  return out;
}

inline void essentialPush(std::vector<double>& to, const Sim3Dev& S) {
  to.insert(to.end(), S.q, S.q + 4);
  to.insert(to.end(), S.t, S.t + 3);
  to.push_back(S.s);
}

// :758-877: the vertices and the edges
template <class Sim3RetT, class LoopConnectionT, class MapPtr, class KeyFramePtr, class KeyFrameAndSim3T>
EssentialGraph<KeyFramePtr, Sim3RetT> buildEssentialGraph(const LoopConnectionT& mLoopConnections, MapPtr mpMap, KeyFramePtr pLoopKf,
                                                           KeyFramePtr pCurrKf, const int& graphTh, const KeyFrameAndSim3T& mCorrectedG2oScw,
                                                           const KeyFrameAndSim3T& mNoCorrectedG2oScw, bool bFixScale = true) {
  using KeyFrameT = typename KeyFramePtr::element_type;
  if (!bFixScale) throw std::invalid_argument("optimizeEssentialGraph: only the fixed-scale optimisation is on the device");
  EssentialGraph<KeyFramePtr, Sim3RetT> G;
  const std::size_t nMaxID = KeyFrameT::getMaxID();
  auto vAllKeyFrames = mpMap->getAllKeyFrames();
  G.keyFrames.assign(nMaxID + 1, nullptr);
  G.vScw.resize(nMaxID + 1);
  G.vertexOfId.assign(nMaxID + 1, -1);
  std::vector<Sim3Dev> vScwg(nMaxID + 1);
  for (auto& pKf : vAllKeyFrames) {
    if (!pKf || pKf->isBad()) continue;
    const std::size_t vID = pKf->getID();
    G.keyFrames[vID] = pKf;
    Sim3RetT Siw;
    auto it = mCorrectedG2oScw.find(pKf);
    if (it != mCorrectedG2oScw.end()) {
      Siw = it->second;
    } else {
      cv::Mat Rcw, tcw;
      pKf->getPose(Rcw, tcw);
      Siw = Sim3RetT(Rcw, tcw, 1.f);
    }
    const Sim3Dev Siwg = essentialSim3(Siw);
    vScwg[vID] = Siwg;
    G.vScw[vID] = Siw;
    G.vertexOfId[vID] = (int32_t)G.ids.size();
    G.ids.push_back(vID);
    essentialPush(G.estimates, Siwg);
    G.fixed.push_back(vID == (std::size_t)pLoopKf->getID() ? 1 : 0);
  }
  auto addEdge = [&](std::size_t id1, std::size_t id2, const Sim3Dev& S2w, const Sim3Dev& Sw1) {
    Sim3Dev S21;
    sim3_mul(S2w, Sw1, S21);
    G.v0.push_back(G.vertexOfId[id1]);
    G.v1.push_back(G.vertexOfId[id2]);
    essentialPush(G.meas, S21);
  };
  std::set<std::pair<std::size_t, std::size_t>> sAlreadyConnected;
  for (const auto& c : mLoopConnections) {  // :804-833 the new covisibility the loop closure produced
    auto pkf1 = c.first;
    const std::size_t id1 = pkf1->getID();
    Sim3Dev Sw1;
    sim3_inverse(vScwg[id1], Sw1);
    for (auto& pkf2 : c.second) {
      if (!pkf2 || pkf2->isBad()) continue;
      const int weight = pkf1->getWeight(pkf2);
      if ((pkf1 != pCurrKf || pkf2 != pLoopKf) && weight < graphTh) continue;
      const std::size_t id2 = pkf2->getID();
      addEdge(id1, id2, vScwg[id2], Sw1);
      sAlreadyConnected.insert({id1, id2});
    }
  }
  for (std::size_t id1 = 0; id1 <= nMaxID; ++id1) {  // :836-877 spanning tree, loop edges, covisibility of weight >= 100
    auto& pkf1 = G.keyFrames[id1];
    if (!pkf1 || pkf1->isBad()) continue;
    auto pEdgesKFs = pkf1->getLoopEdges();
    Sim3Dev Sw1;
    auto n1 = mNoCorrectedG2oScw.find(pkf1);
    if (n1 != mNoCorrectedG2oScw.end())
      sim3_inverse(essentialSim3(n1->second), Sw1);
    else
      sim3_inverse(vScwg[id1], Sw1);
    auto parent = pkf1->getParent().lock();
    if (parent && !parent->isBad()) pEdgesKFs.push_back(parent);
    auto vEssentialKFs = pkf1->getConnectedKfs(100);
    for (auto& k : vEssentialKFs) pEdgesKFs.push_back(k);
    for (auto& pkf2 : pEdgesKFs) {
      const std::size_t id2 = pkf2->getID();
      const auto pair12 = std::make_pair(id1, id2);
      if (sAlreadyConnected.find(pair12) != sAlreadyConnected.end()) continue;
      sAlreadyConnected.insert(pair12);
      auto n2 = mNoCorrectedG2oScw.find(pkf2);
      addEdge(id1, id2, n2 != mNoCorrectedG2oScw.end() ? essentialSim3(n2->second) : vScwg[id2], Sw1);
    }
  }
  for (std::size_t e = 0; e < G.v0.size(); ++e)
    if (G.v0[e] < 0 || G.v1[e] < 0) throw std::runtime_error("optimizeEssentialGraph: an edge names a keyframe that is no vertex (bad or not in the map)");
  return G;
}

// :882-919: the poses and the map points from the optimised estimates ([nv][8])
template <class Sim3RetT, class MapPtr, class KeyFramePtr>
void applyEssentialGraph(const EssentialGraph<KeyFramePtr, Sim3RetT>& G, const std::vector<double>& estimates, MapPtr mpMap,
                         KeyFramePtr pCurrKf) {
  auto estimateOf = [&](int32_t v) {
    Sim3Dev S;
    const double* p = estimates.data() + 8 * (std::size_t)v;
    for (int k = 0; k < 4; ++k) S.q[k] = p[k];
    for (int k = 0; k < 3; ++k) S.t[k] = p[4 + k];
    S.s = p[7];
    return S;
  };
  if (G.vertexOfId.empty() || G.vertexOfId[0] < 0)
    throw std::runtime_error("optimizeEssentialGraph: no good keyframe of id 0 (the reference normalises by vertex 0)");
  Sim3Dev g2oSwc0;
  sim3_inverse(estimateOf(G.vertexOfId[0]), g2oSwc0);
  std::vector<Sim3RetT> vG2oSwc(G.vertexOfId.size());
  for (std::size_t idx = 0; idx < G.vertexOfId.size(); ++idx) {
    if (G.vertexOfId[idx] < 0) continue;
    Sim3Dev prod;
    sim3_mul(estimateOf(G.vertexOfId[idx]), g2oSwc0, prod);
    float model[12];
    sim3_to_model(prod, model);  // Converter::ConvertG2o2Sim3
    cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R.template at<float>(r, c) = model[3 * r + c];
      t.template at<float>(r) = model[9 + r];
    }
    const Sim3RetT Scw(R, t, (float)prod.s);
    vG2oSwc[idx] = Scw.inv();
    G.keyFrames[idx]->setPose(Scw.mRqp, Scw.mtqp / Scw.mfS);
  }
  auto vAllMapPoints = mpMap->getAllMapPoints();
  for (const auto& pMp : vAllMapPoints) {
    if (!pMp || pMp->isBad()) continue;
    KeyFramePtr pCorrectKF;
    if (pMp->getLoopKF() == pCurrKf) {
      pCorrectKF = pMp->getLoopRefKF();
      pMp->setLoopRefKF(nullptr);
    } else
      pCorrectKF = pMp->getRefKF();
    if (!pCorrectKF || pCorrectKF->isBad()) continue;
    cv::Mat p3dW = pMp->getPos();
    const std::size_t kfID = pCorrectKF->getID();
    cv::Mat correctedP3dW = vG2oSwc[kfID] * (G.vScw[kfID] * p3dW);
    pMp->setPos(correctedP3dW);
    pMp->updateDescriptor();
    pMp->updateNormalAndDepth();
  }
  mpMap->setUpdate(true);
}

// the whole body of Optimizer::optimizeEssentialGraph
template <class Sim3RetT, class LoopConnectionT, class MapPtr, class KeyFramePtr, class KeyFrameAndSim3T>
void optimizeEssentialGraph(const LoopConnectionT& mLoopConnections, MapPtr mpMap, KeyFramePtr pLoopKf, KeyFramePtr pCurrKf, const int& graphTh,
                            const KeyFrameAndSim3T& mCorrectedG2oScw, const KeyFrameAndSim3T& mNoCorrectedG2oScw, bool bFixScale = true) {
  auto G = buildEssentialGraph<Sim3RetT>(mLoopConnections, mpMap, pLoopKf, pCurrKf, graphTh, mCorrectedG2oScw, mNoCorrectedG2oScw, bFixScale);
  if (G.vertexOfId.empty() || G.vertexOfId[0] < 0)
    throw std::runtime_error("optimizeEssentialGraph: no good keyframe of id 0 (the reference normalises by vertex 0)");
  std::vector<double> estimates = G.estimates;
  // solver 0: dense on a small map, the block-sparse Cholesky otherwise -- no bound on the keyframes (orbfe_pose_graph_optimize_ex)
  orbfe::Optimizer::optimizeEssentialGraph(solverContext(2), estimates, G.fixed, G.v0, G.v1, G.meas, 20, nullptr, 0);
  applyEssentialGraph<Sim3RetT>(G, estimates, mpMap, pCurrKf);
}

}  // namespace dropin
}  // namespace orbfe
