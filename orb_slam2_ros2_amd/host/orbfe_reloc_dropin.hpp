// orbfe_reloc_dropin.hpp -- ORBMatcher::searchByBow of ONE frame against MANY keyframes resident on the device
// (orbfe_search_by_bow_stored, include/orbfe.h), and the two loops of the reference that are such a search:
//     Tracking::filterKFByBow          (src/Tracking.cc:446-490)      searchByBow(mpCurrFrame, pkf, matches) per relocalisation candidate
//     LoopClosing::computeSim3, loop 1 (src/LoopClosing.cc:308-326)   searchByBow(mpCurrKeyFrame, pKfCandidate, matches, false, true) per loop candidate
// with the orbfe::dropin::KeyframeStore<> of section 12,
//     return orbfe::dropin::filterKFByBow<PnPSolver>(store, mpCurrFrame, relocBowParam, vbDiscard, candidateNum, vpCandidateKFs);
//     int nCandidates = orbfe::dropin::sim3Candidates<Sim3Solver>(store, mpCurrKeyFrame, mvEnoughKfs, vbDiscard, vpSolvers, vvMatches);
// Both stand on
//     orbfe::dropin::searchByBow(store, pFrame, candidates, allMatches, bAddMPs, bLoop, mfRatio, mbCheckOri [, queryStored])
// which gives, per candidate, the std::vector<cv::DMatch> the reference's searchByBow (src/ORBMatcher.cc:170-253) leaves -- ONE device
// call per 64 candidates instead of one per candidate.  A candidate the store does not hold yet is inserted from its host arrays on
// first use (KeyframeStore::ensureBow).  A Frame goes up as arrays; a current KEYFRAME (queryStored) is named by its id.
// At the end of the file, INTEGRATION.md section 16: both ORBMatcher::searchBySim3 overloads over the same store
// (orbfe_search_by_sim3_stored / orbfe_search_by_sim3_points_stored),
//     orbfe::dropin::searchBySim3<Camera>(store, mpCurr, mpMatch, matches, g2oScm, th, mfRatio)
//     orbfe::dropin::searchBySim3<Camera>(store, pCurr, vLoopGroupMps, vMatchedMps, g2oScw, th, mfRatio)
// what follows a successful iterate in Tracking::trackReLocalize (src/Tracking.cc:565-584) as one device call
// (orbfe_reloc_refine_stored),
//     if (orbfe::dropin::relocRefine<Camera>(store, mpCurrFrame, vpCandidateKFs[idx], relocBowParam, idx, vInliers, modelReti.mRcw, modelReti.mtcw))
// the whole body of Tracking::trackReference (src/Tracking.cc:360-371) as one device call
// (orbfe_track_reference_stored),
//     return orbfe::dropin::trackReference<Camera>(store, mpVoc, mpCurrFrame, mpRefKf);
#pragma once

#include <algorithm>
#include <map>
#include <set>

#include "orbfe_kfstore_dropin.hpp"

namespace orbfe {
namespace dropin {

namespace bow_detail {

template <class MapPoints>
inline void flagsOf(const MapPoints& mps, std::vector<uint8_t>& f) {
  f.assign(mps.size(), 0);
  for (size_t i = 0; i < mps.size(); ++i) {
    const bool good = mps[i] && !mps[i]->isBad();
    f[i] = (uint8_t)((good ? ORBFE_TRI_GOOD : 0) | (good && mps[i]->isInMap() ? ORBFE_TRI_INMAP : 0));
  }
}

}  // namespace bow_detail

// The matches of pFrame against every candidate: allMatches[k] is what searchByBow(pFrame, candidates[k], matches, bAddMPs, bLoop) of an
// ORBMatcher(mfRatio, mbCheckOri) leaves in `matches`; returns nothing else (nMatches of candidate k is allMatches[k].size()).
//   !bAddMPs && !bLoop (tracking): the frame is searched with NO map points -- the caller's setMapPointsNull() before every candidate
//   (Tracking.cc:460) -- and the side effects are replayed for every candidate in order: setMapPointsNull(), then setMapPoints
//   (addMatchInTrack on every matched good point, the frame's slots set; ORBMatcher.cc:815-830).  The frame ends as the reference's
//   loop leaves it: with the last candidate's points.
//   bAddMPs: both sides' map state goes up as it is at the call (no side effects in the reference either).
// Candidates must be non-null; bad ones are the caller's to skip (both bodies below do).  queryStored: pFrame is a keyframe of the store
// (inserted on first use) and is named by id; else its descriptors, angles and FeatureVector go up with the call.
template <class FramePtr, class KeyFramePtr, class Access>
void searchByBow(KeyframeStore<Access>& store, FramePtr pFrame, const std::vector<KeyFramePtr>& candidates,
                 std::vector<std::vector<cv::DMatch>>& allMatches, bool bAddMPs, bool bLoop, float mfRatio = 0.6f, bool mbCheckOri = true,
                 bool queryStored = false) {
  const size_t K = candidates.size();
  allMatches.assign(K, std::vector<cv::DMatch>());
  if (K == 0) return;
  const int32_t mode = bAddMPs ? ORBFE_BOW_ADD : bLoop ? ORBFE_BOW_LOOP : ORBFE_BOW_TRACK;
  pFrame->computeBow();
  const auto& kpsF = pFrame->getLeftKeyPoints();
  const size_t n = kpsF.size();
  // the query
  orbfe_bow_query q = orbfe_bow_query();
  std::vector<uint8_t> desc, qFlags;
  std::vector<float> angle;
  std::vector<uint32_t> nodes, features;
  std::vector<int32_t> offsets(1, 0);
  q.n = (int32_t)n;
  if (queryStored) {
    store.ensureBow(pFrame);
    q.from_store = 1;
    q.id = store.id(pFrame);
  } else {
    const auto& descF = pFrame->getDescriptor();
    desc.resize(n * 32);
    angle.resize(n);
    for (size_t i = 0; i < n; ++i) {
      std::memcpy(&desc[32 * i], descF[i].data, 32);
      angle[i] = kpsF[i].angle;
    }
    for (const auto& node : Bodies::featVec(pFrame)) {  // DBoW3::FeatureVector: ascending node ids, feature ids in insertion order
      nodes.push_back((uint32_t)node.first);
      for (const auto f : node.second) features.push_back((uint32_t)f);
      offsets.push_back((int32_t)features.size());
    }
    q.desc = desc.data(), q.angle = angle.data();
    q.n_nodes = (int32_t)nodes.size(), q.nodes = nodes.data(), q.node_offsets = offsets.data(), q.features = features.data();
  }
  if (mode == ORBFE_BOW_ADD) {
    bow_detail::flagsOf(pFrame->getMapPoints(), qFlags);
    q.flags = qFlags.data();
  }  // (tracking: all 0 = setMapPointsNull(); loop: no filter reads them)
  orbfe_ctx* ctx = matcherContext();
  for (size_t k0 = 0; k0 < K; k0 += ORBFE_BOW_SEARCH_MAX_KF) {
    const size_t kn = std::min<size_t>(ORBFE_BOW_SEARCH_MAX_KF, K - k0);
    std::vector<uint64_t> ids(kn);
    std::vector<std::vector<uint8_t>> flags(kn);
    std::vector<const uint8_t*> flagPtrs(kn, nullptr);
    std::vector<decltype(candidates[0]->getMapPoints())> mapPointsKF(kn);
    int64_t cap = 0;
    for (size_t k = 0; k < kn; ++k) {
      const auto& pkf = candidates[k0 + k];
      store.ensureBow(pkf);
      ids[k] = store.id(pkf);
      orbfe_kfstore_info info;
      store.info(pkf, &info);
      cap += info.n_bow_features;  // a match per FeatureVector entry at most
      mapPointsKF[k] = pkf->getMapPoints();
      if (mode != ORBFE_BOW_LOOP) {
        bow_detail::flagsOf(mapPointsKF[k], flags[k]);
        flagPtrs[k] = flags[k].data();
      }
    }
    std::vector<orbfe_bow_match> found((size_t)std::max<int64_t>(cap, 1));
    std::vector<int64_t> off(kn + 1, 0);
    orbfe::check(ctx, orbfe_search_by_bow_stored(ctx, store.get(), &q, (int32_t)kn, ids.data(), flagPtrs.data(), mode, mfRatio,
                                          orbfe::ORBMatcher::mnMinThreshold, mbCheckOri ? 1 : 0, found.data(), cap, off.data()));
    for (size_t k = 0; k < kn; ++k) {
      std::vector<cv::DMatch>& matches = allMatches[k0 + k];
      for (int64_t i = off[k]; i < off[k + 1]; ++i) matches.emplace_back(found[(size_t)i].query, found[(size_t)i].train, (float)found[(size_t)i].distance);
      if (mode == ORBFE_BOW_TRACK) {
        pFrame->setMapPointsNull();
        Bodies::setMapPoints(Bodies::mapPointSlots(pFrame), mapPointsKF[k], matches);
      }
    }
  }
}

// int Tracking::filterKFByBow(RelocBowParam&, std::vector<bool>& vbDiscard, const int& candidateNum, std::vector<KeyFrame::SharedPtr>&)
// (src/Tracking.cc:446-490): the searchByBow of every good candidate in one call, then the reference's per-candidate tail unchanged
template <class PnPSolverT, class RelocBowParamT, class FramePtr, class KeyFramePtr, class Access>
int filterKFByBow(KeyframeStore<Access>& store, FramePtr mpCurrFrame, RelocBowParamT& relocBowParam, std::vector<bool>& vbDiscard, const int& candidateNum,
                  std::vector<KeyFramePtr>& vpCandidateKFs) {
  std::vector<KeyFramePtr> good;
  std::vector<std::size_t> goodIdx;
  for (std::size_t idx = 0; idx < (std::size_t)candidateNum; ++idx) {
    KeyFramePtr pkf = vpCandidateKFs[idx];
    if (!pkf || pkf->isBad()) {
      vbDiscard[idx] = true;
      continue;
    }
    good.push_back(pkf), goodIdx.push_back(idx);
  }
  std::vector<std::vector<cv::DMatch>> allMatches;
  searchByBow(store, mpCurrFrame, good, allMatches, false, false, 0.75f, true);
  int nCandidates = 0;
  for (std::size_t g = 0; g < good.size(); ++g) {
    const std::size_t idx = goodIdx[g];
    const std::vector<cv::DMatch>& matches = allMatches[g];
    relocBowParam.mvAllMatches[idx] = matches;
    if ((int)matches.size() < 10) {
      vbDiscard[idx] = true;
      continue;
    }
    std::vector<cv::Mat> mapPoints;
    std::vector<cv::KeyPoint> ORBPoints;
    const auto& allORBPoints = mpCurrFrame->getLeftKeyPoints();
    const auto allMapPoints = good[g]->getMapPoints();
    std::size_t pnpIdx = 0;
    for (std::size_t jdx = 0; jdx < matches.size(); ++jdx) {
      const auto& match = matches[jdx];
      const auto& pMp = allMapPoints[match.trainIdx];
      if (!pMp || pMp->isBad()) continue;
      ORBPoints.push_back(allORBPoints[match.queryIdx]);
      mapPoints.push_back(pMp->getPos().clone());
      relocBowParam.mvPnPId2MatchID[idx][pnpIdx] = jdx;
      ++pnpIdx;
    }
    relocBowParam.mvpSolvers[idx] = PnPSolverT::create(mapPoints, ORBPoints);
    ++nCandidates;
  }
  return nCandidates;
}

// The first loop of bool LoopClosing::computeSim3(Sim3Ret&, Sim3Ret&, KeyFramePtr&) (src/LoopClosing.cc:302-342): vbDiscard, vpSolvers and
// vvMatches sized n by the caller as the reference sizes them; returns nCandidates.  The current keyframe is named by its id.
template <class Sim3SolverT, class KeyFramePtr, class SolverPtr, class Access>
int sim3Candidates(KeyframeStore<Access>& store, KeyFramePtr mpCurrKeyFrame, const std::vector<KeyFramePtr>& mvEnoughKfs, std::vector<bool>& vbDiscard,
                   std::vector<SolverPtr>& vpSolvers, std::vector<std::vector<cv::DMatch>>& vvMatches) {
  const std::size_t n = mvEnoughKfs.size();
  int nCandidates = (int)n;
  std::vector<KeyFramePtr> good;
  std::vector<std::size_t> goodIdx;
  for (std::size_t idx = 0; idx < n; ++idx) {
    auto pKfCandidate = mvEnoughKfs[idx];
    if (!pKfCandidate || pKfCandidate->isBad()) {
      vbDiscard[idx] = true;
      --nCandidates;
      continue;
    }
    good.push_back(pKfCandidate), goodIdx.push_back(idx);
  }
  std::vector<std::vector<cv::DMatch>> allMatches;
  searchByBow(store, mpCurrKeyFrame, good, allMatches, false, true, 0.75f, true, true);
  for (std::size_t g = 0; g < good.size(); ++g) {
    const std::size_t idx = goodIdx[g];
    const std::vector<cv::DMatch>& matches = allMatches[g];
    if ((int)matches.size() < 20) {
      vbDiscard[idx] = true;
      --nCandidates;
      continue;
    }
    std::vector<bool> vbChoose(matches.size(), true);
    vpSolvers[idx] = Sim3SolverT::create(good[g], mpCurrKeyFrame, matches, vbChoose);
    int nChoose = 0;
    for (std::size_t jdx = 0; jdx < vbChoose.size(); ++jdx)
      if (vbChoose[jdx]) {
        vvMatches[idx].push_back(matches[jdx]);
        ++nChoose;
      }
    if (nChoose < 20) {
      vbDiscard[idx] = true;
      --nCandidates;
    }
  }
  return nCandidates;
}

// ---- ORBMatcher::searchBySim3 over stored keyframes (orbfe_search_by_sim3_stored / _points_stored) ----
namespace sim3_detail {

// the map state of a keyframe's n features (the part of Bodies::keyFrameView the stored call reads)
template <class KeyFramePtr>
inline void mapState(KeyFramePtr kf, size_t n, orbfe::ORBMatcher::KeyFrameView& v) {
  auto mps = kf->getMapPoints();
  v.pos.assign(3 * n, 0.f), v.good.assign(n, 0), v.inMap.assign(n, 0), v.maxDist.assign(n, 0.f), v.minDist.assign(n, 0.f);
  for (size_t i = 0; i < n && i < mps.size(); ++i) {
    const auto& p = mps[i];
    if (!p || p->isBad()) continue;
    v.good[i] = 1, v.inMap[i] = p->isInMap() ? 1 : 0;
    const cv::Mat X = p->getPos();
    for (int a = 0; a < 3; ++a) v.pos[3 * i + a] = X.template at<float>(a);
    p->getDistance(v.maxDist[i], v.minDist[i]);
  }
}
template <class KeyFramePtr, class Access>
inline size_t storedCount(KeyframeStore<Access>& store, const KeyFramePtr& kf) {
  store.ensureFeatures(kf);
  orbfe_kfstore_info i;
  store.info(kf, &i);
  return (size_t)i.n;
}

}  // namespace sim3_detail

// int ORBMatcher::searchBySim3(KeyFramePtr mpCurr, KeyFramePtr mpMatch, std::vector<cv::DMatch>& matches, Sim3Ret& g2oScm, float th)
// (ORBMatcher.h:55, src/ORBMatcher.cc:424-484): both SIM3Project sweeps and the merge in ONE device call; only map state goes up
template <class CameraT, class KeyFramePtr, class Sim3T, class Access>
int searchBySim3(KeyframeStore<Access>& store, KeyFramePtr mpCurr, KeyFramePtr mpMatch, std::vector<cv::DMatch>& matches, Sim3T& g2oScm, float th,
                 float mfRatio = 0.6f) {
  orbfe::ORBMatcher::KeyFrameView C, M;
  sim3_detail::mapState(mpCurr, sim3_detail::storedCount(store, mpCurr), C);
  sim3_detail::mapState(mpMatch, sim3_detail::storedCount(store, mpMatch), M);
  cv::Mat Rcw, tcw, Rmw, tmw;
  mpCurr->getPose(Rcw, tcw), mpMatch->getPose(Rmw, tmw);
  float Rc[9], tc[3], Rm[9], tm[3];
  Bodies::poseFloats(Rcw, tcw, Rc, tc), Bodies::poseFloats(Rmw, tmw, Rm, tm);
  std::vector<std::pair<int, int>> pairs;
  for (const auto& m : matches) pairs.emplace_back(m.queryIdx, m.trainIdx);
  const size_t had = pairs.size();
  orbfe::ORBMatcher(mfRatio).searchBySim3(matcherContext(), store.get(), store.id(mpCurr), store.id(mpMatch), C, M, pairs, Bodies::toSim3(g2oScm), Rc, tc,
                                          Rm, tm, th, Bodies::template intrinsics<CameraT>(mpCurr), Bodies::scaleFactors(mpCurr));
  for (size_t k = had; k < pairs.size(); ++k) {
    cv::DMatch m;
    m.queryIdx = pairs[k].first, m.trainIdx = pairs[k].second;
    matches.push_back(m);
  }
  return (int)matches.size();
}

// int ORBMatcher::searchBySim3(KeyFramePtr pCurr, const std::vector<MapPointPtr>& vLoopGroupMps, std::vector<MapPointPtr>& vMatchedMps,
//                              Sim3Ret& g2oScw, float th)   (ORBMatcher.h:58, src/ORBMatcher.cc:501-559): the projection tests too run on
// the device; the loop group goes up as arrays, pCurr is read where the store keeps it
template <class CameraT, class KeyFramePtr, class MapPointPtr, class Sim3T, class Access>
int searchBySim3(KeyframeStore<Access>& store, KeyFramePtr pCurr, const std::vector<MapPointPtr>& vLoopGroupMps, std::vector<MapPointPtr>& vMatchedMps,
                 Sim3T& g2oScw, float th, float mfRatio = 0.6f) {
  int nMatches = 0;
  std::set<MapPointPtr> sAlreadyMatched;
  for (const auto& p : vMatchedMps)
    if (p && !p->isBad() && p->isInMap()) sAlreadyMatched.insert(p), ++nMatches;
  const size_t m = vLoopGroupMps.size();
  orbfe::ORBMatcher::LoopPoints pts;
  pts.usable.assign(m, 0), pts.pos.assign(3 * m, 0.f), pts.viewDir.assign(3 * m, 0.f), pts.maxDist.assign(m, 0.f), pts.minDist.assign(m, 0.f);
  pts.desc.resize(m);
  for (size_t i = 0; i < m; ++i) {
    const auto& pMp = vLoopGroupMps[i];
    if (!pMp || pMp->isBad() || !pMp->isInMap() || sAlreadyMatched.count(pMp)) continue;
    pts.usable[i] = 1;
    const cv::Mat Xw = pMp->getPos(), vd = pMp->getViewDirection(), d = pMp->getDesc();
    for (int a = 0; a < 3; ++a) pts.pos[3 * i + a] = Xw.template at<float>(a), pts.viewDir[3 * i + a] = vd.template at<float>(a);
    pMp->getDistance(pts.maxDist[i], pts.minDist[i]);
    std::memcpy(pts.desc[i].data(), d.data, 32);
  }
  store.ensureFeatures(pCurr);
  std::vector<int32_t> bestIdx, bestDist;
  orbfe::ORBMatcher(mfRatio).searchBySim3(matcherContext(), store.get(), store.id(pCurr), pts, Bodies::toSim3(g2oScw), th,
                                          Bodies::template intrinsics<CameraT>(pCurr), Bodies::scaleFactors(pCurr), bestIdx, bestDist);
  for (size_t i = 0; i < m; ++i)
    if (bestIdx[i] >= 0) {
      vMatchedMps[(size_t)bestIdx[i]] = vLoopGroupMps[i];
      ++nMatches;
    }
  return nMatches;
}

// setCurrFrameAttrib + OptimizePoseOnly + addMatchByProject of ONE PnP hypothesis (src/Tracking.cc:565-584, :500-517, :612-629): true where the
// reference sets pRelocKf and leaves its loops, false where it goes on to the next hypothesis.  The frame ends with the points, the pose
// and its map points with the counters the reference's chain leaves (Bodies::relocRefine, orbfe_dropin.hpp).
template <class CameraT, class FramePtr, class KeyFramePtr, class RelocBowParamT, class Access>
bool relocRefine(KeyframeStore<Access>& store, FramePtr mpCurrFrame, KeyFramePtr pKF, const RelocBowParamT& relocBowParam, std::size_t idx,
                 const std::vector<std::size_t>& vInliers, const cv::Mat& Rcw, const cv::Mat& tcw) {
  return Bodies::template relocRefine<CameraT>(store, mpCurrFrame, pKF, relocBowParam, idx, vInliers, Rcw, tcw);
}

// bool Tracking::trackReference() (src/Tracking.cc:360-371): computeBow, searchByBow(mpCurrFrame, mpRefKf), the 10-match test,
// OptimizePoseOnly, the 10-inlier test.  The frame ends with the points, the pose, the BoW vectors and its map points with the counters
// the reference's body leaves (Bodies::trackReference, orbfe_dropin.hpp).  vocab: host/compat's DBoW3::Vocabulary (a pointer to it).
template <class CameraT, class VocabPtr, class FramePtr, class KeyFramePtr, class Access>
bool trackReference(KeyframeStore<Access>& store, const VocabPtr& vocab, FramePtr mpCurrFrame, KeyFramePtr mpRefKf) {
  return Bodies::template trackReference<CameraT>(store, vocab, mpCurrFrame, mpRefKf, 0.7f, true);
}

}  // namespace dropin
}  // namespace orbfe
