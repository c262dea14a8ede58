// orbfe_mapping_dropin.hpp -- LocalMapping::createNewMapPoints (src/LocalMapping.cc:165-285) on the device (orbfe_create_new_map_points,
// include/orbfe.h).  INTEGRATION.md section 10: the body of LocalMapping::createNewMapPoints becomes
//     orbfe::dropin::createNewMapPoints<Camera, Frame>(mpCurrKeyFrame, mmUnprocessMps, mpMap, mlpAddedMPs);
// The template reproduces loop 1's neighbour selection (getOrderedConnectedKfs(10), null and bad skipped, the std::map dedup and order;
// the baseline test runs inside the call), flattens the keyframes, makes ONE device call on the calling thread's matcherContext() and
// applies the records in order with the reference's own calls, then erases the consumed unprocessed points and runs the tail.
// The FeatureVector is read through orbfe::dropin::Bodies (INTEGRATION section 3's friend line).  A failed call throws std::runtime_error.
#pragma once

#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

#include "orbfe_dropin.hpp"

namespace orbfe {
namespace dropin {

namespace tri_detail {

struct Flat {  // one keyframe's arrays behind an orbfe_tri_kf
  std::vector<orbfe_keypoint> kps;
  std::vector<uint8_t> desc, flags, unproc;
  std::vector<uint32_t> nodes, features;
  std::vector<int32_t> offsets;
  std::vector<double> depth, right_u;
  std::vector<float> unproc_pos;
  orbfe_tri_kf kf{};
};

template <class KeyFramePtr>
void flatten(const KeyFramePtr& pkf, Flat& f, int& n_levels) {
  pkf->computeBow();
  const auto& kps = pkf->getLeftKeyPoints();
  const auto& desc = pkf->getDescriptor();
  const auto mps = pkf->getMapPoints();
  const size_t n = kps.size();
  f.kps.resize(n);
  static_assert(sizeof(orbfe_keypoint) == sizeof(kps[0]), "cv::KeyPoint is orbfe_keypoint");
  if (n) std::memcpy(f.kps.data(), kps.data(), n * sizeof(orbfe_keypoint));
  f.desc.resize(n * 32);
  f.flags.assign(n, 0);
  for (size_t i = 0; i < n; ++i) {
    std::memcpy(&f.desc[32 * i], desc[i].data, 32);
    const bool good = mps[i] && !mps[i]->isBad();
    f.flags[i] = (uint8_t)((good ? ORBFE_TRI_GOOD : 0) | (good && mps[i]->isInMap() ? ORBFE_TRI_INMAP : 0));
    n_levels = std::max(n_levels, kps[i].octave + 1);
  }
  f.offsets.assign(1, 0);
  for (const auto& node : Bodies::featVec(pkf)) {  // DBoW3::FeatureVector: ascending node ids, feature ids in insertion (ascending) order
    f.nodes.push_back((uint32_t)node.first);
    for (const auto id : node.second) f.features.push_back((uint32_t)id);
    f.offsets.push_back((int32_t)f.features.size());
  }
  f.depth = pkf->getDepth();
  f.right_u = pkf->getRightU();
  const cv::Mat Tcw = pkf->getPose(), Twc = pkf->getPoseInv(), Ow = pkf->getFrameCenter();
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) f.kf.Tcw[4 * r + c] = Tcw.template at<float>(r, c), f.kf.Twc[4 * r + c] = Twc.template at<float>(r, c);
  for (int a = 0; a < 3; ++a) f.kf.Ow[a] = Ow.template at<float>(a);
  f.kf.n = (int32_t)n;
  f.kf.kps = f.kps.data();
  f.kf.desc = f.desc.data();
  f.kf.n_nodes = (int32_t)f.nodes.size();
  f.kf.nodes = f.nodes.data();
  f.kf.node_offsets = f.offsets.data();
  f.kf.features = f.features.data();
  f.kf.flags = f.flags.data();
  f.kf.depth = f.depth.data();
  f.kf.right_u = f.right_u.data();
}

// cur's entries of mmUnprocessMps as the call wants them
struct Unprocessed {
  std::vector<uint8_t> flag;
  std::vector<float> pos;
};

// The device call behind createNewMapPoints as an object: prepare() takes the current keyframe and its neighbours and returns the number
// of pyramid levels the scale factors must cover, run() makes the call.  This one uploads every keyframe's arrays with the call
// (orbfe_create_new_map_points); orbfe_kfstore_dropin.hpp has the one over keyframes resident in a store.
struct UploadCall {
  std::vector<Flat> flat;
  std::vector<orbfe_tri_kf> nbk;
  template <class KeyFramePtr>
  int prepare(const KeyFramePtr& cur, const std::vector<KeyFramePtr>& nbs) {
    int n_levels = 1;
    flat.assign(nbs.size() + 1, Flat());
    flatten(cur, flat[0], n_levels);
    for (size_t i = 0; i < nbs.size(); ++i) flatten(nbs[i], flat[i + 1], n_levels);
    return n_levels;
  }
  orbfe_status run(orbfe_ctx* ctx, const Unprocessed& un, const orbfe_camera* cam, const float* k_inv, float bl, const float* sf, int n_levels,
                   orbfe_tri_record* recs, int64_t cap, int64_t* n_rec, int32_t* tail, int64_t* n_tail, uint8_t* consumed) {
    flat[0].kf.unproc = un.flag.data();
    flat[0].kf.unproc_pos = un.pos.data();
    nbk.clear();
    for (size_t i = 1; i < flat.size(); ++i) nbk.push_back(flat[i].kf);
    return orbfe_create_new_map_points(ctx, &flat[0].kf, (int32_t)nbk.size(), nbk.data(), cam, k_inv, bl, sf, n_levels, recs, cap, n_rec, tail, cap,
                                       n_tail, consumed);
  }
  static const char* name() { return "orbfe_create_new_map_points"; }
};

}  // namespace tri_detail

// void LocalMapping::createNewMapPoints()  (src/LocalMapping.cc:165-285); call: tri_detail::UploadCall or an object of its shape
template <class CameraT, class FrameT, class KeyFramePtr, class UnprocessMps, class MapPtr, class MapPointList, class Call>
void createNewMapPoints(KeyFramePtr curKf, UnprocessMps& mmUnprocessMps, MapPtr map, MapPointList& mlpAddedMPs, Call& call) {
  typedef typename UnprocessMps::mapped_type MapPointPtr;
  // loop 1's neighbour selection: the std::map<KeyFrame::SharedPtr, ..> dedups and orders (T2); the baseline test is the call's (T7)
  std::map<KeyFramePtr, int> chosen;
  for (const auto& pKf : curKf->getOrderedConnectedKfs(10))
    if (pKf && !pKf->isBad()) chosen.emplace(pKf, 0);
  std::vector<KeyFramePtr> nbs;
  for (const auto& it : chosen) nbs.push_back(it.first);
  const int n_levels = call.prepare(curKf, nbs);
  const size_t n = curKf->getLeftKeyPoints().size();
  tri_detail::Unprocessed un;
  un.flag.assign(n, 0);
  un.pos.assign(3 * n, 0.f);
  for (const auto& item : mmUnprocessMps) {
    if (item.first >= n || !item.second) continue;
    const cv::Mat p = item.second->getPos();
    un.flag[item.first] = 1;
    for (int a = 0; a < 3; ++a) un.pos[3 * item.first + a] = p.template at<float>(a);
  }
  std::vector<float> sf((size_t)n_levels);
  for (int l = 0; l < n_levels; ++l) sf[(size_t)l] = FrameT::getScaledFactor(l);
  float k_inv[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) k_inv[3 * r + c] = CameraT::mKInv.template at<float>(r, c);
  orbfe_camera cam{};
  cam.fx = CameraT::mfFx, cam.fy = CameraT::mfFy, cam.cx = CameraT::mfCx, cam.cy = CameraT::mfCy;
  std::vector<orbfe_tri_record> recs(n);
  std::vector<int32_t> tail(n);
  std::vector<uint8_t> consumed(n);
  int64_t n_rec = 0, n_tail = 0;
  orbfe_ctx* ctx = matcherContext();
  const orbfe_status st = call.run(ctx, un, &cam, k_inv, CameraT::mfBl, sf.data(), n_levels, recs.data(), (int64_t)n, &n_rec, tail.data(), &n_tail,
                                   consumed.data());
  if (st != ORBFE_OK) throw std::runtime_error(std::string(Call::name()) + ": " + orbfe_last_error(ctx));
  // loop 2, applied in processing order with the reference's own calls (LocalMapping.cc:248-262)
  for (int64_t r = 0; r < n_rec; ++r) {
    const orbfe_tri_record& x = recs[(size_t)r];
    const KeyFramePtr& pKf = nbs[(size_t)x.nb];
    MapPointPtr pMp;
    if (x.kind == ORBFE_TRI_OWN_STEREO) {
      pMp = mmUnprocessMps[(size_t)x.query];
    } else {
      cv::Mat p3dW(3, 1, CV_32F);
      for (int a = 0; a < 3; ++a) p3dW.template at<float>(a) = x.xyz[a];
      pMp = std::remove_reference<decltype(*pMp)>::type::create(p3dW);
    }
    curKf->setMapPoint(x.query, pMp);
    pKf->setMapPoint(x.train, pMp);
    pMp->addAttriInit(curKf, (std::size_t)x.query);
    pMp->addObservation(pKf, (std::size_t)x.train);
    pMp->updateDescriptor();
    pMp->updateNormalAndDepth();
    map->insertMapPoint(pMp, map);
    mlpAddedMPs.push_back(pMp);
  }
  // the own-stereo branch erased what it consumed, accepted or not (T5)
  for (size_t q = 0; q < n; ++q)
    if (consumed[q]) mmUnprocessMps.erase(q);
  // the tail loop over mmUnprocessMps in the container's own order (LocalMapping.cc:266-278); the call says which slots are still empty (T6)
  std::unordered_set<std::size_t> restore;
  for (int64_t i = 0; i < n_tail; ++i) restore.insert((std::size_t)tail[(size_t)i]);
  for (const auto& item : mmUnprocessMps) {
    if (!restore.count(item.first)) continue;
    curKf->setMapPoint(item.first, item.second);
    item.second->addAttriInit(curKf, item.first);
    map->insertMapPoint(item.second, map);
    mlpAddedMPs.push_back(item.second);
  }
}
template <class CameraT, class FrameT, class KeyFramePtr, class UnprocessMps, class MapPtr, class MapPointList>
void createNewMapPoints(KeyFramePtr curKf, UnprocessMps& mmUnprocessMps, MapPtr map, MapPointList& mlpAddedMPs) {
  tri_detail::UploadCall call;
  createNewMapPoints<CameraT, FrameT>(curKf, mmUnprocessMps, map, mlpAddedMPs, call);
}

}  // namespace dropin
}  // namespace orbfe
