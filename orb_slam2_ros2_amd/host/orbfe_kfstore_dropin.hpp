// orbfe_kfstore_dropin.hpp -- LocalMapping::fuseMapPoints and LocalMapping::createNewMapPoints over keyframes RESIDENT on the device
// (orbfe_kfstore, include/orbfe.h).  INTEGRATION.md section 12: one orbfe::dropin::KeyframeStore<> per map,
//     store.addFromSlot(ctx, pKf, slot, pair)   where KeyFrame::create has the frame's features in an extraction slot,
//     store.erase(pKf)                          in LocalMapping::deleteKeyFrame,
// and the two bodies become
//     orbfe::dropin::fuseMapPoints<Camera, Frame>(mpCurrKeyFrame, mpMap, store);
//     orbfe::dropin::createNewMapPoints<Camera, Frame>(mpCurrKeyFrame, mmUnprocessMps, mpMap, mlpAddedMPs, store);
// Both are the bodies of orbfe_fuse_dropin.hpp / orbfe_mapping_dropin.hpp -- the same selection, replay and record handling
//  -- with the device call exchanged: only poses and map state go up.  A keyframe the store does not hold yet (a loaded map,
// a call site not wired to addFromSlot) is inserted from its host arrays on first use, so the overloads work from the first call on.
#pragma once

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbfe_fuse_dropin.hpp"
#include "orbfe_mapping_dropin.hpp"

namespace orbfe {
namespace dropin {

struct ReferenceKeyFrame {  // how the store reads the reference's KeyFrame: KeyFrame::getID(), VirtualFrame::mfMinU .. mfMaxV
  template <class KeyFramePtr>
  static uint64_t id(const KeyFramePtr& pKf) {
    return (uint64_t)pKf->getID();
  }
  template <class KeyFramePtr>
  static void bounds(const KeyFramePtr& pKf, float b[4]) {
    Bodies::bounds(pKf, b);
  }
};

// Owns one orbfe_kfstore and names its entries by the keyframes' ids.  Access: how a keyframe pointer gives its id and bounds.
template <class Access = ReferenceKeyFrame>
class KeyframeStore {
 public:
  // width, height: the image size (what a keyframe without bounds would get; the bodies always pass bounds); nLevels: ORBExtractor::mnLevels
  KeyframeStore(int width, int height, int nLevels, int deviceId = 0, int64_t slabBytes = 0) : nLevels_(nLevels) {
    if (orbfe_kfstore_create(deviceId, width, height, nLevels, slabBytes, &store_) != ORBFE_OK)
      throw std::runtime_error(std::string("orbfe_kfstore_create: ") + orbfe_last_error(nullptr));
  }
  ~KeyframeStore() { orbfe_kfstore_destroy(store_); }
  KeyframeStore(const KeyframeStore&) = delete;
  KeyframeStore& operator=(const KeyframeStore&) = delete;

  orbfe_kfstore* get() const { return store_; }
  int levels() const { return nLevels_; }
  template <class KeyFramePtr>
  uint64_t id(const KeyFramePtr& pKf) const {
    return Access::id(pKf);
  }
  template <class KeyFramePtr>
  bool info(const KeyFramePtr& pKf, orbfe_kfstore_info* out) const {
    return orbfe_kfstore_info_get(store_, id(pKf), out) == ORBFE_OK;
  }
  size_t size() const {
    int64_t n = 0;
    check(orbfe_kfstore_size(store_, &n, nullptr, nullptr), "orbfe_kfstore_size", nullptr);
    return (size_t)n;
  }

  // KeyFrame::create(const VirtualFrame&): the frame's features are in extraction slot `slot` of ctx (pair >= 0: with that stereo pair's
  // right_u and depth); nothing of them crosses to the host
  template <class KeyFramePtr>
  int addFromSlot(orbfe_ctx* ctx, const KeyFramePtr& pKf, int slot, int pair) {
    float b[4];
    Access::bounds(pKf, b);
    int32_t n = 0;
    check(orbfe_kfstore_add_from_slot(ctx, store_, id(pKf), slot, pair, b, &n), "orbfe_kfstore_add_from_slot", ctx);
    return n;
  }
  // from the keyframe's host arrays (loaded maps).  add: features and bounds as the fuse bodies read them (Bodies::target), no stereo
  // columns; addMapping: through the getters createNewMapPoints' body uses, with depth and right_u
  template <class KeyFramePtr>
  void add(const KeyFramePtr& pKf) {
    Bodies::Target t;
    Bodies::target(pKf, t);
    check(orbfe_kfstore_add(store_, id(pKf), (int32_t)t.kps.size(), t.kps.data(), t.desc.empty() ? nullptr : t.desc[0].data(), nullptr, nullptr, t.bounds),
          "orbfe_kfstore_add", nullptr);
  }
  template <class KeyFramePtr>
  void addMapping(const KeyFramePtr& pKf) {
    const auto& kps = pKf->getLeftKeyPoints();
    const auto& desc = pKf->getDescriptor();
    const std::vector<double> depth = pKf->getDepth(), ru = pKf->getRightU();
    const size_t n = kps.size();
    static_assert(sizeof(orbfe_keypoint) == sizeof(kps[0]), "cv::KeyPoint is orbfe_keypoint");
    std::vector<uint8_t> d(n * 32);
    for (size_t i = 0; i < n; ++i) std::memcpy(&d[32 * i], desc[i].data, 32);
    float b[4];
    Access::bounds(pKf, b);
    check(orbfe_kfstore_add(store_, id(pKf), (int32_t)n, (const orbfe_keypoint*)kps.data(), d.data(), depth.size() == n ? depth.data() : nullptr,
                            ru.size() == n ? ru.data() : nullptr, b),
          "orbfe_kfstore_add", nullptr);
  }
  // the keyframe's FeatureVector (KeyFrame::computeBow first)
  template <class KeyFramePtr>
  void setBow(const KeyFramePtr& pKf) {
    pKf->computeBow();
    std::vector<uint32_t> nodes, features;
    std::vector<int32_t> offsets(1, 0);
    for (const auto& node : Bodies::featVec(pKf)) {
      nodes.push_back((uint32_t)node.first);
      for (const auto f : node.second) features.push_back((uint32_t)f);
      offsets.push_back((int32_t)features.size());
    }
    check(orbfe_kfstore_set_bow(store_, id(pKf), (int32_t)nodes.size(), nodes.data(), offsets.data(), features.data()), "orbfe_kfstore_set_bow", nullptr);
  }
  // LocalMapping::deleteKeyFrame
  template <class KeyFramePtr>
  void erase(const KeyFramePtr& pKf) {
    const uint64_t i = id(pKf);
    check(orbfe_kfstore_erase(store_, 1, &i), "orbfe_kfstore_erase", nullptr);
  }

  // present for the fuse (features, grid) / for the triangulation (stereo columns and FeatureVector too): inserted on first use.
  // The fuse bodies read a keyframe through Bodies::target, which has no stereo columns, so an entry they inserted says has_stereo = 0
  // (orbfe_kfstore_info); when the triangulation meets such an entry -- fuseMapPoints reaches second-order neighbours before they become
  // triangulation neighbours -- it REPLACES it from the keyframe's getters (erase + addMapping under the store's exclusive lock; no stored
  // call runs meanwhile), so that depth and right_u are the keyframe's and not -1.
  template <class KeyFramePtr>
  void ensureFeatures(const KeyFramePtr& pKf) {
    orbfe_kfstore_info i;
    if (!info(pKf, &i)) add(pKf);
  }
  template <class KeyFramePtr>
  void ensureMapping(const KeyFramePtr& pKf) {
    orbfe_kfstore_info i;
    const bool present = info(pKf, &i);
    if (!present || !i.has_stereo) {
      if (present) erase(pKf);
      addMapping(pKf);
      i.has_bow = 0;
    }
    if (!i.has_bow) setBow(pKf);
  }
  // present with its FeatureVector, for the batched searchByBow (orbfe_reloc_dropin.hpp), which reads no stereo column: an entry the fuse
  // inserted only gets its FeatureVector
  template <class KeyFramePtr>
  void ensureBow(const KeyFramePtr& pKf) {
    orbfe_kfstore_info i;
    if (!info(pKf, &i)) {
      addMapping(pKf);
      i.has_bow = 0;
    }
    if (!i.has_bow) setBow(pKf);
  }

 private:
  static void check(orbfe_status st, const char* what, orbfe_ctx* ctx) {
    if (st != ORBFE_OK) throw std::runtime_error(std::string(what) + ": " + orbfe_last_error(ctx));
  }
  orbfe_kfstore* store_ = nullptr;
  int nLevels_;
};

namespace fuse_detail {

// the batch call of fuseIntoKeyframes over stored keyframes (the shape of UploadSearch): ids and poses only
template <class Store>
struct StoredSearch {
  Store& store;
  uint64_t curId = 0;
  int32_t nCur = 0;
  std::vector<uint64_t> ids;
  std::vector<orbfe_fuse_pose> poses;
  explicit StoredSearch(Store& s) : store(s) {}
  template <class KeyFramePtr>
  int prepare(KeyFramePtr cur, const KeyFramePtr* targets, size_t K) {
    store.ensureFeatures(cur);
    curId = store.id(cur);
    nCur = (int32_t)cur->getMapPoints().size();
    ids.resize(K);
    poses.resize(K);
    for (size_t k = 0; k < K; ++k) {
      store.ensureFeatures(targets[k]);
      ids[k] = store.id(targets[k]);
      cv::Mat Rcw, tcw;
      targets[k]->getPose(Rcw, tcw);
      Bodies::poseFloats(Rcw, tcw, poses[k].Rcw, poses[k].tcw);
    }
    return store.levels();
  }
  orbfe_status run(orbfe_ctx* ctx, const orbfe_fuse_points* pts, const float* z, const orbfe_camera* cam, float bl, const float* sf, int n_levels,
                   float ratio, int32_t* bestIdx, int32_t* bestDist, uint8_t* visible) {
    return orbfe_fuse_into_keyframes_stored(ctx, store.get(), curId, nCur, pts, (int32_t)ids.size(), ids.data(), poses.data(), z, cam, bl, sf, n_levels,
                                            3.0f, ratio, orbfe::ORBMatcher::mnMinThreshold, bestIdx, bestDist, visible);
  }
  static const char* name() { return "orbfe_fuse_into_keyframes_stored"; }
};

}  // namespace fuse_detail

namespace tri_detail {

// the device call of createNewMapPoints over stored keyframes (the shape of UploadCall): flags and poses only
template <class Store>
struct StoredCall {
  Store& store;
  std::vector<uint64_t> ids;              // [0]: cur
  std::vector<std::vector<uint8_t>> flags;
  std::vector<orbfe_tri_state> st;
  explicit StoredCall(Store& s) : store(s) {}
  template <class KeyFramePtr>
  void state(const KeyFramePtr& pkf, size_t at) {
    store.ensureMapping(pkf);
    ids[at] = store.id(pkf);
    const auto mps = pkf->getMapPoints();
    std::vector<uint8_t>& f = flags[at];
    f.assign(mps.size(), 0);
    for (size_t i = 0; i < mps.size(); ++i) {
      const bool good = mps[i] && !mps[i]->isBad();
      f[i] = (uint8_t)((good ? ORBFE_TRI_GOOD : 0) | (good && mps[i]->isInMap() ? ORBFE_TRI_INMAP : 0));
    }
    orbfe_tri_state& s = st[at];
    s = orbfe_tri_state();
    s.n = (int32_t)f.size();
    s.flags = f.data();
    const cv::Mat Tcw = pkf->getPose(), Twc = pkf->getPoseInv(), Ow = pkf->getFrameCenter();
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) s.Tcw[4 * r + c] = Tcw.template at<float>(r, c), s.Twc[4 * r + c] = Twc.template at<float>(r, c);
    for (int a = 0; a < 3; ++a) s.Ow[a] = Ow.template at<float>(a);
  }
  template <class KeyFramePtr>
  int prepare(const KeyFramePtr& cur, const std::vector<KeyFramePtr>& nbs) {
    ids.resize(nbs.size() + 1);
    flags.resize(nbs.size() + 1);
    st.resize(nbs.size() + 1);
    state(cur, 0);
    for (size_t i = 0; i < nbs.size(); ++i) state(nbs[i], i + 1);
    return store.levels();
  }
  orbfe_status run(orbfe_ctx* ctx, const Unprocessed& un, const orbfe_camera* cam, const float* k_inv, float bl, const float* sf, int n_levels,
                   orbfe_tri_record* recs, int64_t cap, int64_t* n_rec, int32_t* tail, int64_t* n_tail, uint8_t* consumed) {
    st[0].unproc = un.flag.data();
    st[0].unproc_pos = un.pos.data();
    return orbfe_create_new_map_points_stored(ctx, store.get(), ids[0], &st[0], (int32_t)ids.size() - 1, ids.data() + 1, st.data() + 1, cam, k_inv, bl, sf,
                                              n_levels, recs, cap, n_rec, tail, cap, n_tail, consumed);
  }
  static const char* name() { return "orbfe_create_new_map_points_stored"; }
};

}  // namespace tri_detail

// void LocalMapping::fuseMapPoints()  (src/LocalMapping.cc:352-405) over stored keyframes
template <class CameraT, class FrameT, class KeyFramePtr, class MapPtr, class Access>
void fuseMapPoints(KeyFramePtr mpCurrKeyFrame, MapPtr mpMap, KeyframeStore<Access>& store) {
  fuse_detail::StoredSearch<KeyframeStore<Access>> search(store);
  fuseMapPoints<CameraT, FrameT>(mpCurrKeyFrame, mpMap, search);
}
template <class CameraT, class FrameT, class KeyFramePtr, class MapPtr, class Access>
int fuseIntoKeyframes(KeyFramePtr cur, const std::vector<KeyFramePtr>& targets, MapPtr map, float mfRatio, KeyframeStore<Access>& store) {
  fuse_detail::StoredSearch<KeyframeStore<Access>> search(store);
  return fuseIntoKeyframes<CameraT, FrameT>(cur, targets, map, mfRatio, search);
}

// void LocalMapping::createNewMapPoints()  (src/LocalMapping.cc:165-285) over stored keyframes
template <class CameraT, class FrameT, class KeyFramePtr, class UnprocessMps, class MapPtr, class MapPointList, class Access>
void createNewMapPoints(KeyFramePtr curKf, UnprocessMps& mmUnprocessMps, MapPtr map, MapPointList& mlpAddedMPs, KeyframeStore<Access>& store) {
  tri_detail::StoredCall<KeyframeStore<Access>> call(store);
  createNewMapPoints<CameraT, FrameT>(curKf, mmUnprocessMps, map, mlpAddedMPs, call);
}

}  // namespace dropin
}  // namespace orbfe
