// orbfe_mpstore_dropin.hpp -- Tracking::trackLocalMap over map points RESIDENT on the device (orbfe_mpstore, include/orbfe.h;
// DESIGN 4.30).  INTEGRATION.md section 22: one orbfe::dropin::MapPointStore<> per map,
//     store.touch(mnId)     at the end of MapPoint::setPos, MapPoint::setDesc and MapPoint::updateNormalAndDepth,
// and Tracking::trackLocalMap's middle becomes
//     nMatches = orbfe::dropin::trackLocalMap<Camera>(store, mpCurrFrame, mvpLocalMps, th, nGood);
// The host objects stay the truth.  The store holds what the last upsert brought: a point that changed is read again (its four locked
// accessors) once, at the next flush, instead of on every frame; a point the store has never seen goes in from its accessors on first
// use, so the overload works from the first call on.  isBad / isInMap are read per call and travel as flags: no hook for them.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

#include "orbfe_dropin.hpp"

namespace orbfe {
namespace dropin {

struct ReferenceMapPoint {  // how the store reads the reference's MapPoint: MapPoint::getID()
  template <class MapPointPtr>
  static uint64_t id(const MapPointPtr& pMp) {
    return (uint64_t)pMp->getID();
  }
};

// Owns one orbfe_mpstore and keeps it coherent with the map points.  touch() may come from any thread; flush / ensure / erase / verify
// serialise among themselves.
template <class Access = ReferenceMapPoint>
class MapPointStore {
 public:
  explicit MapPointStore(int deviceId = 0, int rowsPerPage = 0, int maxPages = 0) {
    if (orbfe_mpstore_create(deviceId, rowsPerPage, maxPages, &store_) != ORBFE_OK)
      throw std::runtime_error(std::string("orbfe_mpstore_create: ") + orbfe_last_error(nullptr));
  }
  ~MapPointStore() { orbfe_mpstore_destroy(store_); }
  MapPointStore(const MapPointStore&) = delete;
  MapPointStore& operator=(const MapPointStore&) = delete;

  orbfe_mpstore* get() const { return store_; }
  template <class MapPointPtr>
  uint64_t id(const MapPointPtr& pMp) const {
    return Access::id(pMp);
  }
  size_t size() const {
    int64_t n = 0;
    check(orbfe_mpstore_size(store_, &n, nullptr, nullptr), "orbfe_mpstore_size", nullptr);
    return (size_t)n;
  }

  // the point `id` changed (setPos, setDesc, updateNormalAndDepth): its row is stale until the point is read again
  void touch(uint64_t id) {
    std::lock_guard<std::mutex> lk(touchMu_);
    touched_.push_back(id);
  }
  // Takes the touched ids over into the set of STALE ids: points the store holds whose row is older than the object.  A stale point
  // is read again -- getPos / getViewDirection / getDistance / getDesc, only of such points -- by the first ensure() that meets it, or by
  // flush(lookup); until then it stays in the set however many frames pass, so a point that changes while it is outside the local
  // map is current again on the frame it comes back.  A touched id the store has never held is dropped: ensure() reads that point when
  // it is first needed.  Cost: the touches since the last call, nothing per stale id.
  void flush() {
    std::lock_guard<std::mutex> lk(mu_);
    drain();
  }
  // ... and reads the stale points lookup(id) can reach now, upserting them in one call (an integrator with a map-wide index by id calls
  // this from the mapping thread, off the tracking thread's path).  lookup(id): the map point, or a null pointer: the id stays stale.
  template <class Lookup>
  void flush(Lookup&& lookup) {
    std::lock_guard<std::mutex> lk(mu_);
    drain();
    Rows rows;
    for (auto it = stale_.begin(); it != stale_.end();) {
      const auto pMp = lookup(*it);
      if (!pMp) {
        ++it;
        continue;
      }
      rows.read(*it, pMp);
      it = stale_.erase(it);
    }
    try {
      rows.upsert(store_);
    } catch (...) {  // (a refused upsert has changed nothing: the points are as stale as before)
      stale_.insert(rows.ids.begin(), rows.ids.end());
      throw;
    }
  }
  // Every non-null point of the list the store has never seen goes in from its accessors, and every stale one is read again, in one call.
  template <class MapPointPtr>
  void ensure(const std::vector<MapPointPtr>& points) {
    std::lock_guard<std::mutex> lk(mu_);
    Rows rows;
    std::vector<uint64_t> fresh, again;
    for (const auto& pMp : points) {
      if (!pMp) continue;
      const uint64_t i = Access::id(pMp);
      if (known_.insert(i).second)
        rows.read(i, pMp), fresh.push_back(i);
      else if (!stale_.empty() && stale_.erase(i))
        rows.read(i, pMp), again.push_back(i);
    }
    try {
      rows.upsert(store_);
    } catch (...) {  // (a refused upsert has changed nothing: unknown points stay unknown, stale ones stale)
      for (uint64_t i : fresh) known_.erase(i);
      stale_.insert(again.begin(), again.end());
      throw;
    }
  }
  size_t staleCount() {
    std::lock_guard<std::mutex> lk(mu_);
    return stale_.size();
  }
  // a destroyed point's id (optional: a row nobody names costs nothing, and a new point of that id overwrites it)
  void erase(const std::vector<uint64_t>& ids) {
    std::lock_guard<std::mutex> lk(mu_);
    check(orbfe_mpstore_erase(store_, (int32_t)ids.size(), ids.data()), "orbfe_mpstore_erase", nullptr);
    for (uint64_t i : ids) known_.erase(i), stale_.erase(i);
  }
  // For tests and an integrator's debug build: fetches the rows of the listed points the store holds, compares them with the live
  // objects and returns the ids that differ -- each the id of a point that changed without a touch (or that is touched and not read again yet).
  template <class MapPointPtr>
  std::vector<uint64_t> verify(const std::vector<MapPointPtr>& points) {
    std::lock_guard<std::mutex> lk(mu_);
    Rows live, got;
    std::unordered_set<uint64_t> seen;
    for (const auto& pMp : points) {
      if (!pMp) continue;
      const uint64_t i = Access::id(pMp);
      if (known_.count(i) && seen.insert(i).second) live.read(i, pMp);
    }
    const size_t n = live.ids.size();
    got.pos.resize(3 * n), got.viewDir.resize(3 * n), got.maxDist.resize(n), got.minDist.resize(n), got.desc.resize(32 * n);
    check(orbfe_mpstore_fetch(store_, (int32_t)n, live.ids.data(), got.pos.data(), got.viewDir.data(), got.maxDist.data(), got.minDist.data(), got.desc.data()),
          "orbfe_mpstore_fetch", nullptr);
    std::vector<uint64_t> differ;
    for (size_t k = 0; k < n; ++k)
      if (std::memcmp(&live.pos[3 * k], &got.pos[3 * k], 12) || std::memcmp(&live.viewDir[3 * k], &got.viewDir[3 * k], 12) ||
          std::memcmp(&live.maxDist[k], &got.maxDist[k], 4) || std::memcmp(&live.minDist[k], &got.minDist[k], 4) ||
          std::memcmp(&live.desc[32 * k], &got.desc[32 * k], 32))
        differ.push_back(live.ids[k]);
    return differ;
  }

 private:
  static void check(orbfe_status st, const char* what, orbfe_ctx* ctx) {
    if (st != ORBFE_OK) throw std::runtime_error(std::string(what) + ": " + orbfe_last_error(ctx));
  }
  // the arrays of one upsert, filled from the map points' accessors (an empty view direction or descriptor: zeros, as
  // dropin::trackLocalMap sends them)
  struct Rows {
    std::vector<uint64_t> ids;
    std::vector<float> pos, viewDir, maxDist, minDist;
    std::vector<uint8_t> desc;
    template <class MapPointPtr>
    void read(uint64_t id, const MapPointPtr& pMp) {
      const cv::Mat p = pMp->getPos(), v = pMp->getViewDirection(), d = pMp->getDesc();
      float mx = 0.f, mn = 0.f;
      pMp->getDistance(mx, mn);
      ids.push_back(id);
      for (int a = 0; a < 3; ++a) pos.push_back(p.template at<float>(a)), viewDir.push_back(v.empty() ? 0.f : v.template at<float>(a));
      maxDist.push_back(mx), minDist.push_back(mn);
      const size_t o = desc.size();
      desc.resize(o + 32, 0);
      if (!d.empty()) std::memcpy(desc.data() + o, d.data, 32);
    }
    void upsert(orbfe_mpstore* s) const {
      if (ids.empty()) return;
      check(orbfe_mpstore_upsert(s, (int32_t)ids.size(), ids.data(), ORBFE_MP_ALL, pos.data(), viewDir.data(), maxDist.data(), minDist.data(), desc.data()),
            "orbfe_mpstore_upsert", nullptr);
    }
  };

  // touched_ -> stale_ (mu_ held): only ids the store holds can be stale
  void drain() {
    std::vector<uint64_t> ids;
    {
      std::lock_guard<std::mutex> tl(touchMu_);
      ids.swap(touched_);
    }
    for (uint64_t i : ids)
      if (known_.count(i)) stale_.insert(i);
  }
  orbfe_mpstore* store_ = nullptr;
  std::mutex mu_;                       // flush / ensure / erase / verify
  std::unordered_set<uint64_t> known_;  // the ids the store holds (host side: no device call to ask)
  std::unordered_set<uint64_t> stale_;  // of those, the touched ones whose row has not been read again yet
  std::mutex touchMu_;
  std::vector<uint64_t> touched_;
};

// Tracking::trackLocalMap's middle over the store: Bodies::trackLocalMapStored (orbfe_dropin.hpp)
template <class CameraT, class Access, class FramePtr, class MapPointPtr>
int trackLocalMap(MapPointStore<Access>& store, FramePtr pframe, const std::vector<MapPointPtr>& mapPoints, float th, int& nGood, float mfRatio = 0.8f,
                  int nLevels = 8, int minMatches = 30) {
  return Bodies::template trackLocalMapStored<CameraT>(store, pframe, mapPoints, th, mfRatio, nLevels, nGood, minMatches);
}
// ... in the argument order of Bodies::trackLocalMap
template <class CameraT, class Access, class FramePtr, class MapPointPtr>
int trackLocalMap(MapPointStore<Access>& store, FramePtr pframe, const std::vector<MapPointPtr>& mapPoints, float th, float mfRatio, int nLevels, int& nGood,
                  int minMatches = 30) {
  return Bodies::template trackLocalMapStored<CameraT>(store, pframe, mapPoints, th, mfRatio, nLevels, nGood, minMatches);
}

}  // namespace dropin
}  // namespace orbfe
