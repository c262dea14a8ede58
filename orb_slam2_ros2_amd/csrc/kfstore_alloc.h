// kfstore_alloc.h -- the bookkeeping of the keyframe store (orbfe_kfstore.hip): which bytes of which slab an entry occupies, and the
// id map.  Host only, like scratch_layout.h: no HIP header, so tests/cpp/test_kfstore_alloc.cpp compiles it with the host compiler
// alone (and with its sanitizers).  The store's rules live here:
//   - memory comes in slabs of slab_bytes; a block never moves and never spans slabs, so growing the store copies nothing;
//   - a block larger than a slab gets a slab of its own, which is given back whole when the block is freed;
//   - freed space is merged with its free neighbours and reused, first fit, lowest slab first.
// The allocator never touches memory: take() says when a new slab is needed, and the owner allocates it and calls add_slab().
#pragma once
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <map>
#include <unordered_map>
#include <vector>

struct KfBlock {
  int32_t slab = -1;
  size_t off = 0, bytes = 0;
};

class KfSlabAlloc {
 public:
  static const size_t kAlign = 256;
  explicit KfSlabAlloc(size_t slab_bytes) : slab_bytes_(round(slab_bytes ? slab_bytes : kAlign)) {}
  size_t slab_bytes() const { return slab_bytes_; }
  static size_t round(size_t b) { return (b < kAlign ? kAlign : b + kAlign - 1) / kAlign * kAlign; }

  // a block of `bytes` (rounded up to kAlign) out of the existing shared slabs; false: none has room -- the owner allocates
  // slab_size_for(bytes) bytes, calls add_slab() and take() again
  bool take(size_t bytes, KfBlock* out) {
    bytes = round(bytes);
    if (bytes > slab_bytes_) {
      for (size_t s = 0; s < slabs_.size(); ++s)
        if (slabs_[s].live && slabs_[s].own && slabs_[s].bytes == bytes && whole_free(slabs_[s])) return carve((int32_t)s, 0, bytes, out);
      return false;
    }
    for (size_t s = 0; s < slabs_.size(); ++s) {
      if (!slabs_[s].live || slabs_[s].own) continue;
      for (const auto& f : slabs_[s].free)
        if (f.second >= bytes) return carve((int32_t)s, f.first, bytes, out);
    }
    return false;
  }
  size_t slab_size_for(size_t bytes) const { return round(bytes) > slab_bytes_ ? round(bytes) : slab_bytes_; }
  // a new slab of `bytes` (slab_size_for of the request that failed); -> its index, reusing the index of a released slab
  int32_t add_slab(size_t bytes) {
    Slab s;
    s.bytes = bytes;
    s.own = bytes != slab_bytes_;
    s.live = true;
    s.free[0] = bytes;
    for (size_t i = 0; i < slabs_.size(); ++i)
      if (!slabs_[i].live) {
        slabs_[i] = s;
        return (int32_t)i;
      }
    slabs_.push_back(s);
    return (int32_t)slabs_.size() - 1;
  }
  // gives the block back; true: it was a slab of its own, which is now released -- the owner frees slab b.slab's memory
  bool give(const KfBlock& b) {
    Slab& s = slabs_[(size_t)b.slab];
    used_ -= b.bytes;
    if (s.own) {
      s = Slab();
      return true;
    }
    size_t off = b.off, bytes = b.bytes;
    auto next = s.free.lower_bound(off);
    if (next != s.free.begin()) {
      auto prev = std::prev(next);
      if (prev->first + prev->second == off) {
        off = prev->first;
        bytes += prev->second;
        s.free.erase(prev);
      }
    }
    if (next != s.free.end() && off + bytes == next->first) {
      bytes += next->second;
      s.free.erase(next);
    }
    s.free[off] = bytes;
    return false;
  }
  size_t n_slabs() const { return slabs_.size(); }  // indices handed out so far (released ones included)
  bool slab_live(size_t s) const { return slabs_[s].live; }
  size_t slab_size(size_t s) const { return slabs_[s].bytes; }
  size_t used_bytes() const { return used_; }
  size_t reserved_bytes() const {
    size_t r = 0;
    for (const Slab& s : slabs_) r += s.live ? s.bytes : 0;
    return r;
  }
  // (tests) the free lists are sorted, merged, inside their slab and disjoint from `blocks`, which are disjoint from each other
  bool consistent(const std::vector<KfBlock>& blocks) const {
    std::vector<std::map<size_t, size_t>> all(slabs_.size());
    size_t used = 0;
    for (const KfBlock& b : blocks) {
      if (b.slab < 0 || (size_t)b.slab >= slabs_.size() || !slabs_[(size_t)b.slab].live || b.off % kAlign || b.bytes % kAlign || !b.bytes) return false;
      if (!all[(size_t)b.slab].emplace(b.off, b.bytes).second) return false;
      used += b.bytes;
    }
    if (used != used_) return false;
    for (size_t s = 0; s < slabs_.size(); ++s) {
      if (!slabs_[s].live) {
        if (!all[s].empty()) return false;
        continue;
      }
      size_t last_free_end = (size_t)-1;
      for (const auto& f : slabs_[s].free) {
        if (f.first == last_free_end || !f.second) return false;  // two free neighbours not merged
        last_free_end = f.first + f.second;
        if (!all[s].emplace(f.first, f.second).second) return false;
      }
      size_t at = 0;
      for (const auto& r : all[s]) {  // blocks and free runs together tile the slab
        if (r.first != at) return false;
        at += r.second;
      }
      if (at != slabs_[s].bytes) return false;
    }
    return true;
  }

 private:
  struct Slab {
    size_t bytes = 0;
    bool own = false, live = false;
    std::map<size_t, size_t> free;  // offset -> bytes
  };
  static bool whole_free(const Slab& s) { return s.free.size() == 1 && s.free.begin()->second == s.bytes; }
  bool carve(int32_t s, size_t off, size_t bytes, KfBlock* out) {
    Slab& sl = slabs_[(size_t)s];
    const size_t have = sl.free[off];
    sl.free.erase(off);
    if (have > bytes) sl.free[off + bytes] = have - bytes;
    out->slab = s, out->off = off, out->bytes = bytes;
    used_ += bytes;
    return true;
  }
  size_t slab_bytes_, used_ = 0;
  std::vector<Slab> slabs_;
};

// id -> entry.  A thin wrapper so that the stand-alone test covers the store's "present / absent" rules together with the allocator.
template <class Entry>
class KfIdMap {
 public:
  Entry* find(uint64_t id) {
    auto it = m_.find(id);
    return it == m_.end() ? nullptr : &it->second;
  }
  const Entry* find(uint64_t id) const {
    auto it = m_.find(id);
    return it == m_.end() ? nullptr : &it->second;
  }
  Entry* insert(uint64_t id, const Entry& e) {  // nullptr: the id is present (nothing changes)
    auto r = m_.emplace(id, e);
    return r.second ? &r.first->second : nullptr;
  }
  bool erase(uint64_t id, Entry* out) {  // false: unknown id
    auto it = m_.find(id);
    if (it == m_.end()) return false;
    *out = it->second;
    m_.erase(it);
    return true;
  }
  size_t size() const { return m_.size(); }
  template <class F>
  void for_each(F f) const {
    for (const auto& kv : m_) f(kv.first, kv.second);
  }

 private:
  std::unordered_map<uint64_t, Entry> m_;
};
