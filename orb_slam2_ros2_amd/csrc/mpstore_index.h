// mpstore_index.h -- the bookkeeping of the map-point store (orbfe_mpstore.hip): where a point id lives and which ids are
// present.  Host only, like kfstore_alloc.h: no HIP header, so tests/cpp/test_mpstore_index.cpp compiles it with the host compiler alone
// (and with its sanitizers).  The store's rules live here:
//   - a paged direct index, no hash: id -> page id / rows_per_page, row id % rows_per_page (MapPoint ids are sequential);
//   - a page exists from the first upsert that names one of its rows and never moves;
//   - an id at or past rows_per_page * max_pages has no place: the capacity refusal;
//   - an id the store does not hold must come with every field, and no id may be listed twice in one upsert.
// The index never touches device memory: check_upsert() says which pages an upsert needs, the owner allocates them and calls add_page(),
// then commit_upsert().  A refused upsert has changed nothing.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

enum : uint32_t { MP_FIELD_POS = 1u, MP_FIELD_NORMAL_DEPTH = 2u, MP_FIELD_DESC = 4u, MP_FIELD_ALL = 7u };
static const size_t kMpRowBytes = 64;  // pos[3] view_dir[3] max_dist min_dist (f32) | desc[32]

enum class MpVerdict { ok, bad_mask, duplicate, partial_first, capacity };

class MpIndex {
 public:
  MpIndex(uint32_t rows_per_page = 16384, uint32_t max_pages = 4096)
      : rpp_(rows_per_page ? rows_per_page : 1), max_pages_(max_pages), present_(max_pages) {}
  uint32_t rows_per_page() const { return rpp_; }
  uint32_t max_pages() const { return max_pages_; }
  uint64_t capacity() const { return (uint64_t)rpp_ * max_pages_; }
  // (valid for id < capacity() only: the page number of a larger id need not fit 32 bits)
  uint32_t page_of(uint64_t id) const { return (uint32_t)(id / rpp_); }
  uint32_t row_of(uint64_t id) const { return (uint32_t)(id % rpp_); }
  bool has_page(uint32_t p) const { return p < max_pages_ && !present_[p].empty(); }
  bool has(uint64_t id) const { return id < capacity() && has_page(page_of(id)) && present_[page_of(id)][row_of(id)]; }
  size_t n_points() const { return n_points_; }
  size_t n_pages() const { return n_pages_; }
  // a page on the device: its rows, then one presence byte per row
  size_t page_bytes() const { return (size_t)rpp_ * (kMpRowBytes + 1); }
  size_t presence_offset() const { return (size_t)rpp_ * kMpRowBytes; }

  // May these n ids be upserted with this field mask?  *at: the index of the entry that is refused.  new_pages: the pages (ascending,
  // each once) that do not exist yet.  Nothing changes.
  MpVerdict check_upsert(size_t n, const uint64_t* ids, uint32_t fields, std::vector<uint32_t>* new_pages, size_t* at = nullptr) const {
    size_t dummy = 0;
    size_t& where = at ? *at : dummy;
    where = 0;
    new_pages->clear();
    if (fields == 0 || (fields & ~(uint32_t)MP_FIELD_ALL)) return MpVerdict::bad_mask;
    for (size_t i = 0; i < n; ++i) {
      where = i;
      if (ids[i] >= capacity()) return MpVerdict::capacity;
      if (fields != MP_FIELD_ALL && !has(ids[i])) return MpVerdict::partial_first;
    }
    std::vector<std::pair<uint64_t, size_t>> sorted(n);
    for (size_t i = 0; i < n; ++i) sorted[i] = {ids[i], i};
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < n; ++i)
      if (sorted[i].first == sorted[i - 1].first) return where = sorted[i].second, MpVerdict::duplicate;
    for (size_t i = 0; i < n; ++i) {  // (ascending ids: ascending pages)
      const uint32_t p = page_of(sorted[i].first);
      if (!has_page(p) && (new_pages->empty() || new_pages->back() != p)) new_pages->push_back(p);
    }
    where = 0;
    return MpVerdict::ok;
  }
  void add_page(uint32_t p) {
    if (p >= max_pages_ || has_page(p)) return;
    present_[p].assign(rpp_, 0);
    ++n_pages_;
  }
  // after a check_upsert that said ok and add_page for every page it listed
  void commit_upsert(size_t n, const uint64_t* ids) {
    for (size_t i = 0; i < n; ++i) {
      uint8_t& b = present_[page_of(ids[i])][row_of(ids[i])];
      n_points_ += b ? 0 : 1;
      b = 1;
    }
  }
  bool erase(uint64_t id) {
    if (!has(id)) return false;
    present_[page_of(id)][row_of(id)] = 0;
    --n_points_;
    return true;
  }

 private:
  uint32_t rpp_, max_pages_;
  std::vector<std::vector<uint8_t>> present_;  // [page][row]; an empty vector: the page does not exist
  size_t n_points_ = 0, n_pages_ = 0;
};
