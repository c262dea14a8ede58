// The map-point store's host-side bookkeeping (orb_slam2_ros2_amd/csrc/mpstore_index.h: the paged direct index and its presence map) on
// its own: no HIP, so the host compiler and its sanitizers take it (tests/test_mpstore_host.py builds it with
// -fsanitize=address,undefined where available).  Page and row arithmetic at the page edges, the duplicate check, the first-upsert mask
// rule, the capacity rule, and that a refused upsert changes nothing.  Exit code 0 and "OK".
#include <cstdio>
#include <vector>

#include "mpstore_index.h"

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);    \
      return 1;                                               \
    }                                                         \
  } while (0)

static MpVerdict upsert(MpIndex& ix, const std::vector<uint64_t>& ids, uint32_t fields, std::vector<uint32_t>* pages = nullptr, size_t* at = nullptr) {
  std::vector<uint32_t> np;
  const MpVerdict v = ix.check_upsert(ids.size(), ids.data(), fields, &np, at);
  if (pages) *pages = np;
  if (v != MpVerdict::ok) return v;
  for (uint32_t p : np) ix.add_page(p);
  ix.commit_upsert(ids.size(), ids.data());
  return v;
}

int main() {
  // rows_per_page = 64, max_pages = 8: ids 0 .. 511
  MpIndex ix(64, 8);
  CHECK(ix.capacity() == 512 && ix.page_bytes() == 64 * 65 && ix.presence_offset() == 64 * 64);
  const uint64_t edge[] = {0, 1, 63, 64, 65, 127, 128, 300, 511};
  const uint32_t page[] = {0, 0, 0, 1, 1, 1, 2, 4, 7}, row[] = {0, 1, 63, 0, 1, 63, 0, 44, 63};
  for (int i = 0; i < 9; ++i) CHECK(ix.page_of(edge[i]) == page[i] && ix.row_of(edge[i]) == row[i] && !ix.has(edge[i]));
  CHECK(!ix.has(512) && !ix.has(~0ull) && !ix.has_page(8) && !ix.has_page(~0u));

  // the first upsert, shuffled: five new pages, ascending and each once
  std::vector<uint32_t> pages;
  CHECK(upsert(ix, {300, 63, 511, 0, 128, 65, 1, 127, 64}, MP_FIELD_ALL, &pages) == MpVerdict::ok);
  CHECK((pages == std::vector<uint32_t>{0, 1, 2, 4, 7}) && ix.n_pages() == 5 && ix.n_points() == 9);
  for (uint64_t id : edge) CHECK(ix.has(id));
  CHECK(!ix.has(2) && !ix.has(62) && !ix.has(66) && !ix.has(129) && !ix.has(299) && !ix.has(301) && !ix.has(510) && !ix.has(192));

  // a present id takes any mask, and needs no page; an absent one only the full mask
  size_t at = 99;
  for (uint32_t m = 1; m <= 7; ++m) CHECK(upsert(ix, {511, 0}, m, &pages, &at) == MpVerdict::ok && pages.empty());
  CHECK(ix.n_points() == 9);
  for (uint32_t m = 1; m < 7; ++m) {
    CHECK(upsert(ix, {0, 2, 63}, m, nullptr, &at) == MpVerdict::partial_first && at == 1);  // page exists, row absent
    CHECK(upsert(ix, {64, 65, 200}, m, nullptr, &at) == MpVerdict::partial_first && at == 2);  // page absent
  }
  CHECK(upsert(ix, {0}, 0) == MpVerdict::bad_mask && upsert(ix, {0}, 8) == MpVerdict::bad_mask && upsert(ix, {0}, 15) == MpVerdict::bad_mask);

  // duplicates: adjacent, apart, of a present and of an absent id -- refused whatever the mask allows
  CHECK(upsert(ix, {1, 1}, MP_FIELD_ALL, nullptr, &at) == MpVerdict::duplicate);
  CHECK(upsert(ix, {7, 1, 8, 7}, MP_FIELD_ALL, nullptr, &at) == MpVerdict::duplicate && (at == 0 || at == 3));
  CHECK(upsert(ix, {511, 0, 64, 511}, MP_FIELD_POS) == MpVerdict::duplicate);

  // capacity: the first id past the last row, and ids whose page number does not fit 32 bits
  CHECK(upsert(ix, {3, 512}, MP_FIELD_ALL, nullptr, &at) == MpVerdict::capacity && at == 1);
  CHECK(upsert(ix, {~0ull}, MP_FIELD_ALL) == MpVerdict::capacity && upsert(ix, {1ull << 40, 0}, MP_FIELD_POS) == MpVerdict::capacity);

  // none of the refusals changed anything
  CHECK(ix.n_pages() == 5 && ix.n_points() == 9);
  for (uint64_t id = 0; id < 520; ++id) {
    bool in = false;
    for (uint64_t e : edge) in = in || e == id;
    CHECK(ix.has(id) == in);
  }

  // erase: only what is there; the page stays; the id comes back with the full mask only
  CHECK(ix.erase(64) && !ix.erase(64) && !ix.erase(2) && !ix.erase(200) && !ix.erase(512) && !ix.erase(~0ull));
  CHECK(!ix.has(64) && ix.has(65) && ix.n_points() == 8 && ix.n_pages() == 5);
  CHECK(upsert(ix, {64}, MP_FIELD_DESC) == MpVerdict::partial_first);
  CHECK(upsert(ix, {64}, MP_FIELD_ALL, &pages) == MpVerdict::ok && pages.empty() && ix.n_points() == 9);

  // fill it: every row of every page, then nothing is left to add but everything may be updated
  std::vector<uint64_t> all(512);
  for (size_t i = 0; i < all.size(); ++i) all[i] = 511 - i;
  CHECK(upsert(ix, all, MP_FIELD_ALL, &pages) == MpVerdict::ok && (pages == std::vector<uint32_t>{3, 5, 6}) && ix.n_points() == 512 && ix.n_pages() == 8);
  CHECK(upsert(ix, all, MP_FIELD_POS) == MpVerdict::ok && ix.n_points() == 512);

  // the default geometry, an odd one, and the empty call
  MpIndex big;
  CHECK(big.rows_per_page() == 16384 && big.max_pages() == 4096 && big.capacity() == 67108864ull);
  CHECK(big.page_of(67108863ull) == 4095 && big.row_of(67108863ull) == 16383 && big.page_of(16384) == 1 && big.row_of(16384) == 0);
  CHECK(upsert(big, {67108863ull}, MP_FIELD_ALL, &pages) == MpVerdict::ok && (pages == std::vector<uint32_t>{4095}) && big.has(67108863ull));
  CHECK(upsert(big, {67108864ull}, MP_FIELD_ALL) == MpVerdict::capacity);
  MpIndex odd(7, 3);
  CHECK(odd.capacity() == 21 && odd.page_of(20) == 2 && odd.row_of(20) == 6 && odd.page_of(7) == 1 && odd.row_of(6) == 6);
  CHECK(upsert(odd, {20, 6, 7}, MP_FIELD_ALL, &pages) == MpVerdict::ok && (pages == std::vector<uint32_t>{0, 1, 2}));
  CHECK(upsert(odd, {21}, MP_FIELD_ALL) == MpVerdict::capacity);
  CHECK(upsert(odd, {}, MP_FIELD_ALL, &pages) == MpVerdict::ok && pages.empty() && odd.n_points() == 3);
  MpIndex none(64, 0);
  CHECK(none.capacity() == 0 && !none.has(0) && upsert(none, {0}, MP_FIELD_ALL) == MpVerdict::capacity);
  std::printf("OK\n");
  return 0;
}
