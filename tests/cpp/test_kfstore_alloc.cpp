// The keyframe store's host-side bookkeeping (orb_slam2_ros2_amd/csrc/kfstore_alloc.h: slab allocator and id map) on its own: no HIP, so
// the host compiler and its sanitizers take it (tests/test_kfstore_abi.py builds it with -fsanitize=address,undefined where available).
// A deterministic random walk of insertions and erasures with the store's rules checked after every step.  Exit code 0 and "OK".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kfstore_alloc.h"

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);    \
      return 1;                                               \
    }                                                         \
  } while (0)

struct Entry {
  KfBlock blk;
  uint64_t stamp = 0;
};

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

static std::vector<KfBlock> blocks(const KfIdMap<Entry>& m) {
  std::vector<KfBlock> v;
  m.for_each([&](uint64_t, const Entry& e) { v.push_back(e.blk); });
  return v;
}

static bool take(KfSlabAlloc& a, size_t bytes, KfBlock* b, size_t* slabs_added) {
  if (a.take(bytes, b)) return true;
  a.add_slab(a.slab_size_for(bytes));
  ++*slabs_added;
  return a.take(bytes, b);
}

int main() {
  const size_t slab = 1 << 20;
  KfSlabAlloc a(slab);
  KfIdMap<Entry> map;
  size_t slabs_added = 0;
  CHECK(KfSlabAlloc::round(0) == 256 && KfSlabAlloc::round(1) == 256 && KfSlabAlloc::round(256) == 256 && KfSlabAlloc::round(257) == 512);

  // a dozen 161 KB entries cross several slabs; no block spans a slab, none moves
  std::vector<KfBlock> first;
  for (uint64_t id = 0; id < 12; ++id) {
    Entry e;
    CHECK(take(a, 161024, &e.blk, &slabs_added));
    CHECK(e.blk.off + e.blk.bytes <= slab && e.blk.bytes == 161024);
    CHECK(map.insert(id, e) != nullptr);
    first.push_back(e.blk);
    CHECK(a.consistent(blocks(map)));
  }
  CHECK(slabs_added == 2 && a.reserved_bytes() == 2 * slab);  // six 161 KB entries per 1 MB slab
  for (uint64_t id = 0; id < 12; ++id) CHECK(map.find(id)->blk.slab == first[id].slab && map.find(id)->blk.off == first[id].off);

  // a present id changes nothing
  {
    Entry e;
    e.stamp = 99;
    CHECK(map.insert(3, e) == nullptr && map.find(3)->stamp == 0 && map.size() == 12);
  }
  // erase two in the middle: their space is reused by the next entries of that size, and merged for a larger one
  Entry gone;
  CHECK(map.erase(4, &gone));
  CHECK(!a.give(gone.blk));
  const KfBlock hole4 = gone.blk;
  CHECK(map.erase(5, &gone));
  CHECK(!a.give(gone.blk));
  CHECK(!map.erase(5, &gone) && !map.find(4));  // unknown ids are ignored
  CHECK(a.consistent(blocks(map)));
  {
    Entry e;
    CHECK(take(a, 2 * 161024, &e.blk, &slabs_added));  // needs the two holes merged
    CHECK(e.blk.slab == hole4.slab && e.blk.off == hole4.off && slabs_added == 2);
    CHECK(map.insert(100, e) != nullptr);
    CHECK(a.consistent(blocks(map)));
  }
  // an entry larger than a slab gets a slab of its own, which goes back whole
  {
    Entry e;
    CHECK(take(a, 3 * slab + 5, &e.blk, &slabs_added));
    CHECK(slabs_added == 3 && e.blk.off == 0 && e.blk.bytes == KfSlabAlloc::round(3 * slab + 5) && a.slab_size((size_t)e.blk.slab) == e.blk.bytes);
    CHECK(map.insert(200, e) != nullptr);
    CHECK(a.consistent(blocks(map)));
    const size_t reserved = a.reserved_bytes();
    CHECK(map.erase(200, &gone));
    CHECK(a.give(gone.blk));  // true: the owner frees the slab's memory
    CHECK(!a.slab_live((size_t)gone.blk.slab) && a.reserved_bytes() == reserved - gone.blk.bytes);
    CHECK(a.consistent(blocks(map)));
    Entry f;
    CHECK(take(a, 1000, &f.blk, &slabs_added) && slabs_added == 3);  // (small blocks never land in a slab of its own)
    CHECK(map.insert(201, f) != nullptr);
  }
  // random walk
  uint64_t next_id = 1000;
  std::vector<uint64_t> live;
  for (int step = 0; step < 20000; ++step) {
    const uint32_t r = rnd();
    if (live.empty() || (r & 3) != 0) {
      const size_t bytes = (r >> 8) % 50 == 0 ? slab + (r >> 16) : 1 + (r >> 10) % 300000;
      Entry e;
      e.stamp = next_id;
      CHECK(take(a, bytes, &e.blk, &slabs_added));
      CHECK(e.blk.bytes == KfSlabAlloc::round(bytes));
      CHECK(map.insert(next_id, e) != nullptr);
      live.push_back(next_id++);
    } else {
      const size_t k = (r >> 4) % live.size();
      CHECK(map.erase(live[k], &gone) && gone.stamp == live[k]);
      a.give(gone.blk);
      live[k] = live.back();
      live.pop_back();
    }
    if (step % 64 == 0) CHECK(a.consistent(blocks(map)));
  }
  CHECK(a.consistent(blocks(map)));
  for (uint64_t id : live) {
    CHECK(map.erase(id, &gone));
    a.give(gone.blk);
  }
  for (uint64_t id : {0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 100, 201}) {
    CHECK(map.erase(id, &gone));
    a.give(gone.blk);
  }
  CHECK(map.size() == 0 && a.used_bytes() == 0 && a.consistent({}));
  std::printf("OK %zu slabs, %zu bytes reserved\n", slabs_added, a.reserved_bytes());
  return 0;
}
