// scratch_layout.h -- how the host entry points carve one block of device scratch (and its page-locked mirror) into arrays.  Host only: no
// HIP header, so tests/cpp/test_scratch_layout.cpp compiles it with the host compiler alone.  The one padding rule: every take starts on a
// 256-byte boundary and occupies at least 8 bytes, so an empty array still has an address of its own.
//   ScratchLayout L;  ScratchRegion up, down;        // (L(used): continue behind a caller's block)
//   const size_t o_a = L.open(up).take<float>(n), o_b = L.take(bytes), o_r = L.close(up).open(down).take<int32_t>(n);
//   L.close(down);                                   // reserve L.end() bytes; copy [up.begin, up.end) up, [down.begin, down.end) down
#pragma once
#include <cstddef>
#include <utility>

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// a contiguous run of takes: what one copy or one fill covers
struct ScratchRegion {
  size_t begin = 0, end = 0;
  size_t bytes() const { return end - begin; }
  ScratchRegion upto(size_t e) const { return {begin, e}; }  // its front, up to offset e (a field's offset, or one past its data)
};

struct ScratchLayout {
  size_t off;
  explicit ScratchLayout(size_t start = 0) : off(start) {}
  size_t take(size_t bytes) { return std::exchange(off, off + align_up(bytes < 8 ? 8 : bytes, 256)); }
  template <typename T>
  size_t take(size_t count) { return take(count * sizeof(T)); }
  size_t end() const { return off; }
  ScratchLayout& open(ScratchRegion& r) { return r.begin = r.end = off, *this; }  // r starts with the next take ..
  ScratchLayout& close(ScratchRegion& r) { return r.end = off, *this; }           // .. and ends with the last one
};
