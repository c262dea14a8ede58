// staged_rows.h -- how many bytes of a caller's strided image may be read, and the copy that stages them.  Host only: no HIP header, so
// tests/cpp/test_staged_rows.cpp compiles it with the host compiler and its sanitizers.  The one rule: an image of `rows` rows, `stride`
// bytes apart, `row_bytes` live bytes each, ends with the last live byte of its LAST row -- stride * (rows - 1) + row_bytes, not
// stride * rows.  A column range of a larger image (a cv::Mat ROI: Mat::step is the parent's) has nothing of its own behind that byte, and
// when the range touches the parent's last column the allocation ends there.
#pragma once
#include <cstddef>
#include <cstring>

static inline size_t staged_rows_bytes(size_t stride, size_t rows, size_t row_bytes) { return rows ? stride * (rows - 1) + row_bytes : 0; }

// does a read of `bytes` bytes from offset `first` stay inside a block of `block_bytes`?
static inline bool staged_rows_within(size_t first, size_t bytes, size_t block_bytes) { return first <= block_bytes && bytes <= block_bytes - first; }

// The rows keep their stride in the staging buffer (the reader indexes them by it): one copy from the first row's first byte to the last
// row's last live byte.  Returns the bytes copied.
static inline size_t stage_rows(void* dst, const void* src, size_t stride, size_t rows, size_t row_bytes) {
  const size_t n = staged_rows_bytes(stride, rows, row_bytes);
  if (n) std::memcpy(dst, src, n);
  return n;
}
