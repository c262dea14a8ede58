// test_staged_rows.cpp -- csrc/staged_rows.h, host only (no HIP header, no device): the byte count of a strided image and the copy that
// stages it, on a source that is a column range of a larger image whose allocation ENDS with the range's last element.  Built with the
// host compiler's address and undefined-behaviour sanitizers by tests/test_abi_and_host.py: one byte read past the block aborts the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orb_slam2_ros2_amd/csrc/staged_rows.h"

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// a parent image of `cols` elements per row, of which the block holds everything up to the last element of the range [x0, x0 + w) of the
// last row -- what is left of a parent whose range touches its last column, or of any parent as far as the range owns it
template <typename T>
static void roi_case(size_t cols, size_t rows, size_t x0, size_t w) {
  const size_t stride = cols * sizeof(T), row_bytes = w * sizeof(T);
  const size_t block_bytes = stride * (rows - 1) + (x0 + w) * sizeof(T);
  uint8_t* block = (uint8_t*)std::malloc(block_bytes);  // (malloc: the sanitizer's red zone starts at block + block_bytes)
  for (size_t i = 0; i < block_bytes; ++i) block[i] = (uint8_t)(i * 131u + 7u);
  const uint8_t* roi = block + x0 * sizeof(T);
  const size_t first = x0 * sizeof(T);

  const size_t n = staged_rows_bytes(stride, rows, row_bytes);
  CHECK(n == stride * (rows - 1) + row_bytes);
  CHECK(staged_rows_within(first, n, block_bytes));       // the rule ends exactly with the block ..
  CHECK(first + n == block_bytes);
  CHECK(!staged_rows_within(first, n + 1, block_bytes));  // .. and one byte more does not
  // the count the staging sites used before (stride * rows) leaves the block whenever a row has anything behind the range
  const size_t old_bytes = stride * rows;
  CHECK(staged_rows_within(first, old_bytes, block_bytes) == (stride == row_bytes && x0 == 0));
  if (stride > row_bytes) CHECK(old_bytes - n == stride - row_bytes);

  std::vector<uint8_t> stage(old_bytes + 64, 0xEE);
  const size_t copied = stage_rows(stage.data(), roi, stride, rows, row_bytes);
  CHECK(copied == n);
  for (size_t y = 0; y < rows; ++y)  // the reader's indexing: row y at y * stride
    CHECK(std::memcmp(stage.data() + y * stride, roi + y * stride, row_bytes) == 0);
  bool untouched_behind = true;  // nothing is written behind the last row's last element
  for (size_t i = n; i < stage.size(); ++i) untouched_behind = untouched_behind && stage[i] == 0xEE;
  CHECK(untouched_behind);
  std::free(block);
}

int main() {
  CHECK(staged_rows_bytes(100, 0, 10) == 0);  // no rows: nothing, not stride * (0 - 1) + ..
  CHECK(staged_rows_bytes(100, 1, 10) == 10);
  CHECK(staged_rows_bytes(640, 480, 640) == 640 * 480);  // a contiguous image: the whole of it
  CHECK(staged_rows_within(0, 0, 0) && staged_rows_within(5, 0, 5) && !staged_rows_within(6, 0, 5));
  CHECK(!staged_rows_within(1, (size_t)-1, 16));  // first + bytes would wrap
  uint8_t none = 0;
  CHECK(stage_rows(&none, nullptr, 100, 0, 10) == 0 && none == 0);

  roi_case<uint16_t>(341, 257, 3, 333);  // the column range of tests/test_gpu_input_shapes.py: big[:, 3:3 + w] of an (h, w + 8) image
  roi_case<float>(341, 257, 3, 333);
  roi_case<uint16_t>(341, 257, 8, 333);  // touching the parent's last column
  roi_case<float>(1035, 96, 3, 1027);
  roi_case<uint16_t>(648, 480, 5, 640);
  roi_case<uint16_t>(640, 480, 0, 640);  // contiguous: both counts agree
  roi_case<float>(9, 1, 2, 4);           // one row

  if (failures) return 1;
  std::printf("STAGED_ROWS_OK\n");
  return 0;
}
