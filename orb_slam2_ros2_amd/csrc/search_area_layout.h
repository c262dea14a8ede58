// search_area_layout.h -- the grid geometry, the LDS rule of the grid build (every host file that launches one) and the scratch layout of
// the grid-guided search (orbfe_guided.hip: search_area_core and the callers that reserve for it).  Host only, like scratch_layout.h: tests/cpp/test_scratch_layout.cpp checks that a reservation sized from
// the layout is exactly what the search then takes.
#pragma once
#include <cmath>

#include "scratch_layout.h"

static inline int cv_ceil_f(float v) { return (int)v + ((int)v < v); }  // OpenCV's cvCeil

// grid of a frame: VirtualFrame::initGrid (Frame.cc:55-56) sizes it from the undistorted bounds, findFeaturesInArea clips the box at
// (int)mfMaxU / (int)mfMaxV (:291-293).  bounds = {min_u, max_u, min_v, max_v}; NULL: the image itself (no distortion: 0, width, 0, height)
struct AreaGrid {
  int rows, cols, clip_w, clip_h;
};
static inline bool area_grid(int width, int height, const float* bounds, AreaGrid* g) {
  if (!bounds) {
    *g = {(height + 47) / 48, (width + 63) / 64, width, height};
    return true;
  }
  if (!(std::isfinite(bounds[0]) && std::isfinite(bounds[1]) && std::isfinite(bounds[2]) && std::isfinite(bounds[3])) ||
      !(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2]) || bounds[1] > 65536.f || bounds[3] > 65536.f || bounds[1] < 1.f || bounds[3] < 1.f)
    return false;
  *g = {cv_ceil_f((float)(bounds[3] - bounds[2]) / 48), cv_ceil_f((float)(bounds[1] - bounds[0]) / 64), (int)bounds[1], (int)bounds[3]};
  return g->rows >= 1 && g->cols >= 1;
}

// The LDS of the grid build (area_grid_body.h: one workgroup per grid), the one rule of every caller: the [ncells + 1] offsets and
// [ncells] counters always live there -- a grid whose counters exceed 60 KB is refused; the [n] unordered lists and the [n] cells of
// the features join them while everything fits 56 KB, else the lists are filled and sorted in the scratch block.  bytes: the dynamic
// LDS of the launch (the 4 KB scan array of the kernel is static).
struct AreaGridLds {
  bool refused;
  int in_lds;
  size_t bytes;
};
static inline AreaGridLds area_grid_lds(size_t ncells, size_t n) {
  const size_t counters = (2 * ncells + 1) * sizeof(int32_t), lists = n * 2 * sizeof(int32_t);
  const bool in_lds = counters + lists <= 56 * 1024;
  return {counters > 60 * 1024, in_lds ? 1 : 0, in_lds ? counters + lists : counters};
}

// Queries first (they continue the caller's uploaded block, if any, so that everything goes up as ONE copy through the page-locked
// staging buffer), then the grid, then the results (one download): ten copies from / to pageable memory were most of a 0.2 ms call.
struct SearchAreaLayout {
  AreaGrid grid;
  ScratchRegion in, out;
  size_t o_q, o_r, o_lo, o_hi, o_d, o_ex;       // in: query positions, radii, level windows, descriptors | the targets' exclusion flags
  size_t o_co, o_cf;                            // device only: the grid's cell offsets and feature lists
  size_t o_bi, o_bd, o_sd, o_nc, o_eh;          // out: best index, best and second distance, candidate count | hits on excluded targets
  size_t end() const { return out.end; }  // (the results are the last block)
};
static inline SearchAreaLayout search_area_layout(size_t start, const AreaGrid& ag, size_t n_target, size_t nq) {
  const size_t ncells = (size_t)ag.rows * ag.cols;
  ScratchLayout L(start);
  SearchAreaLayout l;
  l.grid = ag;
  l.o_q = L.open(l.in).take<float>(nq * 2), l.o_r = L.take<float>(nq), l.o_lo = L.take(nq), l.o_hi = L.take(nq), l.o_d = L.take(nq * 32);
  l.o_ex = L.take(n_target);
  l.o_co = L.close(l.in).take<int32_t>(ncells + 1);  // k_grid_build writes cell_off[0 .. ncells], k_search_area reads cell_off[cell + 1]
  l.o_cf = L.take<int32_t>(n_target);
  l.o_bi = L.open(l.out).take<int32_t>(nq), l.o_bd = L.take<int32_t>(nq), l.o_sd = L.take<int32_t>(nq), l.o_nc = L.take<int32_t>(nq);
  l.o_eh = L.take<int32_t>(n_target);
  L.close(l.out);
  return l;
}
