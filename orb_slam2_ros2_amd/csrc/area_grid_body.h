// area_grid_body.h -- the area grid of one frame or keyframe (VirtualFrame::initGrid, src/Frame.cc:53-69) by one workgroup of
// AREA_GRID_NT threads: the one grid build, the body of k_grid_build (k_guided.hip: an image slot), k_fuse_grid (k_fuse.hip: a fuse
// target) and k_kfstore_pack (k_kfstore.hip: a stored keyframe, once, at insertion).  The grid is sized from the frame's own bounds
// (search_area_layout.h: AreaGrid), and its LDS by the one host rule there (area_grid_lds).
#pragma once
#include <hip/hip_runtime.h>

#include "orbfe_internal.h"

#define AREA_GRID_W 64
#define AREA_GRID_H 48
#define AREA_GRID_NT 1024

namespace orbfe {

__device__ __forceinline__ int cvfloor_f(float v) {
  const int i = (int)v;
  return i - (i > v);
}
// cell of a coordinate: cvFloor(v / size) as Frame.cc:64-65, clamped to the grid at BOTH ends.  The reference indexes its vector of
// cells unchecked (a negative or too large undistorted coordinate is undefined behaviour there); here such a feature lands in the
// border cell, and a non-finite coordinate in cell 0, so that no index leaves the LDS counters or the scratch lists.
__device__ __forceinline__ int grid_cell(float v, int size, int n) {
  const float q = v / (float)size;
  if (!(q > 0.0f)) return 0;              // negative, -0, NaN
  if (q >= (float)(n - 1)) return n - 1;  // beyond the last cell, +inf
  return cvfloor_f(q);
}

// cell_off[ncells + 1], cell_feat[n] (a cell's features in ascending index) of the n keypoints kps.  l_grid: the workgroup's dynamic
// LDS, [ncells + 1] offsets, [ncells] counts / fill cursors, then (feat_in_lds) the [n] unordered lists and the [n] cells of the
// features; l_scan: AREA_GRID_NT words of LDS.  Every thread of the workgroup calls it.
__device__ __forceinline__ void area_grid_build(const orbfe_keypoint* __restrict__ kps, int n, int rows, int cols, int feat_in_lds,
                                                int32_t* __restrict__ cell_off, int32_t* __restrict__ cell_feat, int32_t* l_grid,
                                                int32_t* l_scan) {
  const int tid = threadIdx.x;
  const int ncells = rows * cols;
  int32_t* l_off = l_grid;
  int32_t* l_cur = l_grid + ncells + 1;
  int32_t* feat = feat_in_lds ? l_cur + ncells : cell_feat;
  int32_t* l_cell = feat + n;  // (feat_in_lds only)
  for (int c = tid; c < ncells; c += AREA_GRID_NT) l_cur[c] = 0;
  __syncthreads();
  // The coordinates are read ONCE (a thread's loads independent of each other) and the cell kept in LDS: with 256 threads each of the
  // three passes below walked eight dependent trips to memory, ~1 us each -- 24 of this kernel's 27 us.
  for (int i = tid; i < n; i += AREA_GRID_NT) {
    const int cell = grid_cell(kps[i].y, AREA_GRID_H, rows) * cols + grid_cell(kps[i].x, AREA_GRID_W, cols);
    if (feat_in_lds) l_cell[i] = cell;
    atomicAdd(&l_cur[cell], 1);
  }
  __syncthreads();
  // exclusive prefix over the cells: a thread sums a run of consecutive cells, the run totals are scanned, the thread writes its run's offsets
  const int per = (ncells + AREA_GRID_NT - 1) / AREA_GRID_NT;
  const int c0 = min(tid * per, ncells), c1 = min(c0 + per, ncells);
  int local = 0;
  for (int c = c0; c < c1; ++c) local += l_cur[c];
  l_scan[tid] = local;
  __syncthreads();
  for (int o = 1; o < AREA_GRID_NT; o <<= 1) {
    const int v = tid >= o ? l_scan[tid - o] : 0;
    __syncthreads();
    l_scan[tid] += v;
    __syncthreads();
  }
  {
    int acc = l_scan[tid] - local;
    for (int c = c0; c < c1; ++c) {
      const int k = l_cur[c];
      l_off[c] = acc;
      l_cur[c] = 0;
      acc += k;
    }
    if (tid == AREA_GRID_NT - 1) l_off[ncells] = l_scan[AREA_GRID_NT - 1];
  }
  __syncthreads();
  for (int c = tid; c <= ncells; c += AREA_GRID_NT) cell_off[c] = l_off[c];
  for (int i = tid; i < n; i += AREA_GRID_NT) {
    const int cell = feat_in_lds ? l_cell[i] : grid_cell(kps[i].y, AREA_GRID_H, rows) * cols + grid_cell(kps[i].x, AREA_GRID_W, cols);
    feat[l_off[cell] + atomicAdd(&l_cur[cell], 1)] = i;
  }
  __syncthreads();
  // the reference pushes indices in ascending order (Frame.cc:61-68)
  if (feat_in_lds) {
    // every feature finds its place in its cell's list by counting the smaller indices there: the work of a sort, spread over the threads
    // (one thread sorting the densest cell of a clustered frame was the long pole of the per-cell sort below)
    for (int i = tid; i < n; i += AREA_GRID_NT) {
      const int cell = l_cell[i];
      const int b = l_off[cell], k = l_off[cell + 1] - b;
      int rank = 0;
      for (int j = 0; j < k; ++j) rank += feat[b + j] < i ? 1 : 0;
      cell_feat[b + rank] = i;
    }
    return;
  }
  for (int c = tid; c < ncells; c += AREA_GRID_NT) {
    int32_t* L = feat + l_off[c];
    const int k = l_off[c + 1] - l_off[c];
    for (int a = 1; a < k; ++a) {
      const int32_t v = L[a];
      int b = a - 1;
      while (b >= 0 && L[b] > v) {
        L[b + 1] = L[b];
        --b;
      }
      L[b + 1] = v;
    }
  }
}

}  // namespace orbfe
