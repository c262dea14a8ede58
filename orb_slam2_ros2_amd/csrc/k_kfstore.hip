// k_kfstore.hip -- the one launch of an insertion into the keyframe store (orbfe_kfstore.hip).
//
// k_kfstore_pack  workgroup 0 builds the entry's area grid from the source keypoints (area_grid_body.h: the one grid build, so a
//                 stored grid is what orbfe_fuse_into_keyframes and the guided searches build per call); workgroups 1 .. (add_from_slot only) copy the
//                 extraction slot's arrays -- keypoints and descriptors at the slot's stride, right_u and depth at the pair's -- into
//                 the entry's packed block, or write -1 where the keyframe has no stereo columns.
// No workgroup waits on another (the grid is built from the SOURCE keypoints, not from the copy); every loop is bounded by the feature
// count or the grid size; the result does not depend on the number of copy workgroups.
#include <hip/hip_runtime.h>

#include "area_grid_body.h"
#include "orbfe_internal.h"

namespace {

using namespace orbfe;

__global__ __launch_bounds__(AREA_GRID_NT) void k_kfstore_pack(KfPack A) {
  extern __shared__ __attribute__((aligned(16))) int32_t l_grid[];  // (area_grid_body.h)
  __shared__ int32_t l_scan[AREA_GRID_NT];
  if (blockIdx.x == 0) {
    area_grid_build(A.s_kps, A.n, A.rows, A.cols, A.in_lds, A.cell_off, A.cell_feat, l_grid, l_scan);
    return;
  }
  const int t = (blockIdx.x - 1) * AREA_GRID_NT + threadIdx.x, step = A.n_copy * AREA_GRID_NT;
  static_assert(sizeof(orbfe_keypoint) == 28, "a keypoint is seven 32-bit words");
  const uint32_t* __restrict__ sk = (const uint32_t*)A.s_kps;
  uint32_t* __restrict__ dk = (uint32_t*)A.kps;
  for (int w = t; w < A.n * 7; w += step) dk[w] = sk[w];
  const uint4* __restrict__ sd = (const uint4*)A.s_desc;
  uint4* __restrict__ dd = (uint4*)A.desc;
  for (int w = t; w < A.n * 2; w += step) dd[w] = sd[w];
  for (int i = t; i < A.n; i += step) {
    A.depth[i] = A.s_depth ? A.s_depth[i] : -1.0;
    A.right_u[i] = A.s_right_u ? A.s_right_u[i] : -1.0;
  }
}

}  // namespace

// copy false: the features are in the entry already (A.s_kps == A.kps), only the grid is built
void launch_kfstore_pack(hipStream_t st, KfPack A, size_t grid_lds, bool copy) {
  // about four words (of 15 per feature) per copying thread, at most 16 workgroups: a 2000-feature keyframe is 160 KB
  A.n_copy = copy ? max(1, min(16, (A.n * 15 + 4 * AREA_GRID_NT - 1) / (4 * AREA_GRID_NT))) : 0;
  hipLaunchKernelGGL(k_kfstore_pack, dim3(1 + A.n_copy), dim3(AREA_GRID_NT), grid_lds, st, A);
}
