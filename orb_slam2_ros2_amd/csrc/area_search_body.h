// area_search_body.h -- findFeaturesInArea (src/Frame.cc:286-311) + getBestMatch (src/ORBMatcher.cc:967-990) of ONE query as one wave
// runs it over a keyframe's finished area grid: rows outer, columns inner, index order inside a cell; the candidates that pass the octave
// window and the caller's per-feature filter wait in LDS until 64 of them make a chunk of the order-dependent fold (match_fold.h).  The
// loop of k_fuse.hip's k_fuse_search and k_guided.hip's k_search_area (those two stay as they are: their tests are the yardstick), as a
// body for the kernels that come after them (k_sim3search.hip).  Every loop is bounded by the grid size or a cell's feature count.
#pragma once
#include "fuse_grid_body.h"
#include "match_fold.h"
#include "orbfe_internal.h"

namespace orbfe {

// A keyframe as the search reads it: the arrays of a stored keyframe (orbfe_kfstore.h: KfEntry) and its grid geometry.
struct AreaTarget {
  const orbfe_keypoint* kps;
  const uint8_t* desc;
  const int32_t *cell_off, *cell_feat;
  int32_t rows, cols, clip_w, clip_h;
};

// stage: this wave's 128 LDS words.  keep(id): the caller's filter on target feature id (evaluated by the lane that holds the candidate).
// Returns the number of candidates folded; b holds (best, second best, index of the first best).
template <class Keep>
__device__ __forceinline__ int area_fold(const AreaTarget& T, float x, float y, float rad, int lo, int hi, const uint4 a0, const uint4 a1,
                                         int32_t* stage, int lane, Best2& b, Keep keep) {
  const int rows = T.rows, cols = T.cols;
  const int min_x = max(0, __float2int_rn(x - rad)), max_x = min(T.clip_w, __float2int_rn(x + rad));
  const int min_y = max(0, __float2int_rn(y - rad)), max_y = min(T.clip_h, __float2int_rn(y + rad));
  const int c0 = max(0, min(cols - 1, cvfloor_f((float)min_x / (float)FUSE_GRID_W))), c1 = min(cols - 1, cvfloor_f((float)max_x / (float)FUSE_GRID_W));
  const int r0 = max(0, min(rows - 1, cvfloor_f((float)min_y / (float)FUSE_GRID_H))), r1 = min(rows - 1, cvfloor_f((float)max_y / (float)FUSE_GRID_H));
  const uint8_t* __restrict__ desc = T.desc;
  int staged = 0, total = 0;
  auto flush = [&](int count) {  // stage[0 .. count) (count <= 64) as one chunk
    const int idx = (lane < count) ? stage[lane] : 0;
    const int d = (lane < count) ? hamming256(a0, a1, desc + (size_t)idx * 32) : ORB_INT_MAX;
    fold_chunk(b, d, idx, lane);
  };
  for (int r = r0; r <= r1; ++r)
    for (int c = c0; c <= c1; ++c) {
      const int beg = T.cell_off[r * cols + c], end = T.cell_off[r * cols + c + 1];
      for (int j0 = beg; j0 < end; j0 += 64) {
        const int j = j0 + lane;
        int id = 0;
        bool pass = false;
        if (j < end) {
          id = T.cell_feat[j];
          const int oc = T.kps[id].octave;
          pass = oc <= hi && oc >= lo && keep(id);
        }
        const unsigned long long m = __ballot(pass);
        if (pass) stage[staged + __popcll(m & ((1ull << lane) - 1ull))] = id;  // (staged < 64 here: at most 127 words)
        staged += __popcll(m);
        total += __popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (staged >= 64) {
          flush(64);
          const int rest = (lane < staged - 64) ? stage[64 + lane] : 0;
          __builtin_amdgcn_wave_barrier();
          if (lane < staged - 64) stage[lane] = rest;
          staged -= 64;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  if (staged > 0) flush(staged);
  return total;
}

}  // namespace orbfe
