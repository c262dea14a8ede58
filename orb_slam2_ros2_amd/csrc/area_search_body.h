// area_search_body.h -- findFeaturesInArea (src/Frame.cc:286-311) + getBestMatch (src/ORBMatcher.cc:967-990) of ONE query as one wave
// runs it over a finished area grid (area_grid_body.h): rows outer, columns inner, index order inside a cell; the candidates that pass
// the caller's filter wait in LDS until 64 of them make a chunk of the order-dependent fold (match_fold.h).  The one area loop of every
// guided matcher: k_guided.hip's k_search_area, k_fuse.hip's k_fuse_search, both kernels of k_sim3search.hip and k_fusepoints.hip's
// k_fusepts_search; they differ in their
// filter (where a candidate's octave comes from, and what else excludes it), their prologue and their acceptance test, which stay with
// them.  Every loop is bounded by the grid size or a cell's feature count.
#pragma once
#include "area_grid_body.h"
#include "match_fold.h"
#include "orbfe_internal.h"

namespace orbfe {

// A frame as the search reads it: its descriptors, its finished grid and the grid's geometry (search_area_layout.h: AreaGrid).
struct AreaTarget {
  const uint8_t* desc;
  const int32_t *cell_off, *cell_feat;
  int32_t rows, cols, clip_w, clip_h;
};

// stage: this wave's 128 LDS words.  pass(id): the caller's complete filter on target feature id -- the octave window included --
// evaluated exactly once per occurrence of id in the query's window, by the lane that holds the candidate (k_search_area counts there).
// Returns the number of candidates folded; b holds (best, second best, index of the first best).
template <class Pass>
__device__ __forceinline__ int area_fold(const AreaTarget& T, float x, float y, float rad, const uint4 a0, const uint4 a1, int32_t* stage,
                                         int lane, Best2& b, Pass pass) {
  const int rows = T.rows, cols = T.cols;
  const int min_x = max(0, __float2int_rn(x - rad)), max_x = min(T.clip_w, __float2int_rn(x + rad));
  const int min_y = max(0, __float2int_rn(y - rad)), max_y = min(T.clip_h, __float2int_rn(y + rad));
  const int c0 = max(0, min(cols - 1, cvfloor_f((float)min_x / (float)AREA_GRID_W))), c1 = min(cols - 1, cvfloor_f((float)max_x / (float)AREA_GRID_W));
  const int r0 = max(0, min(rows - 1, cvfloor_f((float)min_y / (float)AREA_GRID_H))), r1 = min(rows - 1, cvfloor_f((float)max_y / (float)AREA_GRID_H));
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
        bool ok = false;
        if (j < end) {
          id = T.cell_feat[j];
          ok = pass(id);
        }
        const unsigned long long m = __ballot(ok);
        if (ok) stage[staged + __popcll(m & ((1ull << lane) - 1ull))] = id;  // (staged < 64 here: at most 127 words)
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
