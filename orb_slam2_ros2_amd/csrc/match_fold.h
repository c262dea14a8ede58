// match_fold.h -- getBestMatch's (ORBMatcher.cc:967-990) best / second-best fold over a candidate list, 64 candidates at a time in list
// order (k_match.hip's header comment states the order-free form), and the Hamming-256 distance.  The one fold: k_match.hip, k_tri.hip,
// bow_walk.h and the area search of every guided matcher (area_search_body.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_ops.h"

namespace orbfe {

#define ORB_INT_MAX 2147483647

// one step of a min scan (k_match.hip's row-of-16 scan takes the first four); lanes without a source keep INT_MAX
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_min_step(int v) {
  return dpp_step<OpMinI, CTRL, ROW_MASK>(v);
}
// inclusive prefix-min over the 64 lanes (all lanes active; wave_ops.h: the one DPP scan).  Lane 63 holds the wave minimum.
__device__ __forceinline__ int wave_incl_prefix_min(int v) { return wave_incl_scan_dpp<OpMinI>(v); }
__device__ __forceinline__ int wave_min_i(int v) { return wave_reduce_dpp<OpMinI>(v); }

struct Best2 {
  int min_d, second, min_idx;
};

// Fold one chunk of up to 64 candidates (lane order = list order) into the running (min, idx, second).
// d = distance of this lane's candidate or INT_MAX if the lane holds none; idx = its train index.
__device__ __forceinline__ void fold_chunk(Best2& b, int d, int idx, int lane) {
  const int incl = wave_incl_prefix_min(d);
  const int excl = __builtin_amdgcn_update_dpp(ORB_INT_MAX, incl, ORBFE_DPP_WAVE_SHR1, 0xf, 0xf, false);  // lane 0 <- INT_MAX
  const int pre = min(b.min_d, excl);
  const bool record = d < pre;  // strict prefix-minimum record: becomes the new best, never the second best
  b.second = min(b.second, wave_min_i(record ? ORB_INT_MAX : d));
  const int cmin = __builtin_amdgcn_readlane(incl, 63);
  if (cmin < b.min_d) {
    const unsigned long long m = __ballot(d == cmin);
    b.min_d = cmin;
    b.min_idx = __builtin_amdgcn_readlane(idx, __ffsll((long long)m) - 1);
  }
}

__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint8_t* __restrict__ p) {
  const uint4 b0 = *(const uint4*)p;
  const uint4 b1 = *(const uint4*)(p + 16);
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
         __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

}  // namespace orbfe
