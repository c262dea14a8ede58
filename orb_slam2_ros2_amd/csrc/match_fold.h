// match_fold.h -- getBestMatch's (ORBMatcher.cc:967-990) best / second-best fold over a candidate list, 64 candidates at a time in list
// order (k_match.hip's header comment states the order-free form), and the Hamming-256 distance.  Shared by k_match.hip and k_tri.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbfe {

#define ORB_INT_MAX 2147483647

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_min_step(int v) {
  // lanes without a source keep INT_MAX (the identity of min)
  return min(v, __builtin_amdgcn_update_dpp(ORB_INT_MAX, v, CTRL, ROW_MASK, 0xf, false));
}
// inclusive prefix-min over the 64 lanes (all lanes active): Hillis-Steele inside each row of 16 with DPP row
// shifts, then the row totals are broadcast into the following rows.  Lane 63 holds the wave minimum.
__device__ __forceinline__ int wave_incl_prefix_min(int v) {
  v = dpp_min_step<0x111, 0xf>(v);  // row_shr:1
  v = dpp_min_step<0x112, 0xf>(v);  // row_shr:2
  v = dpp_min_step<0x114, 0xf>(v);  // row_shr:4
  v = dpp_min_step<0x118, 0xf>(v);  // row_shr:8
  v = dpp_min_step<0x142, 0xa>(v);  // row_bcast:15 -> rows 1,3
  v = dpp_min_step<0x143, 0xc>(v);  // row_bcast:31 -> rows 2,3
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) { return __builtin_amdgcn_readlane(wave_incl_prefix_min(v), 63); }

struct Best2 {
  int min_d, second, min_idx;
};

// Fold one chunk of up to 64 candidates (lane order = list order) into the running (min, idx, second).
// d = distance of this lane's candidate or INT_MAX if the lane holds none; idx = its train index.
__device__ __forceinline__ void fold_chunk(Best2& b, int d, int idx, int lane) {
  const int incl = wave_incl_prefix_min(d);
  const int excl = __builtin_amdgcn_update_dpp(ORB_INT_MAX, incl, 0x138, 0xf, 0xf, false);  // wave_shr:1, lane 0 <- INT_MAX
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
