// bow_walk.h -- the inner part of ORBMatcher::searchByBow (ORBMatcher.cc:183-235) for ONE FeatureVector entry of the train side, as one
// wave runs it: the node the entry belongs to, that node in the other FeatureVector, and getBestMatch over the node's features of that
// other side that pass a flag filter (match_fold.h, 64 candidates at a time in list order).  Shared by k_tri.hip (bAddMPs on both sides,
// fixed threshold and ratio) and k_bowsearch.hip (the filter by mode); the filter is a parameter: skip(flag byte) -> leave the feature out.
#pragma once
#include "match_fold.h"

namespace orbfe {

// the node of entry j in a FeatureVector's CSR: the last i with offs[i] <= j (n_nodes >= 1, 0 <= j < offs[n_nodes])
__device__ __forceinline__ int bow_entry_node(const int32_t* __restrict__ offs, int n_nodes, int j) {
  int lo = 0, hi = n_nodes - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// where `node` sits in the ascending list nodes[0 .. n_nodes), or -1
__device__ __forceinline__ int bow_find_node(const uint32_t* __restrict__ nodes, int n_nodes, uint32_t node) {
  int a = 0, e = n_nodes;
  while (a < e) {
    const int mid = (a + e) >> 1;
    if (nodes[mid] < node) a = mid + 1;
    else e = mid;
  }
  return (a < n_nodes && nodes[a] == node) ? a : -1;
}

// getBestMatch of the descriptor (a0, a1) over feat[begin .. end) of the other side, features whose flag byte the filter skips left out.
// All 64 lanes of the wave call it with the same arguments; b starts as {INT_MAX, INT_MAX, 0}.  Returns the number of candidates.
template <class Skip>
__device__ __forceinline__ int bow_fold_node(Best2& b, const uint4 a0, const uint4 a1, const uint32_t* __restrict__ feat, int begin, int end,
                                             const uint8_t* __restrict__ desc, const uint8_t* __restrict__ flags, Skip skip, int lane) {
  int ncand = 0;
  for (int c0 = begin; c0 < end; c0 += 64) {
    const int c = c0 + lane;
    int d = ORB_INT_MAX, idx = 0;
    bool has = false;
    if (c < end) {
      const uint32_t f = feat[c];
      if (!skip(flags[f])) {
        idx = (int)f;
        d = hamming256(a0, a1, desc + (size_t)f * 32);
        has = true;
      }
    }
    ncand += __popcll(__ballot(has));
    fold_chunk(b, d, idx, lane);
  }
  return ncand;
}

// the filter of bAddMPs (both sides): a feature whose map point is good AND in the map is left out
struct SkipGoodInMap {
  __device__ __forceinline__ bool operator()(uint8_t fl) const { return (fl & 3) == 3; }
};

}  // namespace orbfe
