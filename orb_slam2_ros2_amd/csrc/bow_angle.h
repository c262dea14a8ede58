// bow_angle.h -- the two rules of ORBMatcher::verifyAngle (ORBMatcher.cc:1013-1051) that decide which matches survive: the bin of a
// pair of angles and the choice of the three bins.  No HIP header: k_bowsearch.hip compiles this text for the device and
// tests/cpp/test_bow_angle.cpp compiles the same text with the host compiler alone (and with its sanitizers).
//   bin     diff = angle_q - angle_t in float; a negative diff becomes 360 + diff (which can round to 360.0f); bin = (int)(diff / 12.f);
//           bin 30 becomes 0.  Angles outside what an extractor gives (NaN, |diff| of 360 and more) have no defined bin in the reference
//           (it indexes its histogram unchecked); here they fall into bin 0, so that no count is ever written outside the 30 bins.
//   choice  three rounds of "the first strictly largest bin among those not yet chosen, empty bins never": a mask of the chosen bins.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BOW_ANGLE_FN __host__ __device__ inline
#else
#define BOW_ANGLE_FN inline
#endif

#define BOW_ANGLE_BINS 30    // ORBMatcher::mnBinNum
#define BOW_ANGLE_CHOOSE 3   // ORBMatcher::mnBinChoose

BOW_ANGLE_FN int bow_angle_bin(float angle_q, float angle_t) {
  float diff = angle_q - angle_t;
  diff = diff >= 0 ? diff : 360 + diff;
  const float b = diff / (float)(360 / BOW_ANGLE_BINS);
  if (!(b >= 0.f && b < (float)BOW_ANGLE_BINS)) return 0;  // [30, 31) is the reference's bin 30 -> 0; the rest: see above
  return (int)b;
}

// count[BOW_ANGLE_BINS] -> bit i set: bin i is kept
BOW_ANGLE_FN uint32_t bow_angle_choose(const int32_t* count) {
  uint32_t chosen = 0;
  for (int round = 0; round < BOW_ANGLE_CHOOSE; ++round) {
    int32_t best = 0;
    int best_id = -1;
    for (int i = 0; i < BOW_ANGLE_BINS; ++i)
      if (!((chosen >> i) & 1u) && count[i] > best) best = count[i], best_id = i;
    if (best_id >= 0) chosen |= 1u << best_id;
  }
  return chosen;
}
