// lm6_dev.h -- what the one-vertex Levenberg-Marquardt kernels share (k_pose.hip's register-resident OptimizePoseOnly, k_sim3opt.hip's
// OptimizeSim3): a 6-DoF vertex gives both the same 21 + 6 sums per linearisation, the same damped 6x6 solve, the same computeScale and
// the same table of trial dampings (lm6_trial_lambda, next to the reject rule it unrolls: lm_ctrl.h).  Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "lm_ctrl.h"
#include "wave_ops.h"

namespace orbfe {

#define LM6_TRIALS LM_TRIALS
#define LM6_STAGE_LD(NT) ((NT) + 8)  // doubles per row of the staged sums: rows 8 double-banks apart => the readers of a wave 2 per bank pair

// (H + lambda I) x = b with H and b where they are (LDS), for the register-resident kernel, where this lane-0 solve and the pose update
// behind it are the longest serial piece of a pass (9 k of its ~20 k cycles: ~33 fp64 divisions and square roots of ~100 dependent cycles
// each): one reciprocal square root per pivot -- v_rsq_f64 and a third-order correction y0 (1 + e / 2 + 3 e^2 / 8), e = 1 - s y0^2, error
// below double rounding -- L_ii = s y, and every division by L_ii a multiplication by y.
__device__ __forceinline__ bool solve6_lambda(const double* H, double lambda, const double* b, double* x) {
#pragma clang fp contract(off)
  double L[36], inv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = (i == j) ? H[6 * i + j] + lambda : H[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k];
      if (i == j) {
        if (!(s > 0) || !isfinite(s)) return false;
        const double y0 = __builtin_amdgcn_rsq(s);
        const double e = fma(-(s * y0), y0, 1.0);
        const double y = fma(y0 * e, fma(0.375, e, 0.5), y0);
        L[6 * i + i] = s * y;
        inv[i] = y;
      } else
        L[6 * i + j] = s * inv[j];
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[6 * i + k] * y[k];
    y[i] = s * inv[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * x[k];
    x[i] = s * inv[i];
  }
  return true;
}

// computeScale of a 6-vector step: sum of x_j (lambda x_j + b_j), j = 0 .. 5 (the 1e-3 is lm_decide's)
__device__ __forceinline__ double lm6_scale(const double* x, double lambda, const double* b) {
#pragma clang fp contract(off)
  double scale = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) scale += x[j] * (lambda * x[j] + b[j]);
  return scale;
}

// max |H_jj| of the 6x6 system, j = 0 .. 5: what computeLambdaInit scales tau by
// (the callers pass it to lm_begin_iteration at every iteration, which reads it at iteration 0: the compiler computed the scan
//  unconditionally and selected on `it == 0` when it stood under that test too -- the same instructions either way)
__device__ __forceinline__ double lm6_maxdiag(const double* H) {
  double md = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) md = fmax(fabs(H[7 * j]), md);
  return md;
}

// The 27 sums of the normal equations over the NT threads of the workgroup (acc: the 21 entries of H's upper triangle row by row, then
// the 6 of b) into S.H (6x6, both triangles) and S.b; S.stage: 27 * LM6_STAGE_LD(NT) doubles, all in LDS.  Every thread runs it; H and b
// are valid behind it.
// Every thread stages its 27 partial sums; NT / 32 threads per sum add 32 staged values each (ascending), a fixed tree joins
// them: 27 + 32 LDS accesses and ~36 additions per thread, where 27 wave trees of data-parallel-primitive moves took as long as
// the edges' arithmetic (6.7 k of a build's 13.5 k cycles with 256 threads).  The last lane of each group of PARTS (8: half a row of 16,
// 16: a row) ends up with the group's sum; k -> (a, c2), a <= c2, in the order the sums were laid out.
// (A macro, not a function: as an inlined function the same statements gave k_pose_only_reg<512> another 15 spilled registers.)
#define LM6_STAGE_REDUCE(NT, acc, S, tid)                                                        \
  {                                                                                              \
    constexpr int PARTS = (NT) / 32, LD = LM6_STAGE_LD(NT);                                      \
    _Pragma("unroll") for (int k = 0; k < 27; ++k) S.stage[k * LD + tid] = acc[k];               \
    __syncthreads();                                                                             \
    if (tid < 27 * PARTS) {                                                                      \
      const int k = tid / PARTS, part = tid % PARTS;                                             \
      const double* row = S.stage + k * LD + part;                                               \
      double sm = 0;                                                                             \
      _Pragma("unroll") for (int j = 0; j < 32; ++j) sm += row[PARTS * j];                       \
      sm += dpp_f64<ORBFE_DPP_ROW_SHR(1), 0xf>(sm);                                              \
      sm += dpp_f64<ORBFE_DPP_ROW_SHR(2), 0xf>(sm);                                              \
      sm += dpp_f64<ORBFE_DPP_ROW_SHR(4), 0xf>(sm);                                              \
      if (PARTS == 16) sm += dpp_f64<ORBFE_DPP_ROW_SHR(8), 0xf>(sm);                             \
      if (part == PARTS - 1) {                                                                   \
        if (k >= 21) {                                                                           \
          S.b[k - 21] = sm;                                                                      \
        } else {                                                                                 \
          int a = 0, rem = k;                                                                    \
          while (rem >= 6 - a) rem -= 6 - a, ++a;                                                \
          const int c2 = a + rem;                                                                \
          S.H[6 * a + c2] = sm;                                                                  \
          S.H[6 * c2 + a] = sm;                                                                  \
        }                                                                                        \
      }                                                                                          \
    }                                                                                            \
    __syncthreads();                                                                             \
  }

}  // namespace orbfe
