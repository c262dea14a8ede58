// k_sim3.hip -- Sim3Solver's Horn alignment and inlier test (src/Sim3Solver.cc) for a speculated schedule of Ransac<Sim3Ret>::iterate
// calls.  checkInliers clears the list, modelFunc always writes and the scale is fixed (S1, S2), so a hypothesis and its own refine
// depend on nothing but the draw: one kernel, k_sim3_hyp, one wave per hypothesis --
//   the 3-point modelFunc (every lane the same registers), the inlier test with lanes on correspondences and one ballot per 64, and,
//   only where the count exceeds mnMinInlier, refine: modelFunc over the wave's own inlier list (compacted through LDS 256 entries at a
//   time; the 6 centroid sums, then the 9 sums of M, one lane per sum, sequential in list order) and its inlier test.
// Numerics (restated in tests/sim3_restatement.py, which this file must equal bit for bit): float without contraction as
// the reference's CV_32F Mats, gemm's alpha / beta in double, the 4x4 eigen-problem by jacobi_small<4> on N promoted to double.
#include <hip/hip_runtime.h>

#include "orbfe_internal.h"

#pragma clang fp contract(off)

namespace {

#define SIM3_WG 64
#define SIM3_MAX_WORDS 1024  // mask words of ORBFE_BOW_MAX_FEATURES (65535) correspondences
#define SIM3_CH_WORDS 4      // mask words compacted into LDS per chunk
#define SIM3_CH (64 * SIM3_CH_WORDS)

struct Sim3Cam {
  float fx, fy, cx, cy;
};

struct Sim3Lds {
  uint64_t mask[SIM3_MAX_WORDS];
  float pq[SIM3_CH][6];
};

#include "jacobi_dev.h"

__device__ __forceinline__ float canon(float v) { return v != v ? __uint_as_float(0x7FC00000u) : v; }

// (float)(alpha * (double)(r . x) + (double)t): cv::gemm's alpha / beta on a float row sum, left to right
__device__ __forceinline__ float affine_row(double alpha, float r0, float r1, float r2, float x0, float x1, float x2, float t) {
  const float s = (r0 * x0 + r1 * x1) + r2 * x2;
  return (float)(alpha * (double)s + (double)t);
}

// Mat / n: times 1.0 / n in double
__device__ __forceinline__ float div_n(float sum, int n) { return (float)((double)sum * (1.0 / (double)(float)n)); }

// regroupN, computeRotation (the largest eigenvalue's eigenvector as the quaternion (w, x, y, z), Eigen's normalize and toRotationMatrix
// in float), s = 1, t = Oq - s R Op.  Every lane runs it on the same values.
__device__ void horn(const float (&M)[9], const float (&Op)[3], const float (&Oq)[3], float (&m)[12]) {
  const float Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7], Szz = M[8];
  double N[4][4], V[4][4];
  N[0][0] = (double)((Sxx + Syy) + Szz);
  N[1][1] = (double)((Sxx - Syy) - Szz);
  N[2][2] = (double)((-Sxx + Syy) - Szz);
  N[3][3] = (double)((-Sxx - Syy) + Szz);
  N[0][1] = N[1][0] = (double)(Syz - Szy);
  N[0][2] = N[2][0] = (double)(Szx - Sxz);
  N[0][3] = N[3][0] = (double)(Sxy - Syx);
  N[1][2] = N[2][1] = (double)(Sxy + Syx);
  N[1][3] = N[3][1] = (double)(Szx + Sxz);
  N[2][3] = N[3][2] = (double)(Syz + Szy);
  jacobi_small<4>(N, V);
  double bv = N[0][0];
  float w = (float)V[0][0], x = (float)V[1][0], y = (float)V[2][0], z = (float)V[3][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (N[k][k] > bv) {
      bv = N[k][k];
      w = (float)V[0][k];
      x = (float)V[1][k];
      y = (float)V[2][k];
      z = (float)V[3][k];
    }
  const float nrm = sqrtf(((x * x + y * y) + z * z) + w * w);
  w = w / nrm;
  x = x / nrm;
  y = y / nrm;
  z = z / nrm;
  const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * x, txy = ty * x, txz = tz * x;
  const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
  m[0] = 1.0f - (tyy + tzz);
  m[1] = txy - twz;
  m[2] = txz + twy;
  m[3] = txy + twz;
  m[4] = 1.0f - (txx + tzz);
  m[5] = tyz - twx;
  m[6] = txz - twy;
  m[7] = tyz + twx;
  m[8] = 1.0f - (txx + tyy);
#pragma unroll
  for (int r = 0; r < 3; ++r) m[9 + r] = affine_row(-1.0, m[3 * r], m[3 * r + 1], m[3 * r + 2], Op[0], Op[1], Op[2], Oq[r]);
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = canon(m[i]);
}

// Sim3Solver::checkInliers for the model m: mask words [0, words) to gmask and S.mask, returns the count (the same on every lane)
__device__ int check_wave(Sim3Lds& S, const float (&m)[12], int n, int words, const float* __restrict__ pq, const float* __restrict__ px,
                          const float* __restrict__ thr, Sim3Cam cam, uint64_t* __restrict__ gmask, int lane) {
  // Spq = Sqp.inv(): R^T, -(R^T t)
  const float i0 = -((m[0] * m[9] + m[3] * m[10]) + m[6] * m[11]);
  const float i1 = -((m[1] * m[9] + m[4] * m[10]) + m[7] * m[11]);
  const float i2 = -((m[2] * m[9] + m[5] * m[10]) + m[8] * m[11]);
  int cnt = 0;
  for (int w = 0; w < words; ++w) {
    const int i = w * 64 + lane;
    bool in = false;
    if (i < n) {
      const float* p = pq + 6 * (int64_t)i;
      const float P0 = p[0], P1 = p[1], P2 = p[2], Q0 = p[3], Q1 = p[4], Q2 = p[5];
      const float* x = px + 4 * (int64_t)i;
      // Sqp * P3d -> Q2d_
      const float a0 = affine_row(1.0, m[0], m[1], m[2], P0, P1, P2, m[9]);
      const float a1 = affine_row(1.0, m[3], m[4], m[5], P0, P1, P2, m[10]);
      const float a2 = affine_row(1.0, m[6], m[7], m[8], P0, P1, P2, m[11]);
      // Spq * Q3d -> P2d_
      const float b0 = affine_row(1.0, m[0], m[3], m[6], Q0, Q1, Q2, i0);
      const float b1 = affine_row(1.0, m[1], m[4], m[7], Q0, Q1, Q2, i1);
      const float b2 = affine_row(1.0, m[2], m[5], m[8], Q0, Q1, Q2, i2);
      const float qu = cam.fx * (a0 / a2) + cam.cx, qv = cam.fy * (a1 / a2) + cam.cy;
      const float pu = cam.fx * (b0 / b2) + cam.cx, pv = cam.fy * (b1 / b2) + cam.cy;
      const float dpu = pu - x[0], dpv = pv - x[1], dqu = qu - x[2], dqv = qv - x[3];
      const float eP = (float)((double)dpu * (double)dpu + (double)dpv * (double)dpv);
      const float eQ = (float)((double)dqu * (double)dqu + (double)dqv * (double)dqv);
      in = !(eP > thr[2 * (int64_t)i]) && !(eQ > thr[2 * (int64_t)i + 1]);  // a NaN error is an inlier, as in the reference
    }
    const unsigned long long b = __ballot(in);
    if (lane == 0) {
      gmask[w] = b;
      S.mask[w] = b;
    }
    cnt += __popcll(b);
  }
  __syncthreads();
  return cnt;
}

// compact the inliers of mask words [w0, w0 + SIM3_CH_WORDS) into S.pq in list order; returns how many
__device__ int stage_chunk(Sim3Lds& S, int w0, int words, const float* __restrict__ pq, int lane) {
  int k = 0;
#pragma unroll
  for (int d = 0; d < SIM3_CH_WORDS; ++d) {
    const int w = w0 + d;
    const unsigned long long b = w < words ? S.mask[w] : 0ull;
    if ((b >> lane) & 1ull) {
      const int pos = k + __popcll(b & ((1ull << lane) - 1ull));
      const float* p = pq + 6 * (int64_t)(w * 64 + lane);
#pragma unroll
      for (int c = 0; c < 6; ++c) S.pq[pos][c] = p[c];
    }
    k += __popcll(b);
  }
  __syncthreads();
  return k;
}

__global__ __launch_bounds__(SIM3_WG) void k_sim3_hyp(const Sim3Hyp* __restrict__ hyps, const RansacProb* __restrict__ probs,
                                                      const float* __restrict__ pq, const float* __restrict__ px,
                                                      const float* __restrict__ thr, Sim3Cam cam, Sim3Out* __restrict__ out,
                                                      uint64_t* __restrict__ masks, uint64_t* __restrict__ ref_masks) {
  __shared__ Sim3Lds S;
  const int lane = threadIdx.x, h = blockIdx.x;
  const Sim3Hyp H = hyps[h];
  const RansacProb pr = probs[H.prob];
  const float* PQ = pq + 6 * (int64_t)pr.off;
  const float* PX = px + 4 * (int64_t)pr.off;
  const float* T = thr + 2 * (int64_t)pr.off;
  float model[12];
  {  // modelFunc of the sample
    const float* a = PQ + 6 * (int64_t)H.idx[0];
    const float* b = PQ + 6 * (int64_t)H.idx[1];
    const float* c = PQ + 6 * (int64_t)H.idx[2];
    float O[6], A[6], B[6], C[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      O[i] = div_n(((0.0f + a[i]) + b[i]) + c[i], 3);
      A[i] = a[i] - O[i];
      B[i] = b[i] - O[i];
      C[i] = c[i] - O[i];
    }
    float M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) M[3 * i + j] = (A[i] * A[3 + j] + B[i] * B[3 + j]) + C[i] * C[3 + j];
    const float Op[3] = {O[0], O[1], O[2]}, Oq[3] = {O[3], O[4], O[5]};
    horn(M, Op, Oq, model);
  }
  const int cnt = check_wave(S, model, pr.n, pr.words, PQ, PX, T, cam, masks + H.mask_off, lane);
  Sim3Out& o = out[h];
  const bool refine = cnt > pr.min_inlier;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) o.model[i] = model[i];
    o.count = cnt;
    o.refined = refine ? 1 : 0;
    o.ref_count = 0;
    o.pad = 0;
  }
  if (!refine) return;
  // refine: modelFunc over the inlier list.  Lane l < 6 sums component l of (P, Q) from 0; then lane e < 9 sums M[e / 3][e % 3] from
  // its first term.
  float acc = 0.0f;
  for (int w0 = 0; w0 < pr.words; w0 += SIM3_CH_WORDS) {
    const int k = stage_chunk(S, w0, pr.words, PQ, lane);
    if (lane < 6)
      for (int i = 0; i < k; ++i) acc = acc + S.pq[i][lane];
    __syncthreads();
  }
  const float ctr = div_n(acc, cnt);
  float Op[3], Oq[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Op[i] = __shfl(ctr, i, 64);
    Oq[i] = __shfl(ctr, 3 + i, 64);
  }
  const int e = lane < 9 ? lane : 0, ei = e / 3, ej = e % 3;
  const float cp = ei == 0 ? Op[0] : (ei == 1 ? Op[1] : Op[2]);
  const float cq = ej == 0 ? Oq[0] : (ej == 1 ? Oq[1] : Oq[2]);
  acc = 0.0f;
  bool first = true;
  for (int w0 = 0; w0 < pr.words; w0 += SIM3_CH_WORDS) {
    const int k = stage_chunk(S, w0, pr.words, PQ, lane);
    if (lane < 9)
      for (int i = 0; i < k; ++i) {
        const float t = (S.pq[i][ei] - cp) * (S.pq[i][3 + ej] - cq);
        acc = first ? t : acc + t;
        first = false;
      }
    __syncthreads();
  }
  float M[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) M[i] = __shfl(acc, i, 64);
  horn(M, Op, Oq, model);
  const int rc = check_wave(S, model, pr.n, pr.words, PQ, PX, T, cam, ref_masks + H.mask_off, lane);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) o.ref_model[i] = model[i];
    o.ref_count = rc;
  }
}

}  // namespace

void launch_sim3(hipStream_t st, const Sim3Hyp* hyps, int n_hyp, const RansacProb* probs, const float* pq, const float* px, const float* thr,
                 const float cam[4], Sim3Out* out, uint64_t* masks, uint64_t* ref_masks) {
  const Sim3Cam c{cam[0], cam[1], cam[2], cam[3]};
  if (n_hyp > 0)
    hipLaunchKernelGGL(k_sim3_hyp, dim3((unsigned)n_hyp), dim3(SIM3_WG), 0, st, hyps, probs, pq, px, thr, c, out, masks, ref_masks);
}
