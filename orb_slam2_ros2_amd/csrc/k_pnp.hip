// k_pnp.hip -- PnPSolver's EPnP and inlier test (src/PnPSolver.cc) for a speculated schedule of Ransac<PnPRet>::iterate calls.
//
// Phase A (k_pnp_hyp): one wave per hypothesis -- the 4-point EPnP of its sample, then the float inlier test over the problem's points
// with lanes on points; out: pose, count, degenerate flag, inlier mask.  A "given" hypothesis skips EPnP and counts an entry pose.
// Phase B (k_pnp_call): one workgroup per iterate call.  It walks the call's hypotheses in order with the reference's running inlier list
// (P1: never cleared between hypotheses) and stale pose (P2: a degenerate sample recounts the previous pose) and runs refine -- EPnP over
// the list, duplicates included, then the inlier test -- wherever the count exceeds mnMinInlier, up to the first refine that succeeds.
//
// Numerics (restated in tests/pnp_restatement.py, which this file must equal bit for bit): fp64 without contraction, every
// sum sequential in list order starting from its first term; cyclic trig-free Jacobi for the symmetric eigen-problems (12x12 on 12 lanes
// through LDS, 3x3 / 4x4 on one lane), a selection sort to descending eigenvalues and the P7 sign rule; Cramer for the 3x3 solves;
// eigen-based pseudo-inverses for DECOMP_SVD; the pose rounded to float and the inlier test in float.
#include <hip/hip_runtime.h>

#include "orbfe_internal.h"

#pragma clang fp contract(off)

namespace {

#define PNP_CH 256         // list entries staged in LDS per chunk
#define PNP_SWEEPS 50      // Jacobi sweeps at most (jacobi12; the small ones: JAC_SWEEPS, the same)
#define PNP_NEGL_SWEEP 4   // from this sweep on, negligible off-diagonals are set to 0
#define PNP_HYP_WG 64
#define PNP_CALL_WG 256

struct PnpCam {
  float fx, fy, cx, cy;
};

struct PnpLds {
  double P[PNP_CH][3];
  double Q[PNP_CH][2];
  double al[PNP_CH][4];
  double M[144], V[144], lam[12];
  double acc[78];
  double vv[4][4][3], L[6][10], rho[6];  // the one-lane tail's larger arrays
  double c[3], ctl[4][3], m[9], invD;
  float pose[12];
  int degen, zdet, cnt;
  int idx[4];
  int64_t len;
};

__device__ __forceinline__ void entry_ab(int e, int& a, int& b) {  // e-th (a <= b) entry of a 12x12 upper triangle, row-major
  a = 0;
  int left = e;
  while (left >= 12 - a) {
    left -= 12 - a;
    ++a;
  }
  b = a + left;
}

#include "jacobi_dev.h"

template <int n>
__device__ void eig_sorted_small(double (&a)[n][n], double (&w)[n], double (&V)[n][n]) {
  jacobi_small<n>(a, V);
#pragma unroll
  for (int i = 0; i < n; ++i) w[i] = a[i][i];
#pragma unroll
  for (int p = 0; p < n - 1; ++p) {
    int best = p;
    double bv = w[p];
#pragma unroll
    for (int q = p + 1; q < n; ++q)
      if (w[q] > bv) {
        best = q;
        bv = w[q];
      }
#pragma unroll
    for (int q = p + 1; q < n; ++q)
      if (q == best) {
        const double tw = w[p];
        w[p] = w[q];
        w[q] = tw;
#pragma unroll
        for (int r = 0; r < n; ++r) {
          const double tv = V[r][p];
          V[r][p] = V[r][q];
          V[r][q] = tv;
        }
      }
  }
#pragma unroll
  for (int k = 0; k < n; ++k) {
    int bi = 0;
    double bv = fabs(V[0][k]);
#pragma unroll
    for (int j = 1; j < n; ++j)
      if (fabs(V[j][k]) > bv) {
        bi = j;
        bv = fabs(V[j][k]);
      }
    double piv = V[0][k];
#pragma unroll
    for (int j = 1; j < n; ++j)
      if (j == bi) piv = V[j][k];
    if (piv < 0)
#pragma unroll
      for (int j = 0; j < n; ++j) V[j][k] = -V[j][k];
  }
}

// x = pinv(N) g for a symmetric 4x4 N (eigenpairs with lam > 0 and lam > rel * max(lam), in Jacobi's order, x starting at 0)
__device__ void pinv_sym4(double (&N)[4][4], const double (&g)[4], double rel, double (&x)[4]) {
  double V[4][4];
  jacobi_small<4>(N, V);
  double lam[4] = {N[0][0], N[1][1], N[2][2], N[3][3]};
  double lmax = lam[0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (lam[k] > lmax) lmax = lam[k];
  const double tol = lmax * rel;
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool use = lam[k] > 0 && lam[k] > tol;
    const double proj = ((V[0][k] * g[0] + V[1][k] * g[1]) + V[2][k] * g[2]) + V[3][k] * g[3];
    const double coef = proj / lam[k];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (use) x[j] = x[j] + coef * V[j][k];
  }
}

__device__ __forceinline__ double dot3(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

__device__ void fullbeta(const double (&b)[4], double (&fb)[10]) {
  fb[0] = b[0] * b[0];
  fb[1] = b[1] * b[1];
  fb[2] = b[2] * b[2];
  fb[3] = b[3] * b[3];
  fb[4] = b[0] * b[1];
  fb[5] = b[0] * b[2];
  fb[6] = b[0] * b[3];
  fb[7] = b[1] * b[2];
  fb[8] = b[1] * b[3];
  fb[9] = b[2] * b[3];
}

__device__ void residual(const double (&L)[6][10], const double (&fb)[10], const double (&rho)[6], double (&r)[6]) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double s = L[c][0] * fb[0];
#pragma unroll
    for (int k = 1; k < 10; ++k) s = s + L[c][k] * fb[k];
    r[c] = s - rho[c];
  }
}

__device__ __forceinline__ float to_f32(double v) {
  const float f = (float)v;
  return f != f ? __uint_as_float(0x7FC00000u) : f;
}

// ---- block-level pieces -------------------------------------------------------------------------------------------------------
// 12x12 Jacobi on S.M / S.V: lanes 0..11 own rows; every thread of the block calls it
__device__ void jacobi12(PnpLds& S, int tid, int nt) {
  double* a = S.M;
  double* V = S.V;
  for (int i = tid; i < 144; i += nt) V[i] = (i / 12 == i % 12) ? 1.0 : 0.0;
  __syncthreads();
  for (int sweep = 0; sweep < PNP_SWEEPS; ++sweep) {
    bool off = false;
    for (int p = 0; p < 11; ++p)
      for (int q = p + 1; q < 12; ++q) off |= a[p * 12 + q] != 0;
    if (!off) break;
    for (int p = 0; p < 11; ++p)
      for (int q = p + 1; q < 12; ++q) {
        const double apq = a[p * 12 + q];
        if (apq == 0) continue;
        const double app = a[p * 13], aqq = a[q * 13];
        if (sweep >= PNP_NEGL_SWEEP) {
          const double g = 100.0 * fabs(apq);
          if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
            __syncthreads();
            if (tid == 0) {
              a[p * 12 + q] = 0.0;
              a[q * 12 + p] = 0.0;
            }
            __syncthreads();
            continue;
          }
        }
        const double theta = (aqq - app) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c), h = t * apq;
        double g = 0, hh = 0, gv = 0, hv = 0;
        if (tid < 12) {
          g = a[tid * 12 + p];
          hh = a[tid * 12 + q];
          gv = V[tid * 12 + p];
          hv = V[tid * 12 + q];
        }
        __syncthreads();
        if (tid < 12) {
          if (tid != p && tid != q) {
            const double np = g - s * (hh + g * tau), nq = hh + s * (g - hh * tau);
            a[tid * 12 + p] = np;
            a[p * 12 + tid] = np;
            a[tid * 12 + q] = nq;
            a[q * 12 + tid] = nq;
          }
          V[tid * 12 + p] = gv - s * (hv + gv * tau);
          V[tid * 12 + q] = hv + s * (gv - hv * tau);
          if (tid == 0) {
            a[p * 13] = app - h;
            a[q * 13] = aqq + h;
            a[p * 12 + q] = 0.0;
            a[q * 12 + p] = 0.0;
          }
        }
        __syncthreads();
      }
  }
  // descending selection sort (one lane), then the P7 sign rule (one lane per eigenvector)
  if (tid == 0) {
    for (int i = 0; i < 12; ++i) S.lam[i] = a[i * 13];
    for (int p = 0; p < 11; ++p) {
      int best = p;
      double bv = S.lam[p];
      for (int q = p + 1; q < 12; ++q)
        if (S.lam[q] > bv) {
          best = q;
          bv = S.lam[q];
        }
      const double tw = S.lam[p];
      S.lam[p] = S.lam[best];
      S.lam[best] = tw;
      for (int r = 0; r < 12; ++r) {
        const double tv = V[r * 12 + p];
        V[r * 12 + p] = V[r * 12 + best];
        V[r * 12 + best] = tv;
      }
    }
  }
  __syncthreads();
  if (tid < 12) {
    int bi = 0;
    double bv = fabs(V[tid]);
    for (int j = 1; j < 12; ++j)
      if (fabs(V[j * 12 + tid]) > bv) {
        bi = j;
        bv = fabs(V[j * 12 + tid]);
      }
    if (V[bi * 12 + tid] < 0)
      for (int j = 0; j < 12; ++j) V[j * 12 + tid] = -V[j * 12 + tid];
  }
  __syncthreads();
}

// stage list entries [base, base + k) as doubles
__device__ void stage(PnpLds& S, const int* list, int64_t base, int k, const float* xyz, const float* uv, bool with_uv, int tid, int nt) {
  for (int i = tid; i < k; i += nt) {
    const int j = list[base + i];
    S.P[i][0] = (double)xyz[3 * j];
    S.P[i][1] = (double)xyz[3 * j + 1];
    S.P[i][2] = (double)xyz[3 * j + 2];
    if (with_uv) {
      S.Q[i][0] = (double)uv[2 * j];
      S.Q[i][1] = (double)uv[2 * j + 1];
    }
  }
}

// the solver tail on one lane: L, rho, betas, Gauss-Newton, camera control points, ICP -> S.pose
__device__ void epnp_tail(PnpLds& S) {
  double(&v)[4][4][3] = S.vv;  // v[k][j] = point j of vMREVec[k] (eigenvector of the (k+1)-th smallest eigenvalue)
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int x = 0; x < 3; ++x) v[k][j][x] = S.V[(3 * j + x) * 12 + (11 - k)];
  double ctl[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int x = 0; x < 3; ++x) ctl[j][x] = S.ctl[j][x];
  const int PA[6] = {0, 0, 0, 1, 1, 2}, PB[6] = {1, 2, 3, 2, 3, 3};
  double(&L)[6][10] = S.L;
  double(&rho)[6] = S.rho;
#pragma unroll
  for (int row = 0; row < 6; ++row) {
    double x[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) x[k][c] = v[k][PA[row]][c] - v[k][PB[row]][c];
    L[row][0] = dot3(x[0], x[0]);
    L[row][1] = dot3(x[1], x[1]);
    L[row][2] = dot3(x[2], x[2]);
    L[row][3] = dot3(x[3], x[3]);
    L[row][4] = 2.0 * dot3(x[0], x[1]);
    L[row][5] = 2.0 * dot3(x[0], x[2]);
    L[row][6] = 2.0 * dot3(x[0], x[3]);
    L[row][7] = 2.0 * dot3(x[1], x[2]);
    L[row][8] = 2.0 * dot3(x[1], x[3]);
    L[row][9] = 2.0 * dot3(x[2], x[3]);
    double dd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dd[c] = ctl[PA[row]][c] - ctl[PB[row]][c];
    rho[row] = dot3(dd, dd);
  }
  const int C4[4] = {0, 4, 5, 6};
  double N4[4][4], g4[4], beta[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = L[0][C4[i]] * L[0][C4[j]];
#pragma unroll
      for (int r = 1; r < 6; ++r) s = s + L[r][C4[i]] * L[r][C4[j]];
      N4[i][j] = s;
    }
    double s = L[0][C4[i]] * rho[0];
#pragma unroll
    for (int r = 1; r < 6; ++r) s = s + L[r][C4[i]] * rho[r];
    g4[i] = s;
  }
  pinv_sym4(N4, g4, 1e-24, beta);
  if (beta[0] < 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) beta[i] = -beta[i];
  const double b1 = sqrt(beta[0]);
  beta[0] = b1;
  beta[1] = beta[1] / b1;
  beta[2] = beta[2] / b1;
  beta[3] = beta[3] / b1;
  // Gauss-Newton (GLOptimize)
  const int JI[4][4] = {{1, 5, 6, 7}, {5, 2, 8, 9}, {6, 8, 3, 10}, {7, 9, 10, 4}};
  double old = 3.4028234663852886e38;  // FLT_MAX
  for (int it = 0; it < 5; ++it) {
    double fb[10], J[4][6], r[6], Hm[4][4], g[4], d[4];
    fullbeta(beta, fb);
#pragma unroll
    for (int row = 0; row < 4; ++row)
#pragma unroll
      for (int col = 0; col < 6; ++col) {
        double tm[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) tm[i] = (i == row) ? (2.0 * L[col][JI[row][i] - 1]) * beta[i] : L[col][JI[row][i] - 1] * beta[i];
        J[row][col] = ((tm[0] + tm[1]) + tm[2]) + tm[3];
      }
    residual(L, fb, rho, r);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double s = J[i][0] * J[j][0];
#pragma unroll
        for (int c = 1; c < 6; ++c) s = s + J[i][c] * J[j][c];
        Hm[i][j] = s;
      }
      double s = J[i][0] * r[0];
#pragma unroll
      for (int c = 1; c < 6; ++c) s = s + J[i][c] * r[c];
      g[i] = -s;
    }
    pinv_sym4(Hm, g, 1e-12, d);
    const double nrm = sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]);
    if (nrm < 1e-4) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) beta[i] = beta[i] + d[i];
    fullbeta(beta, fb);
    residual(L, fb, rho, r);
    double e2 = r[0] * r[0];
#pragma unroll
    for (int c = 1; c < 6; ++c) e2 = e2 + r[c] * r[c];
    const double err = sqrt(e2);
    if (err > old) {
#pragma unroll
      for (int i = 0; i < 4; ++i) beta[i] = beta[i] - d[i];
      break;
    }
    old = err;
  }
  // camera control points and ICP
  double Cc[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int x = 0; x < 3; ++x) Cc[j][x] = ((beta[0] * v[0][j][x] + beta[1] * v[1][j][x]) + beta[2] * v[2][j][x]) + beta[3] * v[3][j][x];
  double cW[3], cC[3], Aw[4][3], Bc[4][3];
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    cW[x] = (((ctl[0][x] + ctl[1][x]) + ctl[2][x]) + ctl[3][x]) / 4.0;
    cC[x] = (((Cc[0][x] + Cc[1][x]) + Cc[2][x]) + Cc[3][x]) / 4.0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      Aw[j][x] = ctl[j][x] - cW[x];
      Bc[j][x] = Cc[j][x] - cC[x];
    }
  double Hx[3][3], Sm[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = Bc[0][i] * Aw[0][j];
#pragma unroll
      for (int k = 1; k < 4; ++k) s = s + Bc[k][i] * Aw[k][j];
      Hx[i][j] = s;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = Hx[0][i] * Hx[0][j];
#pragma unroll
      for (int k = 1; k < 3; ++k) s = s + Hx[k][i] * Hx[k][j];
      Sm[i][j] = s;
    }
  double lam3[3], V3[3][3];
  eig_sorted_small<3>(Sm, lam3, V3);
  double sig[3], U[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) sig[k] = lam3[k] > 0 ? sqrt(lam3[k]) : 0.0;
  bool ok[3];
  ok[0] = sig[0] > 0;
  ok[1] = ok[0] && sig[1] > sig[0] * 1e-12;
  ok[2] = ok[0] && sig[2] > sig[0] * 1e-12;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double hv = (Hx[r][0] * V3[0][k] + Hx[r][1] * V3[1][k]) + Hx[r][2] * V3[2][k];
      U[r][k] = ok[k] ? hv / sig[k] : 0.0;
    }
  if (!ok[2] && ok[1]) {
    const double c0 = U[1][0] * U[2][1] - U[2][0] * U[1][1], c1 = U[2][0] * U[0][1] - U[0][0] * U[2][1],
                 c2 = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    U[0][2] = c0;
    U[1][2] = c1;
    U[2][2] = c2;
  }
  double R[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) R[r][s] = (U[r][0] * V3[s][0] + U[r][1] * V3[s][1]) + U[r][2] * V3[s][2];
  const double det = (((((R[0][0] * R[1][1]) * R[2][2] + (R[0][1] * R[1][2]) * R[2][0]) + (R[0][2] * R[1][0]) * R[2][1]) -
                       (R[0][2] * R[1][1]) * R[2][0]) -
                      (R[0][1] * R[1][0]) * R[2][2]) -
                     (R[0][0] * R[1][2]) * R[2][1];
  if (det < 0)
#pragma unroll
    for (int s = 0; s < 3; ++s) R[2][s] = -R[2][s];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double t = cC[r] - ((R[r][0] * cW[0] + R[r][1] * cW[1]) + R[r][2] * cW[2]);
#pragma unroll
    for (int s = 0; s < 3; ++s) S.pose[3 * r + s] = to_f32(R[r][s]);
    S.pose[9 + r] = to_f32(t);
  }
}

// PnPSolver::modelFunc over list[0 .. len) (problem-local indices): S.degen, and S.pose when not degenerate.  Every thread calls it.
__device__ void epnp_block(PnpLds& S, const int* list, int64_t len, const float* xyz, const float* uv, PnpCam cam, int tid, int nt) {
  // 1. centroid
  double acc = 0;
  for (int64_t base = 0; base < len; base += PNP_CH) {
    const int k = (int)min<int64_t>(PNP_CH, len - base);
    stage(S, list, base, k, xyz, uv, false, tid, nt);
    __syncthreads();
    if (tid < 3)
      for (int i = 0; i < k; ++i) acc = (base + i == 0) ? S.P[i][tid] : acc + S.P[i][tid];
    __syncthreads();
  }
  if (tid < 3) S.c[tid] = acc / (double)len;
  __syncthreads();
  // 2. A^T A of the centred points (entries 00 01 02 11 12 22)
  const int EI[6] = {0, 0, 0, 1, 1, 2}, EJ[6] = {0, 1, 2, 1, 2, 2};
  const int ei = tid < 6 ? EI[tid] : 0, ej = tid < 6 ? EJ[tid] : 0;
  acc = 0;
  for (int64_t base = 0; base < len; base += PNP_CH) {
    const int k = (int)min<int64_t>(PNP_CH, len - base);
    stage(S, list, base, k, xyz, uv, false, tid, nt);
    __syncthreads();
    if (tid < 6)
      for (int i = 0; i < k; ++i) {
        const double t = (S.P[i][ei] - S.c[ei]) * (S.P[i][ej] - S.c[ej]);
        acc = (base + i == 0) ? t : acc + t;
      }
    __syncthreads();
  }
  if (tid < 6) S.acc[tid] = acc;
  __syncthreads();
  // 3. control points, the degenerate test, the Cramer matrix
  if (tid == 0) {
    double A[3][3], lam[3], E[3][3];
    A[0][0] = S.acc[0];
    A[0][1] = A[1][0] = S.acc[1];
    A[0][2] = A[2][0] = S.acc[2];
    A[1][1] = S.acc[3];
    A[1][2] = A[2][1] = S.acc[4];
    A[2][2] = S.acc[5];
    eig_sorted_small<3>(A, lam, E);
    S.degen = (lam[0] < 1e-3) || (lam[1] < 1e-3) || (lam[2] < 1e-3);
    const double c[3] = {S.c[0], S.c[1], S.c[2]};
#pragma unroll
    for (int x = 0; x < 3; ++x) S.ctl[0][x] = c[x];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double s = sqrt(lam[k] / (double)len);
#pragma unroll
      for (int x = 0; x < 3; ++x) S.ctl[k + 1][x] = c[x] + s * E[x][k];
    }
    // m[r][k] = ctl[k + 1][r] - c[r]
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) S.m[3 * r + k] = S.ctl[k + 1][r] - c[r];
    const double* m = S.m;
    const double D = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    S.zdet = D == 0;
    S.invD = 1.0 / D;
  }
  __syncthreads();
  if (S.degen) return;
  // 4. alphas (one entry per thread) and M^T M (one entry per thread, sequential over the list's rows 2i, 2i + 1)
  const double fx = cam.fx, fy = cam.fy, cx = cam.cx, cy = cam.cy;
  for (int e = tid; e < 78; e += nt) S.acc[e] = 0;
  for (int64_t base = 0; base < len; base += PNP_CH) {
    const int k = (int)min<int64_t>(PNP_CH, len - base);
    stage(S, list, base, k, xyz, uv, true, tid, nt);
    __syncthreads();
    for (int i = tid; i < k; i += nt) {
      const double m00 = S.m[0], m01 = S.m[1], m02 = S.m[2], m10 = S.m[3], m11 = S.m[4], m12 = S.m[5], m20 = S.m[6], m21 = S.m[7],
                   m22 = S.m[8], invD = S.invD;
      const double b0 = S.P[i][0] - S.c[0], b1 = S.P[i][1] - S.c[1], b2 = S.P[i][2] - S.c[2];
      double a1 = invD * (b0 * (m11 * m22 - m12 * m21) - m01 * (b1 * m22 - m12 * b2) + m02 * (b1 * m21 - m11 * b2));
      double a2 = invD * (m00 * (b1 * m22 - m12 * b2) - b0 * (m10 * m22 - m12 * m20) + m02 * (m10 * b2 - b1 * m20));
      double a3 = invD * (m00 * (m11 * b2 - b1 * m21) - m01 * (m10 * b2 - b1 * m20) + b0 * (m10 * m21 - m11 * m20));
      if (S.zdet) a1 = a2 = a3 = 0.0;
      S.al[i][0] = 1.0 - a1 - a2 - a3;
      S.al[i][1] = a1;
      S.al[i][2] = a2;
      S.al[i][3] = a3;
    }
    __syncthreads();
    for (int e = tid; e < 78; e += nt) {
      int a, b;
      entry_ab(e, a, b);
      const int ja = a / 3, ca = a % 3, jb = b / 3, cb = b % 3;
      double s = S.acc[e];
      for (int i = 0; i < k; ++i) {
        const double du = cx - S.Q[i][0], dv = cy - S.Q[i][1];
        const double r0a = ca == 0 ? S.al[i][ja] * fx : (ca == 1 ? 0.0 : S.al[i][ja] * du);
        const double r0b = cb == 0 ? S.al[i][jb] * fx : (cb == 1 ? 0.0 : S.al[i][jb] * du);
        const double r1a = ca == 0 ? 0.0 : (ca == 1 ? S.al[i][ja] * fy : S.al[i][ja] * dv);
        const double r1b = cb == 0 ? 0.0 : (cb == 1 ? S.al[i][jb] * fy : S.al[i][jb] * dv);
        s = (base + i == 0) ? r0a * r0b : s + r0a * r0b;
        s = s + r1a * r1b;
      }
      S.acc[e] = s;
    }
    __syncthreads();
  }
  for (int e = tid; e < 78; e += nt) {
    int a, b;
    entry_ab(e, a, b);
    S.M[a * 12 + b] = S.acc[e];
    S.M[b * 12 + a] = S.acc[e];
  }
  __syncthreads();
  // 5. eigenvectors of M^T M, then the tail on one lane
  jacobi12(S, tid, nt);
  if (tid == 0) epnp_tail(S);
  __syncthreads();
}

// PnPSolver::checkInliers in float for the pose `pose` (LDS): mask words [0, words) and S.cnt.  Every thread calls it.
__device__ void check_block(PnpLds& S, const float* pose, int n, int words, const float* xyz, const float* uv, const float* thr, PnpCam cam,
                            uint64_t* mask, int tid, int nt) {
  if (tid == 0) S.cnt = 0;
  __syncthreads();
  float R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = pose[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = pose[9 + i];
  const int lane = tid & 63;
  int cnt = 0;
  for (int base = 0; base < words * 64; base += nt) {
    const int i = base + tid;
    bool in = false;
    if (i < n) {
      const float X0 = xyz[3 * i], X1 = xyz[3 * i + 1], X2 = xyz[3 * i + 2];
      float pc[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float s = (R[3 * r] * X0 + R[3 * r + 1] * X1) + R[3 * r + 2] * X2;
        pc[r] = (float)((double)s + (double)t[r]);
      }
      const float u = pc[0] / pc[2] * cam.fx + cam.cx;
      const float v = pc[1] / pc[2] * cam.fy + cam.cy;
      const float du = uv[2 * i] - u, dv = uv[2 * i + 1] - v;
      const float err = du * du + dv * dv;
      in = err < thr[i];
    }
    const unsigned long long b = __ballot(in);
    const int w = i >> 6;
    if (lane == 0 && w < words) {
      mask[w] = b;
      cnt += __popcll(b);
    }
  }
  if (lane == 0) atomicAdd(&S.cnt, cnt);
  __syncthreads();
}

// append the set bits of mask[0 .. words) (ascending) to list at S.len; wave 0 does it, every thread calls it
__device__ void append_mask(PnpLds& S, const uint64_t* mask, int words, int* list, int tid) {
  if (tid < 64) {
    int64_t at = S.len;
    for (int base = 0; base < words; base += 64) {
      const int w = base + tid;
      unsigned long long m = w < words ? mask[w] : 0ull;
      const int pc = __popcll(m);
      int incl = pc;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (tid >= d) incl += o;
      }
      int64_t pos = at + (incl - pc);
      while (m) {
        const int bit = __ffsll((long long)m) - 1;
        list[pos++] = w * 64 + bit;
        m &= m - 1;
      }
      at += __shfl(incl, 63, 64);
    }
    if (tid == 0) S.len = at;
  }
  __syncthreads();
}

__global__ __launch_bounds__(PNP_HYP_WG) void k_pnp_hyp(const PnpHyp* __restrict__ hyps, const RansacProb* __restrict__ probs,
                                                        const float* __restrict__ xyz, const float* __restrict__ uv,
                                                        const float* __restrict__ thr, PnpCam cam, PnpOut* __restrict__ out,
                                                        uint64_t* __restrict__ masks) {
  __shared__ PnpLds S;
  const int tid = threadIdx.x, h = blockIdx.x;
  const PnpHyp& H = hyps[h];
  const RansacProb pr = probs[H.prob];
  const float* X = xyz + 3 * (int64_t)pr.off;
  const float* Q = uv + 2 * (int64_t)pr.off;
  if (H.given) {
    if (tid < 12) S.pose[tid] = H.pose[tid];
    if (tid == 0) S.degen = 0;
    __syncthreads();
  } else {
    if (tid < 4) S.idx[tid] = H.idx[tid];
    __syncthreads();
    epnp_block(S, S.idx, 4, X, Q, cam, tid, PNP_HYP_WG);
  }
  PnpOut& o = out[h];
  if (S.degen) {
    if (tid == 0) {
      o.degen = 1;
      o.count = 0;
      o.refined = 0;
      o.err = 0;
    }
    return;
  }
  check_block(S, S.pose, pr.n, pr.words, X, Q, thr + pr.off, cam, masks + H.mask_off, tid, PNP_HYP_WG);
  if (tid < 12) o.pose[tid] = S.pose[tid];
  if (tid == 0) {
    o.degen = 0;
    o.count = S.cnt;
    o.refined = 0;
    o.err = 0;
  }
}

__global__ __launch_bounds__(PNP_CALL_WG) void k_pnp_call(const PnpCall* __restrict__ calls, const PnpHyp* __restrict__ hyps,
                                                          const RansacProb* __restrict__ probs, const float* __restrict__ xyz,
                                                          const float* __restrict__ uv, const float* __restrict__ thr, PnpCam cam,
                                                          const int* __restrict__ entry, PnpOut* __restrict__ out,
                                                          const uint64_t* __restrict__ masks, uint64_t* __restrict__ ref_masks,
                                                          int* __restrict__ lists) {
  __shared__ PnpLds S;
  const int tid = threadIdx.x;
  const PnpCall C = calls[blockIdx.x];
  const RansacProb pr = probs[C.prob];
  const float* X = xyz + 3 * (int64_t)pr.off;
  const float* Q = uv + 2 * (int64_t)pr.off;
  const float* T = thr + pr.off;
  // a refine needs a count above mnMinInlier, and only a hypothesis' own pose or the entry pose can give the first one
  bool any = C.entry_hyp >= 0 && out[C.entry_hyp].count > pr.min_inlier;
  for (int i = 0; i < C.nh && !any; ++i) any = !out[C.h0 + i].degen && out[C.h0 + i].count > pr.min_inlier;
  if (!any) return;
  int* list = lists + C.list_off;
  for (int i = tid; i < C.entry_len; i += PNP_CALL_WG) list[i] = entry[C.entry_off + i];
  if (tid == 0) S.len = C.entry_len;
  __syncthreads();
  // the stale state: mask, count and pose of the last pose counted (P2)
  const uint64_t* st_mask = C.entry_hyp >= 0 ? masks + hyps[C.entry_hyp].mask_off : nullptr;
  int st_cnt = C.entry_hyp >= 0 ? out[C.entry_hyp].count : 0;
  const float* st_pose = C.entry_hyp >= 0 ? out[C.entry_hyp].pose : nullptr;
  for (int i = 0; i < C.nh; ++i) {
    const int h = C.h0 + i;
    if (!out[h].degen) {
      st_mask = masks + hyps[h].mask_off;
      st_cnt = out[h].count;
      st_pose = out[h].pose;
    }
    if (!st_mask) continue;
    if (S.len + st_cnt > C.list_cap) {
      if (tid == 0) out[h].err = 1;
      return;
    }
    append_mask(S, st_mask, pr.words, list, tid);
    if (st_cnt <= pr.min_inlier) continue;
    epnp_block(S, list, S.len, X, Q, cam, tid, PNP_CALL_WG);
    const int rdeg = S.degen;
    if (rdeg && tid < 12) S.pose[tid] = st_pose[tid];
    __syncthreads();
    uint64_t* rm = ref_masks + hyps[h].mask_off;
    check_block(S, S.pose, pr.n, pr.words, X, Q, T, cam, rm, tid, PNP_CALL_WG);
    const int rc = S.cnt;
    if (tid < 12) out[h].ref_pose[tid] = S.pose[tid];
    if (tid == 0) {
      out[h].refined = 1;
      out[h].ref_degen = rdeg;
      out[h].ref_count = rc;
    }
    if (rc > pr.min_inlier) return;
    __syncthreads();
    if (tid == 0) S.len = 0;
    __syncthreads();
    append_mask(S, rm, pr.words, list, tid);
    st_mask = rm;
    st_cnt = rc;
    st_pose = out[h].ref_pose;
  }
}

}  // namespace

void launch_pnp(hipStream_t st, const PnpHyp* hyps, int n_hyp, const PnpCall* calls, int n_calls, const RansacProb* probs, const float* xyz,
                const float* uv, const float* thr, const float cam[4], const int* entry, PnpOut* out, uint64_t* masks, uint64_t* ref_masks,
                int* lists) {
  const PnpCam c{cam[0], cam[1], cam[2], cam[3]};
  if (n_hyp > 0)
    hipLaunchKernelGGL(k_pnp_hyp, dim3((unsigned)n_hyp), dim3(PNP_HYP_WG), 0, st, hyps, probs, xyz, uv, thr, c, out, masks);
  if (n_calls > 0)
    hipLaunchKernelGGL(k_pnp_call, dim3((unsigned)n_calls), dim3(PNP_CALL_WG), 0, st, calls, hyps, probs, xyz, uv, thr, c, entry, out, masks,
                       ref_masks, lists);
}
