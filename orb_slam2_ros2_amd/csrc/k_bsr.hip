// k_bsr.hip -- the reduced camera system of a bundle adjustment as 6x6 block-CSR, and a block-Jacobi preconditioned conjugate-gradient
// solver for it.  What the global BA (orbfe_gba.hip) runs where the local BA runs a dense Cholesky: after a loop closure every keyframe
// of the map is a vertex, consecutive keyframes share points and a few loop blocks sit far from the diagonal, so S has O(nf) blocks.
//
// Layout: row_off[nb + 1], col[nnzb] ascending per row, blocks[nnzb][36] row-major (block (i, j) entry (a, c) = S[6i + a][6j + c]),
// both triangles stored, the diagonal always present, twin[q] = index of the transposed block.
//
// All fp64, no FMA contraction, no floating-point atomics: every sum has one fixed order, so a repeated call is bit-identical.  Plain
// launches only -- nothing waits on another workgroup inside a kernel.  A dot product is two stages: the producing kernel leaves one
// partial per block row, every workgroup of the consuming kernel adds them up in the same order and so arrives at the same bits.  alpha,
// beta and the stopping test live on the device (PcgState); the kernels of iteration k read state[k & 1] and rz[k & 1], the last one writes
// the other entry, so no word is read and written by the same launch.  Once state != 0 every later launch returns at once; the last
// kernel of such an iteration only copies the verdict into the entry the next iteration reads.
#include <hip/hip_runtime.h>

#include "orbfe_internal.h"

namespace orbfe {

#define BSR_VEC_T 192  // threads of the vector kernels: 32 block rows of 6
#define BSR_VEC_ROWS 32

// Inverse of a symmetric positive-definite 6x6 matrix by Cholesky, in registers.  A = the lower triangle, A[r * (r + 1) / 2 + c], c <= r.
// Lane k < 6 leaves column k of the inverse in x[0..5].  Returns false on a pivot that is not positive and finite.
__device__ __forceinline__ bool chol6_inverse_column(const double (&A)[21], int k, double (&x)[6]) {
#pragma clang fp contract(off)
  double L[21];
  bool good = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j * (j + 1) / 2 + j];
#pragma unroll
    for (int m = 0; m < j; ++m) d -= L[j * (j + 1) / 2 + m] * L[j * (j + 1) / 2 + m];
    if (!(d > 0) || !isfinite(d)) good = false;
    d = sqrt(d);
    L[j * (j + 1) / 2 + j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i * (i + 1) / 2 + j];
#pragma unroll
      for (int m = 0; m < j; ++m) v -= L[i * (i + 1) / 2 + m] * L[j * (j + 1) / 2 + m];
      L[i * (i + 1) / 2 + j] = v / d;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {  // L y = e_k
    double v = (i == k) ? 1.0 : 0.0;
#pragma unroll
    for (int m = 0; m < i; ++m) v -= L[i * (i + 1) / 2 + m] * y[m];
    y[i] = v / L[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {  // L^T x = y
    double v = y[i];
#pragma unroll
    for (int m = i + 1; m < 6; ++m) v -= L[m * (m + 1) / 2 + i] * x[m];
    x[i] = v / L[i * (i + 1) / 2 + i];
  }
  return good;
}

// The wave's lanes 0..35 hold a diagonal block (lane = 6 a + c, symmetric): write its inverse (symmetric to the bit: entry (r, k), r >= k,
// comes from column k and is stored at both places) or, on a bad pivot, zeros and *ok = 0.  Every lane of the wave must call this.
__device__ __forceinline__ void wave_diag_inverse(double v, int lane, double* __restrict__ Minv_i, int* __restrict__ ok) {
  double A[21];
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) A[r * (r + 1) / 2 + c] = __shfl(v, 6 * r + c);
  double x[6];
  const bool good = chol6_inverse_column(A, lane, x);  // (lanes >= 6 solve for a zero right-hand side; the verdict is the same in every lane)
  if (!good && lane == 0) *ok = 0;
  if (lane < 6) {
#pragma unroll
    for (int r = 0; r < 6; ++r)
      if (r >= lane) {
        const double w = good ? x[r] : 0.0;
        Minv_i[6 * r + lane] = w;
        Minv_i[6 * lane + r] = w;
      }
  }
}

// Reduced system, one wave per stored block (i, j) with i >= j: k_lba_schur's arithmetic on the block's pair list,
//   S_ij = [i == j] (Hpp_i + lambda I) - sum_pairs W(e1) Hpl(e2)^T          rhs_i = bp_i - sum_{e of pose i} W(e) bl(point(e))
// The wave also writes the transpose into the twin block, and a diagonal block takes its upper triangle from its lower one, so S is
// symmetric to the bit; a diagonal block's inverse is the preconditioner.
__global__ __launch_bounds__(64) void k_bsr_schur(int n_low, const int32_t* __restrict__ low, const int32_t* __restrict__ low_row,
                                                  const int32_t* __restrict__ col, const int32_t* __restrict__ twin,
                                                  const int32_t* __restrict__ pair_off, const int2* __restrict__ pairs,
                                                  const int32_t* __restrict__ free_pose, const int32_t* __restrict__ ps_off,
                                                  const int32_t* __restrict__ ps_edges, const int32_t* __restrict__ edge_point,
                                                  const double* __restrict__ Hpp, const double* __restrict__ bp, const double* __restrict__ bl,
                                                  const double* __restrict__ Hpl, const double* __restrict__ W,
                                                  const double* __restrict__ lambda_p, double* __restrict__ blocks, double* __restrict__ rhs,
                                                  double* __restrict__ Minv, int* __restrict__ ok) {
#pragma clang fp contract(off)
  const int l = blockIdx.x, lane = threadIdx.x;
  if (l >= n_low) return;
  const int q = low[l], i = low_row[l], j = col[q];
  const int ki = free_pose[i];
  double acc = 0;
  if (lane < 36) {
    const int a = lane / 6, c = lane - 6 * a;
    if (i == j) {
      acc = Hpp[(size_t)ki * 36 + lane];
      if (a == c) acc += lambda_p[0];
    }
    for (int t = pair_off[l]; t < pair_off[l + 1]; ++t) {
      const int2 pr = pairs[t];
      const double* w = W + (size_t)pr.x * 18 + 3 * a;
      const double* h = Hpl + (size_t)pr.y * 18 + 3 * c;
      acc -= w[0] * h[0] + w[1] * h[1] + w[2] * h[2];
    }
  } else if (lane < 42 && i == j) {
    const int a = lane - 36;
    double r = bp[(size_t)ki * 6 + a];
    for (int t = ps_off[ki]; t < ps_off[ki + 1]; ++t) {
      const int e = ps_edges[t];
      const double* w = W + (size_t)e * 18 + 3 * a;
      const double* b = bl + (size_t)edge_point[e] * 3;
      r -= w[0] * b[0] + w[1] * b[1] + w[2] * b[2];
    }
    rhs[6 * i + a] = r;
  }
  if (i == j) {
    const int a = (lane % 36) / 6, c = lane % 6;
    acc = __shfl(acc, a >= c ? 6 * a + c : 6 * c + a);  // the upper triangle is the lower one
    if (lane < 36) blocks[(size_t)q * 36 + lane] = acc;
    wave_diag_inverse(acc, lane, Minv + (size_t)i * 36, ok);
  } else if (lane < 36) {
    const int a = lane / 6, c = lane - 6 * a;
    blocks[(size_t)q * 36 + lane] = acc;
    blocks[(size_t)twin[q] * 36 + 6 * c + a] = acc;
  }
}

// the preconditioner of a system given as blocks (orbfe_debug_bsr_pcg): one wave per block row, the diagonal block found by its column
__global__ __launch_bounds__(64) void k_bsr_diag_inv(int nb, const int32_t* __restrict__ row_off, const int32_t* __restrict__ col,
                                                     const double* __restrict__ blocks, double* __restrict__ Minv, int* __restrict__ ok) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= nb) return;
  int qd = -1;
  for (int q = row_off[i]; q < row_off[i + 1]; ++q)
    if (col[q] == i) qd = q;
  double v = 0;  // (no diagonal block: a zero pivot, ok = 0)
  if (qd >= 0 && lane < 36) {
    const int a = lane / 6, c = lane - 6 * a;
    v = blocks[(size_t)qd * 36 + (a >= c ? 6 * a + c : 6 * c + a)];
  }
  wave_diag_inverse(v, lane, Minv + (size_t)i * 36, ok);
}

// Sum of m partials in one fixed order by a workgroup of BSR_VEC_T threads (sh: 256 doubles).  Every workgroup that calls it with the same
// partials gets the same bits.
__device__ __forceinline__ double bsr_sum_partials(const double* __restrict__ part, int m, double* sh) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  double acc = 0;
  for (int k = t; k < m; k += BSR_VEC_T) acc += part[k];
  sh[t] = acc;
  if (t < 256 - BSR_VEC_T) sh[BSR_VEC_T + t] = 0.0;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] = sh[t] + sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// x = 0, r = b, z = M^-1 r, p = z, and the partials of r.z: one thread per unknown
__global__ __launch_bounds__(BSR_VEC_T) void k_pcg_init(int nb, const double* __restrict__ b, const double* __restrict__ Minv,
                                                        double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                        double* __restrict__ p, double* __restrict__ part_rz) {
#pragma clang fp contract(off)
  __shared__ double sh[BSR_VEC_T];
  const int t = threadIdx.x, i = blockIdx.x * BSR_VEC_ROWS + t / 6, a = t % 6;
  double prod = 0;
  if (i < nb) {
    const double* bi = b + (size_t)6 * i;
    const double* Mi = Minv + (size_t)36 * i + 6 * a;
    double zv = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) zv += Mi[c] * bi[c];
    const size_t g = (size_t)6 * i + a;
    x[g] = 0.0, r[g] = bi[a], z[g] = zv, p[g] = zv;
    prod = bi[a] * zv;
  }
  sh[t] = prod;
  __syncthreads();
  if (i < nb && a == 0) part_rz[i] = ((((sh[t] + sh[t + 1]) + sh[t + 2]) + sh[t + 3]) + sh[t + 4]) + sh[t + 5];
}

// the first verdict (one workgroup): b.M^-1 b, and whether there is anything to iterate on
__global__ __launch_bounds__(BSR_VEC_T) void k_pcg_start(int nb, const double* __restrict__ part_rz, double tol,
                                                         const int* __restrict__ ok, PcgState* __restrict__ st) {
  __shared__ double sh[256];
  const double rz0 = bsr_sum_partials(part_rz, nb, sh);
  if (threadIdx.x == 0) {
    st->rz[0] = rz0, st->rz[1] = 0.0, st->rz0 = rz0, st->tol2 = tol * tol;
    st->iters = 0, st->pq_bad = 0;
    int s = PCG_RUNNING;
    if (*ok == 0 || !isfinite(rz0) || rz0 < 0) s = PCG_BREAKDOWN;  // (a diagonal block was not positive definite: x stays 0)
    else if (rz0 == 0) s = PCG_CONVERGED;                          // x = 0 solves it
    st->state[0] = s, st->state[1] = s, st->done = s;
  }
}

// q = S p and the partials of p.q.  One wave per block row; lane = 6 * slot + a (10 slots a pass) reads row a of its block and the six
// entries of p behind the block's column; a row longer than ten blocks takes further passes.  The slots are added in ascending order.
__global__ __launch_bounds__(256) void k_pcg_spmv(int nb, int k, const int32_t* __restrict__ row_off, const int32_t* __restrict__ col,
                                                  const double* __restrict__ blocks, const double* __restrict__ p, double* __restrict__ q,
                                                  double* __restrict__ part_pq, const PcgState* __restrict__ st) {
#pragma clang fp contract(off)
  if (st->state[k & 1] != PCG_RUNNING) return;  // uniform
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nb) return;  // (whole waves; no barrier below)
  const int slot = lane / 6, a = lane - 6 * slot;
  const int q0 = row_off[i], q1 = row_off[i + 1];
  double acc = 0;
  if (slot < 10)
    for (int s = q0 + slot; s < q1; s += 10) {
      const double* B = blocks + (size_t)s * 36 + 6 * a;
      const double* pv = p + (size_t)6 * col[s];
      acc += ((((B[0] * pv[0] + B[1] * pv[1]) + B[2] * pv[2]) + B[3] * pv[3]) + B[4] * pv[4]) + B[5] * pv[5];
    }
  double sum = 0;
#pragma unroll
  for (int s = 0; s < 10; ++s) sum += __shfl(acc, 6 * s + (lane % 6));
  const double pa = p[(size_t)6 * i + (lane % 6)];
  const double prod = sum * pa;
  double dot = 0;
#pragma unroll
  for (int c = 0; c < 6; ++c) dot += __shfl(prod, c);
  if (lane < 6) q[(size_t)6 * i + lane] = sum;
  if (lane == 0) part_pq[i] = dot;
}

// alpha = r.z / p.q;  x += alpha p, r -= alpha q, z = M^-1 r, and the partials of the new r.z.  p.q <= 0 or not finite: breakdown, nothing
// is updated and the next kernel stops the iteration.
__global__ __launch_bounds__(BSR_VEC_T) void k_pcg_update(int nb, int k, const double* __restrict__ part_pq, const double* __restrict__ Minv,
                                                          const double* __restrict__ p, const double* __restrict__ q, double* __restrict__ x,
                                                          double* __restrict__ r, double* __restrict__ z, double* __restrict__ part_rz,
                                                          PcgState* __restrict__ st) {
#pragma clang fp contract(off)
  __shared__ double sh[256];
  if (st->state[k & 1] != PCG_RUNNING) return;  // uniform
  const double pq = bsr_sum_partials(part_pq, nb, sh);
  const bool broken = !(pq > 0) || !isfinite(pq);
  if (blockIdx.x == 0 && threadIdx.x == 0) st->pq_bad = broken ? 1 : 0;  // (read by k_pcg_direction only)
  if (broken) return;
  const double alpha = st->rz[k & 1] / pq;
  const int t = threadIdx.x, i = blockIdx.x * BSR_VEC_ROWS + t / 6, a = t % 6;
  const size_t g0 = (size_t)6 * i;
  double ra = 0, zv = 0;
  if (i < nb) {
    const double* Mi = Minv + (size_t)36 * i + 6 * a;
    double rn[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) rn[c] = r[g0 + c] - alpha * q[g0 + c];  // (the six threads of a row compute the same six values)
#pragma unroll
    for (int c = 0; c < 6; ++c) zv += Mi[c] * rn[c];
    ra = rn[0];
#pragma unroll
    for (int c = 1; c < 6; ++c) ra = (c == a) ? rn[c] : ra;
  }
  __syncthreads();  // every thread of a row has read r before one of them writes it
  if (i < nb) {
    x[g0 + a] = x[g0 + a] + alpha * p[g0 + a];
    r[g0 + a] = ra;
    z[g0 + a] = zv;
  }
  const double prod = ra * zv;
  sh[t] = prod;
  __syncthreads();
  if (i < nb && a == 0) part_rz[i] = ((((sh[t] + sh[t + 1]) + sh[t + 2]) + sh[t + 3]) + sh[t + 4]) + sh[t + 5];
}

// The stopping test r.z <= tol^2 b.M^-1 b, then beta = r.z_new / r.z and p = z + beta p.  Writes the state and r.z of iteration k + 1.
__global__ __launch_bounds__(BSR_VEC_T) void k_pcg_direction(int nb, int k, const double* __restrict__ part_rz, const double* __restrict__ z,
                                                             double* __restrict__ p, PcgState* __restrict__ st) {
#pragma clang fp contract(off)
  __shared__ double sh[256];
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  const int s0 = st->state[k & 1];
  if (s0 != PCG_RUNNING) {  // uniform.  Over: hand the verdict on to the entry the next iteration reads (this one reads the other)
    if (first) st->state[(k + 1) & 1] = s0;
    return;
  }
  if (st->pq_bad) {
    if (first) st->state[(k + 1) & 1] = PCG_BREAKDOWN, st->done = PCG_BREAKDOWN;
    return;
  }
  const double rz_new = bsr_sum_partials(part_rz, nb, sh);
  const double rz_old = st->rz[k & 1];
  int s = PCG_RUNNING;
  if (!isfinite(rz_new)) s = PCG_BREAKDOWN;
  else if (rz_new <= st->tol2 * st->rz0) s = PCG_CONVERGED;
  if (first) {
    st->iters = st->iters + 1;  // (written and read by this thread alone)
    st->rz[(k + 1) & 1] = rz_new;
    st->state[(k + 1) & 1] = s;
    st->done = s;  // (the host's copy of the verdict: no kernel reads it)
  }
  if (s != PCG_RUNNING) return;
  const double beta = rz_new / rz_old;
  const int t = threadIdx.x, i = blockIdx.x * BSR_VEC_ROWS + t / 6, a = t % 6;
  if (i < nb) {
    const size_t g = (size_t)6 * i + a;
    p[g] = z[g] + beta * p[g];
  }
}

// ---------------------------------------------------------------------------------------------
void launch_bsr_schur(hipStream_t s, int n_low, const int32_t* low, const int32_t* low_row, const int32_t* col, const int32_t* twin,
                      const int32_t* pair_off, const int2* pairs, const int32_t* free_pose, const int32_t* ps_off, const int32_t* ps_edges,
                      const int32_t* edge_point, const double* Hpp, const double* bp, const double* bl, const double* Hpl, const double* W,
                      const double* lambda_p, double* blocks, double* rhs, double* Minv, int* ok) {
  if (n_low > 0)
    hipLaunchKernelGGL(k_bsr_schur, dim3(n_low), dim3(64), 0, s, n_low, low, low_row, col, twin, pair_off, pairs, free_pose, ps_off, ps_edges,
                       edge_point, Hpp, bp, bl, Hpl, W, lambda_p, blocks, rhs, Minv, ok);
}
void launch_bsr_diag_inv(hipStream_t s, const BsrPcgLaunch& L) {
  if (L.nb > 0) hipLaunchKernelGGL(k_bsr_diag_inv, dim3(L.nb), dim3(64), 0, s, L.nb, L.row_off, L.col, L.blocks, L.Minv, L.ok);
}
void launch_pcg_begin(hipStream_t s, const BsrPcgLaunch& L, double tol) {
  const int g = (L.nb + BSR_VEC_ROWS - 1) / BSR_VEC_ROWS;
  hipLaunchKernelGGL(k_pcg_init, dim3(g), dim3(BSR_VEC_T), 0, s, L.nb, L.rhs, L.Minv, L.x, L.r, L.z, L.p, L.part_rz);
  hipLaunchKernelGGL(k_pcg_start, dim3(1), dim3(BSR_VEC_T), 0, s, L.nb, L.part_rz, tol, L.ok, L.state);
}
// iterations [k0, k0 + n) of the solve launch_pcg_begin started: three launches each
void launch_pcg_iterations(hipStream_t s, const BsrPcgLaunch& L, int k0, int n) {
  const int g = (L.nb + BSR_VEC_ROWS - 1) / BSR_VEC_ROWS;
  for (int k = k0; k < k0 + n; ++k) {
    hipLaunchKernelGGL(k_pcg_spmv, dim3((L.nb + 3) / 4), dim3(256), 0, s, L.nb, k, L.row_off, L.col, L.blocks, L.p, L.q, L.part_pq, L.state);
    hipLaunchKernelGGL(k_pcg_update, dim3(g), dim3(BSR_VEC_T), 0, s, L.nb, k, L.part_pq, L.Minv, L.p, L.q, L.x, L.r, L.z, L.part_rz, L.state);
    hipLaunchKernelGGL(k_pcg_direction, dim3(g), dim3(BSR_VEC_T), 0, s, L.nb, k, L.part_rz, L.z, L.p, L.state);
  }
}

}  // namespace orbfe
