// k_pgsparse.hip -- the block-sparse Cholesky of the pose graph (orbfe_pose_graph_optimize_ex, solver 2): Hpp + lambda I of
// Optimizer::optimizeEssentialGraph factorised over the structure pg_symbolic.h computes, in vertex order, and both substitutions.  The
// sparse counterpart of k_lba_chol_solve (k_lba.hip); the 6x6 block arithmetic is pg_chol_dev.h's.  Rules F1 .. F6 of DESIGN 4.26.
//   k_pgs_assemble  one wave per block of Hpp: k_pg_assemble's incidence lists and edge order (G6), the block written to its place in
//                   L's storage (lower triangle only; the fill blocks stay zero from the memset before it) and the right-hand side
//   k_pgs_solve     ONE workgroup, right-looking by block column: (a) the diagonal block factorised by one lane in LDS, (b) every row
//                   of the blocks below it, and the right-hand side's own block, solved against it, (c) the rank-6 update of every
//                   block (r_a, r_b), a >= b, of the rows r of that column -- the symbolic phase guarantees each exists; its place in
//                   column r_b is found by a binary search of search_steps halvings -- and of the right-hand side; then L^T x = y from
//                   the last column up.  The dependent chain is nb block steps; a path-shaped elimination tree has no more to give.
// The column's solved blocks are parked in an LDS panel for step (c) up to PGS_PANEL_BLOCKS of them; a longer column (a loop connection's
// hub) reads them back from L's storage, where step (b) wrote them: same values, same order, a column of any length works.
// Guarantees: all fp64, no FMA contraction, no atomics; every entry has ONE owner per step and every sum a fixed order (F4 .. F6); the
// one launch is (1 workgroup, 1024 threads) whatever the size; every loop is bounded by a count of the symbolic phase; no wave waits on
// another workgroup; no private array is indexed at run time.
#include <hip/hip_runtime.h>

#include "orbfe_internal.h"
#include "pg_chol_dev.h"

namespace orbfe {

#define PGS_PANEL_BLOCKS 64  // 18 KB of LDS
#define PGS_BACK_PARTS 8     // F6: partial sums of the backward substitution's gather

// the incidence lists are k_pg_assemble's (k_posegraph.hip); pos[k] = the place of block k in L's storage
__global__ __launch_bounds__(64) void k_pgs_assemble(const int2* __restrict__ blk, const int32_t* __restrict__ blk_off,
                                                     const int32_t* __restrict__ ent, const int32_t* __restrict__ pos,
                                                     const double* __restrict__ Hee, const double* __restrict__ be,
                                                     const double* __restrict__ lambda_p, double* __restrict__ Lv, double* __restrict__ rhs) {
#pragma clang fp contract(off)
  const int k = blockIdx.x, lane = threadIdx.x;
  const int2 ij = blk[k];
  const int i = ij.x, j = ij.y;
  const int q0 = blk_off[k], q1 = blk_off[k + 1];
  if (lane < 36) {
    const int a = lane / 6, c = lane - 6 * a;
    double acc = 0;
    for (int q = q0; q < q1; ++q) {
      const int en = ent[q], code = en & 3;
      const double* H = Hee + (size_t)(en >> 2) * 108;
      acc += code == 3 ? H[72 + 6 * c + a] : H[36 * code + lane];
    }
    if (i == j && a == c) acc += lambda_p[0];
    Lv[(size_t)pos[k] * 36 + lane] = acc;  // row a of slot i, column c of slot j
  } else if (lane < 42 && i == j) {
    const int a = lane - 36;
    double acc = 0;
    for (int q = q0; q < q1; ++q) {
      const int en = ent[q];
      acc -= be[(size_t)(en >> 2) * 12 + 6 * (en & 3) + a];
    }
    rhs[6 * i + a] = acc;
  }
}

// step (c) of column k: P = the m solved blocks below the diagonal (LDS panel or L's storage), rows = their block rows, yk = the solved
// right-hand side of the column.  Item p < m (m + 1) / 2 is the pair (a, b), a >= b, in row-major order of the triangle; 36 threads a pair.
__device__ __forceinline__ void pgs_update(int t, int m, const double* __restrict__ P, const int32_t* __restrict__ rows,
                                           const double* __restrict__ yk, const int32_t* __restrict__ col_off,
                                           const int32_t* __restrict__ row, int search_steps, double* __restrict__ Lv, double* __restrict__ y) {
#pragma clang fp contract(off)
  const long long n_pair = (long long)m * (m + 1) / 2;
  const long long n_item = n_pair * 36 + 6 * (long long)m;
  for (long long idx = t; idx < n_item; idx += 1024) {
    if (idx < n_pair * 36) {
      const long long p = idx / 36;
      const int e = (int)(idx - p * 36), i = e / 6, j = e - 6 * i;
      // p -> (a, b): a = the largest integer with a (a + 1) / 2 <= p (the square root only proposes; the two corrections decide)
      long long a = (long long)((sqrt((double)(8 * p + 1)) - 1.0) * 0.5);
      if ((a + 1) * (a + 2) / 2 <= p) ++a;
      if (a * (a + 1) / 2 > p) --a;
      const int b = (int)(p - a * (a + 1) / 2);
      const int ra = rows[a], rb = rows[b];
      // F1: block (ra, rb) is in column rb; a == b is its diagonal block, the column's first
      int lo = col_off[rb], hi = col_off[rb + 1];
      if (a == b) hi = lo;
      else ++lo;
      for (int s = 0; s < search_steps; ++s) {
        if (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (row[mid] < ra) lo = mid + 1;
          else hi = mid;
        }
      }
      // F4: L(ra, rb)[i][j] -= row i of L(ra, k) . row j of L(rb, k); the upper triangle of a diagonal block is never read
      if (a != b || j <= i) Lv[(size_t)lo * 36 + e] -= pg_dot6(P + (size_t)a * 36 + 6 * i, P + (size_t)b * 36 + 6 * j);
    } else {
      const int r = (int)(idx - n_pair * 36), a = r / 6, i = r - 6 * a;
      y[(size_t)6 * rows[a] + i] -= pg_dot6(P + (size_t)a * 36 + 6 * i, yk);
    }
  }
}

// Lv: the blocks of Hpp + lambda I at their places in L's storage, the rest zero; L on return.  x = the solution, or zero with *ok = 0
// where a pivot is not positive and finite (*ok is only ever cleared).
__global__ __launch_bounds__(1024) void k_pgs_solve(int nb, const int32_t* __restrict__ col_off, const int32_t* __restrict__ row,
                                                    int search_steps, double* __restrict__ Lv, const double* __restrict__ rhs,
                                                    double* __restrict__ x, int* __restrict__ ok) {
#pragma clang fp contract(off)
  __shared__ double P[PGS_PANEL_BLOCKS * 36];
  __shared__ double Lk[36];
  __shared__ double yk[6];
  __shared__ double part[PGS_BACK_PARTS][6];
  __shared__ int s_ok;
  const int t = threadIdx.x;
  const int n = 6 * nb;
  for (int r = t; r < n; r += 1024) x[r] = rhs[r];  // x carries the right-hand side -> y -> x
  if (t == 0) s_ok = 1;
  __syncthreads();
  for (int k = 0; k < nb; ++k) {
    const int q0 = col_off[k], m = col_off[k + 1] - q0 - 1;
    if (t < 36) Lk[t] = Lv[(size_t)q0 * 36 + t];
    __syncthreads();
    if (t == 0 && !pg_chol6(Lk)) s_ok = 0;  // (a), F2
    __syncthreads();
    if (!s_ok) break;  // uniform
    // (b), F3: row r < 6 m of the blocks below the diagonal; r == 6 m is the right-hand side's block of this column
    const bool in_lds = m <= PGS_PANEL_BLOCKS;
    double* Lc = Lv + (size_t)(q0 + 1) * 36;
    for (int r = t; r <= 6 * m; r += 1024) {
      double v[6];
      if (r < 6 * m) {
        pg_row_solve6(Lk, Lc + (size_t)6 * r, v);
#pragma unroll
        for (int c = 0; c < 6; ++c) Lc[(size_t)6 * r + c] = v[c];
        if (in_lds) {
#pragma unroll
          for (int c = 0; c < 6; ++c) P[6 * r + c] = v[c];
        }
      } else {
        pg_row_solve6(Lk, x + (size_t)6 * k, v);
#pragma unroll
        for (int c = 0; c < 6; ++c) x[(size_t)6 * k + c] = v[c], yk[c] = v[c];
      }
    }
    if (t >= 64 && t < 100) Lv[(size_t)q0 * 36 + (t - 64)] = Lk[t - 64];  // the factorised diagonal block, for the way back
    __syncthreads();
    // (c)
    if (in_lds) pgs_update(t, m, P, row + q0 + 1, yk, col_off, row, search_steps, Lv, x);
    else pgs_update(t, m, Lc, row + q0 + 1, yk, col_off, row, search_steps, Lv, x);
    __syncthreads();
  }
  if (!s_ok) {
    if (t == 0) *ok = 0;
    for (int r = t; r < n; r += 1024) x[r] = 0.0;
    return;
  }
  // L^T x = y, column by column from the last.  F6: thread (w, c) adds the terms of the blocks a = w, w + PGS_BACK_PARTS, ... in
  // ascending a, rows 0 .. 5 of each; one lane adds the partial sums in ascending w, subtracts and solves the column's own block.
  for (int k = nb - 1; k >= 0; --k) {
    const int q0 = col_off[k], m = col_off[k + 1] - q0 - 1;
    if (t < 6 * PGS_BACK_PARTS) {
      const int w = t / 6, c = t - 6 * w;
      double acc = 0;
      for (int a = w; a < m; a += PGS_BACK_PARTS) {
        const double* B = Lv + (size_t)(q0 + 1 + a) * 36;
        const double* xa = x + (size_t)6 * row[q0 + 1 + a];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc += B[6 * i + c] * xa[i];
      }
      part[w][c] = acc;
    } else if (t >= 64 && t < 100) {
      Lk[t - 64] = Lv[(size_t)q0 * 36 + (t - 64)];
    }
    __syncthreads();
    if (t == 0) {
      double v[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double g = part[0][c];
#pragma unroll
        for (int w = 1; w < PGS_BACK_PARTS; ++w) g += part[w][c];
        v[c] = x[(size_t)6 * k + c] - g;
      }
      pg_back6(Lk, v);
#pragma unroll
      for (int c = 0; c < 6; ++c) x[(size_t)6 * k + c] = v[c];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
void launch_pgs_assemble(hipStream_t s, int n_blocks, const int2* blk, const int32_t* blk_off, const int32_t* ent, const int32_t* pos,
                         const double* Hee, const double* be, const double* lambda_p, double* Lv, double* rhs) {
  if (n_blocks > 0) hipLaunchKernelGGL(k_pgs_assemble, dim3(n_blocks), dim3(64), 0, s, blk, blk_off, ent, pos, Hee, be, lambda_p, Lv, rhs);
}
void launch_pgs_solve(hipStream_t s, int nb, const int32_t* col_off, const int32_t* row, int search_steps, double* Lv, const double* rhs,
                      double* x, int* ok) {
  if (nb > 0) hipLaunchKernelGGL(k_pgs_solve, dim3(1), dim3(1024), 0, s, nb, col_off, row, search_steps, Lv, rhs, x, ok);
}

}  // namespace orbfe
