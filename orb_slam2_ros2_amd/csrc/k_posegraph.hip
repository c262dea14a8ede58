// k_posegraph.hip -- the device side of Optimizer::optimizeEssentialGraph (src/ORB_SLAM2/src/Optimizer.cc:746-920): the pose graph over
// the essential graph's keyframes, 7-DoF vertices with the scale fixed, one EdgeSim3 per spanning-tree / loop / covisibility link.
//
// Replaces what g2o runs inside optimizer.optimize(20) there: EdgeSim3::computeError and the numeric linearizeOplus of both vertices
// (posegraph_edge_dev.h), constructQuadraticForm into the 6x6 blocks of Hpp (column 6 of every Jacobian is exactly 0 with the scale
// fixed, rule G1 of DESIGN 4.24, so the 7x7 block problem is a 6x6 one), BlockSolver::setLambda, the linear solve -- a pose graph has
// no landmarks and no Schur complement: Hpp + lambda I goes straight to launch_lba_chol (k_lba.hip), the LDS solver up to LBA_MAX_FREE
// block rows and the panel solver past it -- VertexSim3Expmap::oplusImpl, activeChi2 and computeScale.  The Levenberg-Marquardt control is
// on the host (orbfe_posegraph.hip), a few scalars per trial.
//   k_pg_build     one wave per edge: lanes 0 .. 24 evaluate the edge at the 25 estimates of a linearisation, the errors meet in LDS,
//                  lanes 0 .. 35 form the edge's three 6x6 blocks (J0^T J0, J1^T J1, J0^T J1), lanes 36 .. 47 its two 6-vectors J^T e
//   k_pg_maxdiag   computeLambdaInit: max |diag| over the free vertices, each diagonal entry summed in the order k_pg_assemble sums it
//   k_pg_assemble  one wave per non-empty block of S (the diagonal block of every free vertex, one block per joined pair): the edges of
//                  a host-built incidence list added in ascending edge index, lambda on the diagonal, S column-major with both triangles
//                  filled, and the right-hand side
//   k_pg_update    oplus of the step into the TRIAL estimates (the current ones stay: a rejected trial needs no restore)
//   k_pg_chi2      the error-only pass, one thread per edge;  k_pg_reduce  the sum of the chi2 and computeScale, one workgroup
// Guarantees: all fp64, no FMA contraction, no floating-point atomics (every block and every sum has ONE owner that adds in a fixed
// order); no result depends on the launch geometry (k_pg_build's waves per workgroup only choose which workgroup an edge lands in; the
// reductions are one workgroup of 1024 with a fixed tree); every loop is bounded by a vertex, edge or incidence count; no wave waits on
// another workgroup; no private array is indexed at run time (the 25 evaluations differ by lane, not by a loop counter, and meet in
// LDS).
#include <hip/hip_runtime.h>

#include "orbfe_internal.h"
#include "posegraph_edge_dev.h"

namespace orbfe {

#define PG_MAX_WAVES 4

__device__ __forceinline__ void pg_load_sim3(const double* __restrict__ p, Sim3Dev& S) {
#pragma unroll
  for (int k = 0; k < 4; ++k) S.q[k] = p[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) S.t[k] = p[4 + k];
  S.s = p[7];
}

// fixed-order workgroup sum / max of one double per thread (blockDim.x == 1024): k_lba.hip's tree
__device__ __forceinline__ double pg_block_reduce(double v, double* sh, bool take_max) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (t < o) sh[t] = take_max ? fmax(sh[t], sh[t + o]) : sh[t] + sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// Hee[e] = J0^T J0 | J1^T J1 | J0^T J1 (row-major 6x6 each), be[e] = J0^T e | J1^T e, err[e], chi2[e]; jac (nullable) [e][2][6][6] =
// J0[r][d] | J1[r][d].  A fixed vertex gets no evaluations: its Jacobian and its blocks are zero and nothing reads them.
__global__ __launch_bounds__(64 * PG_MAX_WAVES) void k_pg_build(int n_edges, int waves, const double* __restrict__ est,
                                                                const uint8_t* __restrict__ fixed, const int32_t* __restrict__ ev0,
                                                                const int32_t* __restrict__ ev1, const double* __restrict__ meas,
                                                                double* __restrict__ Hee, double* __restrict__ be, double* __restrict__ err,
                                                                double* __restrict__ chi2, double* __restrict__ jac) {
#pragma clang fp contract(off)
  __shared__ double E[PG_MAX_WAVES][PG_N_EVAL][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = (int)blockIdx.x * waves + wave;
  const bool have = e < n_edges;  // (uniform in the wave)
  if (have && lane < PG_N_EVAL) {
    const int v0 = ev0[e], v1 = ev1[e];
    const bool skip = (lane >= 1 && lane <= 12 && fixed[v0]) || (lane >= 13 && fixed[v1]);
    double ev[6] = {0, 0, 0, 0, 0, 0};
    if (!skip) {
      Sim3Dev C, S0, S1;
      pg_load_sim3(meas + (size_t)e * 8, C);
      pg_load_sim3(est + (size_t)v0 * 8, S0);
      pg_load_sim3(est + (size_t)v1 * 8, S1);
      pg_edge_eval(C, S0, S1, lane, ev);
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) E[wave][lane][r] = ev[r];
  }
  __syncthreads();
  if (!have) return;
  const double(*Ew)[6] = E[wave];
  if (lane < 36) {
    const int a = lane / 6, c = lane - 6 * a;
    double h00 = 0, h11 = 0, h01 = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double j0a = sim3_num_diff(Ew[1 + 2 * a][r], Ew[2 + 2 * a][r]), j0c = sim3_num_diff(Ew[1 + 2 * c][r], Ew[2 + 2 * c][r]);
      const double j1a = sim3_num_diff(Ew[13 + 2 * a][r], Ew[14 + 2 * a][r]), j1c = sim3_num_diff(Ew[13 + 2 * c][r], Ew[14 + 2 * c][r]);
      const double t00 = j0a * j0c, t11 = j1a * j1c, t01 = j0a * j1c;
      h00 = r ? h00 + t00 : t00;
      h11 = r ? h11 + t11 : t11;
      h01 = r ? h01 + t01 : t01;
    }
    double* H = Hee + (size_t)e * 108;
    H[lane] = h00, H[36 + lane] = h11, H[72 + lane] = h01;
    if (jac) {  // lane = (row a, column c) of both Jacobians
      jac[(size_t)e * 72 + lane] = sim3_num_diff(Ew[1 + 2 * c][a], Ew[2 + 2 * c][a]);
      jac[(size_t)e * 72 + 36 + lane] = sim3_num_diff(Ew[13 + 2 * c][a], Ew[14 + 2 * c][a]);
    }
  } else if (lane < 48) {
    const int w = (lane - 36) / 6, a = lane - 36 - 6 * w, k0 = w ? 13 : 1;
    double s = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double t = sim3_num_diff(Ew[k0 + 2 * a][r], Ew[k0 + 1 + 2 * a][r]) * Ew[0][r];
      s = r ? s + t : t;
    }
    be[(size_t)e * 12 + 6 * w + a] = s;
  } else if (lane < 54) {
    err[(size_t)e * 6 + (lane - 48)] = Ew[0][lane - 48];
  } else if (lane == 54) {
    double ev[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) ev[r] = Ew[0][r];
    chi2[e] = pg_edge_chi2(ev);
  }
}

// the incidence list: block k joins slots blk[k] = (i, j), i >= j, blocks 0 .. nf - 1 are the diagonal ones of slots 0 .. nf - 1; its
// entries ent[blk_off[k] .. blk_off[k + 1]) = 4 * edge + code in ascending edge index; code 0: the slot is the edge's vertex 0 (J0^T J0,
// J0^T e), 1: its vertex 1; 2: vertex 0 is slot i and vertex 1 slot j (the block is J0^T J1), 3: the other way round (its transpose)
__global__ __launch_bounds__(1024) void k_pg_maxdiag(int nf, const int32_t* __restrict__ blk_off, const int32_t* __restrict__ ent,
                                                     const double* __restrict__ Hee, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sh[1024];
  double m = 0;
  for (int i = threadIdx.x; i < nf * 6; i += 1024) {
    const int k = i / 6, a = i - 6 * k;
    double acc = 0;
    for (int q = blk_off[k]; q < blk_off[k + 1]; ++q) {
      const int en = ent[q];
      acc += Hee[(size_t)(en >> 2) * 108 + 36 * (en & 3) + 7 * a];
    }
    m = fmax(m, fabs(acc));
  }
  const double r = pg_block_reduce(m, sh, true);
  if (threadIdx.x == 0) out[0] = r;
}

__global__ __launch_bounds__(64) void k_pg_assemble(int nf, const int2* __restrict__ blk, const int32_t* __restrict__ blk_off,
                                                    const int32_t* __restrict__ ent, const double* __restrict__ Hee,
                                                    const double* __restrict__ be, const double* __restrict__ lambda_p,
                                                    double* __restrict__ S, double* __restrict__ rhs) {
#pragma clang fp contract(off)
  const int k = blockIdx.x, lane = threadIdx.x;
  const int2 ij = blk[k];
  const int i = ij.x, j = ij.y;
  const size_t n = (size_t)6 * nf;
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
    S[(size_t)(6 * i + a) + (size_t)(6 * j + c) * n] = acc;
    if (i != j) S[(size_t)(6 * j + c) + (size_t)(6 * i + a) * n] = acc;
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

// SparseOptimizer::update into the trial estimates: exp(dx) * estimate for a free vertex; a fixed vertex, and a vertex whose step is
// exactly zero (no edge: a zero block row), keep their bytes
__global__ __launch_bounds__(256) void k_pg_update(int n_vertices, const int32_t* __restrict__ slot, const double* __restrict__ x,
                                                   const double* __restrict__ est, double* __restrict__ trial) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_vertices) return;
  const int s = slot[v];
  double upd[6] = {0, 0, 0, 0, 0, 0};
  bool moves = false;
  if (s >= 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      upd[a] = x[6 * (size_t)s + a];
      moves = moves || upd[a] != 0.0;
    }
  }
  Sim3Dev T, R;
  pg_load_sim3(est + (size_t)v * 8, T);
  R = T;
  if (moves) sim3_oplus(T, upd, R);
  double* o = trial + (size_t)v * 8;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = R.q[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) o[4 + k] = R.t[k];
  o[7] = R.s;
}

// computeActiveErrors: the chi2 of every edge at the given estimates
__global__ __launch_bounds__(256) void k_pg_chi2(int n_edges, const double* __restrict__ est, const int32_t* __restrict__ ev0,
                                                 const int32_t* __restrict__ ev1, const double* __restrict__ meas, double* __restrict__ chi2) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  Sim3Dev C, S0, S1;
  pg_load_sim3(meas + (size_t)e * 8, C);
  pg_load_sim3(est + (size_t)ev0[e] * 8, S0);
  pg_load_sim3(est + (size_t)ev1[e] * 8, S1);
  double ev[6];
  pg_edge_error(C, S0, S1, ev);
  chi2[e] = pg_edge_chi2(ev);
}

// activeChi2 = sum of the chi2 -> out[0]; with n > 0 also computeScale = sum_i x_i (lambda x_i + b_i) over the n rows -> out[4]
__global__ __launch_bounds__(1024) void k_pg_reduce(int n_edges, const double* __restrict__ chi2, int n, const double* __restrict__ x,
                                                    const double* __restrict__ rhs, const double* __restrict__ lambda_p,
                                                    double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sh[1024];
  double acc = 0;
  for (int e = threadIdx.x; e < n_edges; e += 1024) acc += chi2[e];
  const double chi = pg_block_reduce(acc, sh, false);
  if (threadIdx.x == 0) out[0] = chi;
  if (n <= 0) return;  // (uniform)
  const double lambda = lambda_p[0];
  acc = 0;
  for (int i = threadIdx.x; i < n; i += 1024) acc += x[i] * (lambda * x[i] + rhs[i]);
  const double sc = pg_block_reduce(acc, sh, false);
  if (threadIdx.x == 0) out[4] = sc;
}

// ---------------------------------------------------------------------------------------------
int pg_max_waves() { return PG_MAX_WAVES; }
void launch_pg_build(hipStream_t s, int n_edges, int waves, const double* est, const uint8_t* fixed, const int32_t* ev0, const int32_t* ev1,
                     const double* meas, double* Hee, double* be, double* err, double* chi2, double* jac) {
  if (n_edges > 0)
    hipLaunchKernelGGL(k_pg_build, dim3((n_edges + waves - 1) / waves), dim3(64 * waves), 0, s, n_edges, waves, est, fixed, ev0, ev1, meas, Hee, be,
                       err, chi2, jac);
}
void launch_pg_maxdiag(hipStream_t s, int nf, const int32_t* blk_off, const int32_t* ent, const double* Hee, double* out) {
  hipLaunchKernelGGL(k_pg_maxdiag, dim3(1), dim3(1024), 0, s, nf, blk_off, ent, Hee, out);
}
void launch_pg_assemble(hipStream_t s, int nf, int n_blocks, const int2* blk, const int32_t* blk_off, const int32_t* ent, const double* Hee,
                        const double* be, const double* lambda_p, double* S, double* rhs) {
  if (n_blocks > 0) hipLaunchKernelGGL(k_pg_assemble, dim3(n_blocks), dim3(64), 0, s, nf, blk, blk_off, ent, Hee, be, lambda_p, S, rhs);
}
void launch_pg_update(hipStream_t s, int n_vertices, const int32_t* slot, const double* x, const double* est, double* trial) {
  if (n_vertices > 0) hipLaunchKernelGGL(k_pg_update, dim3((n_vertices + 255) / 256), dim3(256), 0, s, n_vertices, slot, x, est, trial);
}
void launch_pg_chi2(hipStream_t s, int n_edges, const double* est, const int32_t* ev0, const int32_t* ev1, const double* meas, double* chi2) {
  if (n_edges > 0) hipLaunchKernelGGL(k_pg_chi2, dim3((n_edges + 255) / 256), dim3(256), 0, s, n_edges, est, ev0, ev1, meas, chi2);
}
void launch_pg_reduce(hipStream_t s, int n_edges, const double* chi2, int n, const double* x, const double* rhs, const double* lambda_p,
                      double* out) {
  hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(1024), 0, s, n_edges, chi2, n, x, rhs, lambda_p, out);
}

}  // namespace orbfe
