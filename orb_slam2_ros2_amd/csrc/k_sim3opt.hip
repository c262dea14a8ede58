// k_sim3opt.hip -- Optimizer::OptimizeSim3 on the device: one workgroup runs the whole optimisation of one loop candidate.
//
// Replaces src/ORB_SLAM2/src/Optimizer.cc:464-619 from the point where the graph is built: one VertexSim3Expmap with the scale fixed, per
// match an EdgeSim3ProjectXYZ and an EdgeInverseSim3ProjectXYZ with Huber sqrt(9.210), optimize(5), pairs with a chi2 > 9.210 dropped,
// fewer than 20 left: nothing happens, else optimize(nBad ? 10 : 5) and the pairs with both chi2 <= 9.210 are the inliers.  Rules O1 .. O7
// of DESIGN 4.22; the edge model (numeric Jacobians included) is sim3_edge_dev.h's, the Levenberg-Marquardt machinery (27 staged sums,
// damped 6x6 solve, table of trial steps) is lm6_dev.h's, shared with k_pose_only_reg, whose state machine this one follows: ONE
// evaluation site, ONE build site, ONE solve site, the control replicated in every thread.
// A linearisation is 1 + 12 evaluations of every edge: the twelve estimates oplus(+-1e-9 e_d) are the same for all pairs, so twelve lanes
// compute them (and their inverses) into LDS once per build and every thread walks them in a loop that is NOT unrolled (code size: the
// instruction cache two compute units share holds 64 KB).  Column d of a pair's Jacobians lands in registers by compile-time index
// (a select per entry), never in a private array indexed at run time.
// Two instantiations: the pairs in registers (S3O_PPT per thread, n <= S3O_NT * S3O_PPT = 512: searchBySim3 yields 50 to a few hundred
// matches), or read from memory on every pass with the errors and flags in a scratch array (any n).  Every loop is bounded by n, 10 trials
// and 5 / 10 iterations; there is one workgroup.
#include <hip/hip_runtime.h>

#include "lm6_dev.h"
#include "orbfe_internal.h"
#include "sim3_edge_dev.h"
#include "wave_ops.h"

namespace orbfe {

#define S3O_NT 256
#define S3O_PPT 2

struct S3oShared {
  double H[36], b[6];
  double red[2][S3O_NT / 64];  // the evaluation's per-wave partial sums alternate between two rows: one barrier per sum
  Sim3Dev trial_T[LM6_TRIALS];  // every trial step an iteration can take, solved at once when its system is built
  double trial_x[LM6_TRIALS][6];
  int trial_ok[LM6_TRIALS];
  Sim3Dev pert[12], pert_inv[12];  // the estimates of the numeric Jacobian (sim3_perturbed) and their inverses
  double stage[27 * LM6_STAGE_LD(S3O_NT)];
};

struct S3oPair {
  Sim3Pair P;
  double E[4];  // the _error of both edges: what the last computeError left
  int idx;
  bool have, act;
};

struct S3oArgs {
  int n;
  const float *pc, *pm, *uvc, *uvm;
  const double *wc, *wm;
  const float* model_in;
  BaParamsDev prm;
  double delta;
  double* scratch_e;     // [n][4], memory path only
  uint8_t* scratch_act;  // [n], memory path only
  float* model_out;      // [12]
  uint8_t* inlier_out;   // [n]
  int32_t* ret;          // n_inliers, 1 if the optimisation ran to its end (0: fewer than 20 pairs were left, nothing else is written)
  double* est_out;       // [8]
};

__device__ __forceinline__ void s3o_load_pair(const S3oArgs& a, int i, Sim3Pair& P) {
#pragma unroll
  for (int k = 0; k < 3; ++k) P.pc[k] = (double)a.pc[3 * (size_t)i + k], P.pm[k] = (double)a.pm[3 * (size_t)i + k];
#pragma unroll
  for (int k = 0; k < 2; ++k) P.uvc[k] = (double)a.uvc[2 * (size_t)i + k], P.uvm[k] = (double)a.uvm[2 * (size_t)i + k];
  P.wc = a.wc[i], P.wm = a.wm[i];
}

template <bool MEM>
__global__ __launch_bounds__(S3O_NT) void k_sim3_optimize(S3oArgs a) {
#pragma clang fp contract(off)
  __shared__ S3oShared S;
  constexpr int NT = S3O_NT;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = a.n;
  const BaParamsDev prm = a.prm;
  const double delta = a.delta;

  S3oPair R[MEM ? 1 : S3O_PPT];
  if constexpr (!MEM) {
#pragma unroll
    for (int u = 0; u < S3O_PPT; ++u) {
      const int i = tid + u * NT;
      R[u].have = i < n;
      R[u].act = R[u].have;
      R[u].idx = i;
      s3o_load_pair(a, R[u].have ? i : 0, R[u].P);
#pragma unroll
      for (int k = 0; k < 4; ++k) R[u].E[k] = 0.0;
    }
  } else {
    for (int i = tid; i < n; i += NT) a.scratch_act[i] = 1;  // (pair i is always this thread's: no barrier between its passes)
  }
  // f(pair) on every pair of this thread: the register-resident ones, or each read from memory and its errors and flag written back
  auto for_each_pair = [&](auto&& f) {
    if constexpr (!MEM) {
#pragma unroll
      for (int u = 0; u < S3O_PPT; ++u)
        if (R[u].have) f(R[u]);
    } else {
      for (int i = tid; i < n; i += NT) {
        S3oPair r;
        s3o_load_pair(a, i, r.P);
#pragma unroll
        for (int k = 0; k < 4; ++k) r.E[k] = a.scratch_e[4 * (size_t)i + k];
        r.idx = i, r.have = true, r.act = a.scratch_act[i] != 0;
        f(r);
#pragma unroll
        for (int k = 0; k < 4; ++k) a.scratch_e[4 * (size_t)i + k] = r.E[k];
        a.scratch_act[i] = r.act ? 1 : 0;
      }
    }
  };
  int sum_slot = 0;
  auto block_sum_alt = [&](double v) {
    const double w = wave_sum_f64(v);
    double* row = S.red[sum_slot];
    if (lane == 0) row[wv] = w;
    __syncthreads();
    double sm = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) sm += row[k];
    sum_slot ^= 1;
    return sm;
  };

  Sim3Dev Tb;  // the current estimate (every thread: the same value)
  {
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = a.model_in[k];
    sim3_from_model(m, Tb);
  }
  int n_bad = 0, n_inl = 0;
  bool ran = true;
  for (int phase = 0; phase < 2; ++phase) {
    const int iterations = phase == 0 ? 5 : (n_bad ? 10 : 5);
    // ---- SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg, as a state machine (k_pose_only_reg's) ----
    {
      int it = 0;             // iterations completed
      bool do_solve = false;  // the pass starts with a trial step and its evaluation decides that trial
      double chi_cur = 0, current_chi = 0, lambda = 0, ni = 2;
      int qmax = 0;
      for (;;) {
        // the estimate the pass evaluates at: trial qmax of this iteration (solved when the system was built), or the current estimate
        Sim3Dev Te = Tb;
        bool trial_ok = true;
        if (do_solve) {
          Te = S.trial_T[qmax];
          trial_ok = S.trial_ok[qmax] != 0;  // ok2
        }
        // computeActiveErrors + activeRobustChi2 at Te -- the ONE evaluation site
        double chi;
        {
          Sim3Dev Tei;
          sim3_inverse(Te, Tei);
          double part = 0;
          for_each_pair([&](S3oPair& r) {
            if (!r.act) return;
            sim3_pair_errors(Te, Tei, r.P, prm, r.E);
            double c[2], r0, r1;
            sim3_pair_chi2(r.E, r.P, c);
            huber_robustify(c[0], delta, r0, r1);
            part += r0;
            huber_robustify(c[1], delta, r0, r1);
            part += r0;
          });
          chi = block_sum_alt(part);
        }
        if (!do_solve) {
          chi_cur = chi;  // the errors of the current estimate: an iteration starts
        } else {
          // decide the trial (every thread, the same numbers)
          double xs[6], bs[6];
#pragma unroll
          for (int j = 0; j < 6; ++j) xs[j] = S.trial_x[qmax][j], bs[j] = S.b[j];
          const double scale = lm6_scale(xs, lambda, bs);
          const LmDecision d = lm_decide(lambda, ni, current_chi, qmax, chi, scale, trial_ok, false);
          if (d.next == LM_RETRY) continue;  // another trial of the same iteration (new lambda, the same system)
          if (d.accepted) Tb = Te;  // (rejected: the estimate stays Tb, where g2o restores its backup)
          if (d.next == LM_TERMINATE) break;
          if (++it == iterations) break;
          if (!d.accepted) {  // (a trial neither accepted nor retried, e.g. a NaN gain ratio: the next iteration re-evaluates at the restored estimate)
            do_solve = false;
            continue;
          }
          chi_cur = chi;  // accepted: these ARE the errors and the chi2 of the new current estimate
        }
        // linearizeOplus (numeric) + constructQuadraticForm of every active edge at the current estimate -- the ONE build site
        {
          if (tid < 12) {
            Sim3Dev Sp, Spi;
            sim3_perturbed(Tb, tid, Sp);
            sim3_inverse(Sp, Spi);
            S.pert[tid] = Sp;
            S.pert_inv[tid] = Spi;
          }
          __syncthreads();
          double acc[27];
#pragma unroll
          for (int k = 0; k < 27; ++k) acc[k] = 0;
          for_each_pair([&](S3oPair& r) {
            if (!r.act) return;
            double J[4][6], ep[4] = {0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int d = 0; d < 6; ++d) J[q][d] = 0;
#pragma unroll 1
            for (int k = 0; k < 12; ++k) {
              const Sim3Dev Sp = S.pert[k], Spi = S.pert_inv[k];
              double e[4];
              sim3_pair_errors(Sp, Spi, r.P, prm, e);
              if ((k & 1) == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) ep[q] = e[q];
              } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const double col = sim3_num_diff(ep[q], e[q]);
#pragma unroll
                  for (int d = 0; d < 6; ++d) J[q][d] = (d == (k >> 1)) ? col : J[q][d];
                }
              }
            }
            double c[2];
            sim3_pair_chi2(r.E, r.P, c);
#pragma unroll
            for (int ed = 0; ed < 2; ++ed) {
              const double w = ed ? r.P.wm : r.P.wc;
              const double e0 = r.E[2 * ed], e1 = r.E[2 * ed + 1];
              double r0, r1;
              huber_robustify(c[ed], delta, r0, r1);
              int k = 0;
#pragma unroll
              for (int p = 0; p < 6; ++p) {
                acc[21 + p] -= r1 * (J[2 * ed][p] * (w * e0) + J[2 * ed + 1][p] * (w * e1));
#pragma unroll
                for (int c2 = p; c2 < 6; ++c2) acc[k++] += J[2 * ed][p] * (r1 * w) * J[2 * ed][c2] + J[2 * ed + 1][p] * (r1 * w) * J[2 * ed + 1][c2];
              }
            }
          });
          // (the previous system's b and trial table are rewritten only behind the barrier inside: every thread has read them by then)
          LM6_STAGE_REDUCE(NT, acc, S, tid)
        }
        // (lambda is initialised at every optimize(): tau * max |diag|; the seventh diagonal entry is 0, O1)
        lm_begin_iteration(lambda, ni, current_chi, qmax, chi_cur, it, lm6_maxdiag(S.H));
        // the trial steps of this iteration, all at once: lane q solves (H + lambda_q I) x = b and applies x to the estimate
        if (tid < LM6_TRIALS) {
          const double lam = lm6_trial_lambda(lambda, ni, tid);
          double xs[6] = {0, 0, 0, 0, 0, 0};
          const bool ok = solve6_lambda(S.H, lam, S.b, xs);
          Sim3Dev Tn;
          sim3_oplus(Tb, xs, Tn);
          S.trial_T[tid] = Tn;
          for (int j = 0; j < 6; ++j) S.trial_x[tid][j] = xs[j];
          S.trial_ok[tid] = ok ? 1 : 0;
        }
        __syncthreads();
        do_solve = true;
      }
    }
    // ---- the driver's two classifications (Optimizer.cc:568-607), on the errors the last evaluation left ----
    {
      int cnt = 0;
      for_each_pair([&](S3oPair& r) {
        double c[2];
        sim3_pair_chi2(r.E, r.P, c);
        if (phase == 0) {
          if (c[0] > SIM3_CHI2_TH || c[1] > SIM3_CHI2_TH) r.act = false, ++cnt;  // (a NaN chi2 is not bad here)
        } else {
          const bool inl = r.act && c[0] <= SIM3_CHI2_TH && c[1] <= SIM3_CHI2_TH;  // (and no inlier there)
          a.inlier_out[r.idx] = inl ? 1 : 0;
          cnt += inl ? 1 : 0;
        }
      });
      const int tot = (int)block_sum_alt((double)cnt);
      if (phase == 0) {
        n_bad = tot;
        if (n - n_bad < SIM3_MIN_PAIRS) {
          ran = false;
          break;
        }
      } else
        n_inl = tot;
    }
  }
  if (tid == 0) {
    a.ret[0] = ran ? n_inl : 0;
    a.ret[1] = ran ? 1 : 0;
    if (ran) {
      float m[12];
      sim3_to_model(Tb, m);
      for (int k = 0; k < 12; ++k) a.model_out[k] = m[k];
    }
    for (int k = 0; k < 4; ++k) a.est_out[k] = Tb.q[k];
    for (int k = 0; k < 3; ++k) a.est_out[4 + k] = Tb.t[k];
    a.est_out[7] = Tb.s;
  }
}

void launch_sim3_optimize(hipStream_t s, int n, const float* pc, const float* pm, const float* uvc, const float* uvm, const double* wc,
                          const double* wm, const float* model_in, BaParamsDev prm, double delta, double* scratch_e, uint8_t* scratch_act,
                          float* model_out, uint8_t* inlier_out, int32_t* ret, double* est_out) {
  S3oArgs a{n, pc, pm, uvc, uvm, wc, wm, model_in, prm, delta, scratch_e, scratch_act, model_out, inlier_out, ret, est_out};
  if (n <= S3O_NT * S3O_PPT)
    hipLaunchKernelGGL(k_sim3_optimize<false>, dim3(1), dim3(S3O_NT), 0, s, a);
  else
    hipLaunchKernelGGL(k_sim3_optimize<true>, dim3(1), dim3(S3O_NT), 0, s, a);
}
int sim3_optimize_register_capacity() { return S3O_NT * S3O_PPT; }

// orbfe_debug_sim3_edges: the edges as the optimiser sees them -- errors, chi2 and the numeric Jacobians of every pair at one estimate,
// one thread per pair, through the same header functions
__global__ __launch_bounds__(64) void k_debug_sim3_edges(S3oArgs a, const double* __restrict__ est, double* __restrict__ err,
                                                         double* __restrict__ chi2, double* __restrict__ jac) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  Sim3Dev T, Ti;
  for (int k = 0; k < 4; ++k) T.q[k] = est[k];
  for (int k = 0; k < 3; ++k) T.t[k] = est[4 + k];
  T.s = est[7];
  sim3_inverse(T, Ti);
  Sim3Pair P;
  s3o_load_pair(a, i, P);
  double e[4], c[2];
  sim3_pair_errors(T, Ti, P, a.prm, e);
  sim3_pair_chi2(e, P, c);
  for (int k = 0; k < 4; ++k) err[4 * (size_t)i + k] = e[k];
  chi2[2 * (size_t)i] = c[0], chi2[2 * (size_t)i + 1] = c[1];
  // (a column at a time, straight to memory: no Jacobian array indexed by the loop counter)
#pragma unroll 1
  for (int d = 0; d < 6; ++d) {
    Sim3Dev Sp, Spi;
    double ep[4], em[4];
    sim3_perturbed(T, 2 * d, Sp);
    sim3_inverse(Sp, Spi);
    sim3_pair_errors(Sp, Spi, P, a.prm, ep);
    sim3_perturbed(T, 2 * d + 1, Sp);
    sim3_inverse(Sp, Spi);
    sim3_pair_errors(Sp, Spi, P, a.prm, em);
    for (int q = 0; q < 4; ++q) jac[24 * (size_t)i + 6 * q + d] = sim3_num_diff(ep[q], em[q]);
  }
}

void launch_debug_sim3_edges(hipStream_t s, int n, const float* pc, const float* pm, const float* uvc, const float* uvm, const double* wc,
                             const double* wm, BaParamsDev prm, const double* est, double* err, double* chi2, double* jac) {
  S3oArgs a{n, pc, pm, uvc, uvm, wc, wm, nullptr, prm, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (n > 0) hipLaunchKernelGGL(k_debug_sim3_edges, dim3((n + 63) / 64), dim3(64), 0, s, a, est, err, chi2, jac);
}

}  // namespace orbfe
