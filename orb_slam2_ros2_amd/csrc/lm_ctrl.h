// lm_ctrl.h -- the ONE Levenberg-Marquardt controller of the optimisers: what g2o's OptimizationAlgorithmLevenberg::solve decides between
// two linear solves -- tau * max |diag| as the first damping, the gain ratio, lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)) on an
// accepted trial, lambda *= ni, ni *= 2 on a rejected one, at most ten trials per iteration, and SparseOptimizer::optimize's Terminate
// test.  The damping state is four scalars (lambda, ni, current_chi, qmax) passed by reference, so that each caller keeps them where they
// already live: registers (k_pose_only_reg, k_sim3_optimize), LDS (k_pose_only), the LmState record (k_lm_ctrl), host locals (lm_host.h).
// Every expression is spelled in g2o's evaluation order: fp64, contraction off.
// Host + device like ba_edge_dev.h: tests/cpp/test_lm_ctrl.cpp compiles this header with the host compiler alone.
#pragma once
#include "se3_dev.h"
#ifndef __HIPCC__
#include <cmath>
#endif

namespace orbfe {

#define LM_TRIALS 10  // g2o's Levenberg-Marquardt gives an iteration at most 10 trial steps (qmax)

enum LmNext {
  LM_RETRY = 0,           // another trial of the same iteration: the same system, the new lambda
  LM_NEXT_ITERATION = 1,  // the iteration is over (without `accepted`: a trial neither accepted nor retried, e.g. a NaN gain ratio)
  LM_TERMINATE = 2,       // OptimizationAlgorithm::Terminate
};
struct LmDecision {
  bool accepted;  // the trial's estimate becomes the current one (else g2o pops its backup)
  int next;       // LmNext
};

// (2 rho - 1)^3 the way each side has always taken it: the device library's pow with an int exponent, the C library's pow on the host --
// one different last bit of lambda changes a trajectory
ORBFE_HD_INLINE double lm_cube(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return pow(v, 3);
#else
  return std::pow(v, 3);
#endif
}

// (isfinite is a device-only overload under the HIP compiler and std::isfinite a host-only one)
ORBFE_HD_INLINE bool lm_isfinite(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return isfinite(v);
#else
  return std::isfinite(v);
#endif
}

// An iteration starts on the system linearised at the current estimate (chi: its robust chi2; maxdiag: max |H_jj|, read at it == 0 only).
// computeLambdaInit (tau = 1e-5) runs once per optimize(): lambda and ni carry over from one iteration to the next.
ORBFE_HD_INLINE void lm_begin_iteration(double& lambda, double& ni, double& current_chi, int& qmax, double chi, int it, double maxdiag) {
  ORBFE_FP_STRICT
  current_chi = chi;
  if (it == 0) {
    lambda = 1e-5 * maxdiag;
    ni = 2;
  }
  qmax = 0;
}

// A trial ran: trial_chi is the robust chi2 at the trial estimate, scale = sum x_j (lambda x_j + b_j) (computeScale, without the 1e-3),
// ok whether the linear solve succeeded, stopped the caller's stop flag.
ORBFE_HD_INLINE LmDecision lm_decide(double& lambda, double& ni, double& current_chi, int& qmax, double trial_chi, double scale, bool ok,
                                     bool stopped) {
  ORBFE_FP_STRICT
  const double temp_chi = ok ? trial_chi : 1.7976931348623157e308;
  double rho = (current_chi - temp_chi) / (scale + 1e-3);
  if (!ok) rho = -1.0;  // the linear solver failed: the trial is rejected whatever its step looked like
  LmDecision d = {rho > 0 && lm_isfinite(temp_chi), LM_NEXT_ITERATION};
  bool alive = true;  // lambda is still finite
  if (d.accepted) {
    double alpha = 1. - lm_cube(2 * rho - 1);
    alpha = fmin(alpha, 2. / 3.);
    lambda *= fmax(1. / 3., alpha);
    ni = 2;
    current_chi = temp_chi;
  } else {
    lambda *= ni;
    ni *= 2;
    alive = lm_isfinite(lambda);
  }
  // (g2o breaks out of the trial loop before ++qmax when lambda dies.  A flag, not an early return: the register kernels run this in
  //  every wave behind a barrier, and with the extra exit k_sim3_optimize and k_pose_only_reg ran 1 to 1.5 % longer -- profiles/NOTES_r8.md)
  qmax += alive ? 1 : 0;
  if (alive && rho < 0 && qmax < LM_TRIALS && !stopped)
    d.next = LM_RETRY;
  else if (!alive || qmax == LM_TRIALS || rho == 0 || !lm_isfinite(lambda))
    d.next = LM_TERMINATE;
  return d;
}

// The damping of trial q of an iteration that starts with (lambda, ni): the reject rule above, q times -- the system and the estimate a
// rejected trial started from stay, so every trial's damping is known when the system is built (k_pose_only_reg and k_sim3_optimize solve
// all LM_TRIALS of them at once).  tests/cpp/test_lm_ctrl.cpp holds it against q rejects of lm_decide.
ORBFE_HD_INLINE double lm6_trial_lambda(double lambda, double ni, int q) {
  ORBFE_FP_STRICT
  double lam = lambda, nu = ni;
  for (int k = 0; k < q; ++k) lam *= nu, nu *= 2;
  return lam;
}

}  // namespace orbfe
