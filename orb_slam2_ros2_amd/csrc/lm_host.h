// lm_host.h -- SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve as the ONE host-driven loop of the local
// BA (host path), the global BA and the pose graph.  The loop owns the skeleton (for / do-while, iterations started, trials taken, the
// stop-flag poll), the five scalars it exchanges with the device and the controller's decisions (lm_ctrl.h); the caller owns the kernels.
//
// d_sc, five doubles of device memory: [0] robust chi2 of the last evaluation, [1] max diagonal (written at it == 0), [2] lambda and
// [3] ok (int, the two the loop uploads before a trial: the solver kernels read the one and clear the other), [4] computeScale's sum.
//
// The caller's steps, each enqueueing on `st` and returning an orbfe_status:
//   linearize(it)              computeActiveErrors + buildSystem at the current estimate -> d_sc[0], and d_sc[1] at it == 0
//   trial(lambda, solver_ok)   push, lm_host_upload(lambda) -- behind the push copies, where the loops always had it --, solve with
//                              d_sc[2], update, evaluate -> d_sc[0], d_sc[3], d_sc[4]; clears solver_ok where the failure of its solver
//                              is known to the host only
//   on_accept()                the trial estimate is the current one
//   on_reject(ok)              pop; ok: whether the linear solve had succeeded
//   lap(phase)                 the phase clocks' hook, called right behind a read-back: 0 after linearize's, 3 after trial's
// One read-back with one synchronisation follows linearize and trial each; nothing else here waits for the device.  The stop flag is
// read at the top of an iteration and once behind every trial (the loops this replaces read it there only when the trial was about to
// be retried: the same decisions, a volatile byte read more).
#pragma once
#include "lm_ctrl.h"
#include "orbfe_ctx.h"

namespace {

struct HostScalars {
  double chi, maxdiag, lambda;
  int32_t ok, pad;
  double scale;
};

// the {lambda, ok} a trial's solver kernels read and clear: d_sc[2], d_sc[3]
inline hipError_t lm_host_upload(hipStream_t st, double* d_sc, double lambda) {
  const struct {
    double lambda;
    int32_t ok, pad;
  } upv = {lambda, 1, 0};
  return hipMemcpyAsync(d_sc + 2, &upv, sizeof upv, hipMemcpyHostToDevice, st);
}

template <class Linearize, class Trial, class Accept, class Reject, class Lap>
orbfe_status lm_host_optimize(orbfe_ctx* c, hipStream_t st, double* d_sc, int iterations, const volatile uint8_t* stop_flag, int32_t& done,
                              int32_t& trials, Linearize linearize, Trial trial, Accept on_accept, Reject on_reject, Lap lap) {
  auto read_scalars = [&](HostScalars& h) -> hipError_t {
    hipError_t e = hipMemcpyAsync(&h, d_sc, sizeof h, hipMemcpyDeviceToHost, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
  };
  auto stopped = [&]() { return stop_flag && *stop_flag; };
  done = 0, trials = 0;
  double lambda = 0, ni = 2, current_chi = 0;
  int qmax = 0;
  for (int it = 0; it < iterations; ++it) {
    if (stopped()) break;
    ++done;
    TRY(linearize(it));
    HostScalars h;
    HIP_TRY(c, read_scalars(h));
    lap(0);
    lm_begin_iteration(lambda, ni, current_chi, qmax, h.chi, it, h.maxdiag);
    LmDecision d;
    do {
      bool solver_ok = true;
      TRY(trial(lambda, solver_ok));
      HIP_TRY(c, read_scalars(h));
      lap(3);
      ++trials;
      const bool ok = h.ok != 0 && solver_ok;
      d = lm_decide(lambda, ni, current_chi, qmax, h.chi, h.scale, ok, stopped());
      TRY(d.accepted ? on_accept() : on_reject(ok));
    } while (d.next == LM_RETRY);
    if (d.next == LM_TERMINATE) break;
  }
  return ORBFE_OK;
}

}  // namespace
