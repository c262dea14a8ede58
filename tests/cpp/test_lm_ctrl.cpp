// The Levenberg-Marquardt controller of the optimisers (csrc/lm_ctrl.h), compiled by the host compiler alone and run on the tables
// tests/test_lm_ctrl.py writes: the same source lines the gfx950 kernels and the host loop inline, to be compared with that test's
// restatement of g2o's rule.
//   test_lm_ctrl IN OUT
// IN  (little-endian doubles):
//   n_case | case [n_case][9] = op lambda ni current_chi qmax a b c d    op 0: lm_begin_iteration(chi = a, it = b, maxdiag = c)
//                                                                        op 1: lm_decide(trial_chi = a, scale = b, ok = c, stopped = d)
//   n_damp | (lambda, ni) [n_damp][2]
//   n_loop | per loop: iterations chi0 maxdiag n_trial | trial [n_trial][14] = chi ok x[6] b[6]
// OUT (doubles):
//   per case: lambda ni current_chi qmax accepted next (the last two -1 for op 0)
//   per (lambda, ni) and q = 0 .. 9: lm6_trial_lambda(lambda, ni, q) | lambda after q rejected lm_decide | qmax after them
//   per loop, twice -- as the host's do-while (lm_host.h) and as the state machine of k_pose_only_reg / k_sim3_optimize, whose trial
//   dampings come from lm6_trial_lambda: n_row | row [n_row][6] = it qmax lambda accepted next trial_lambda
// Prints OK and returns 0 when everything ran.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lm_ctrl.h"

using namespace orbfe;

static std::vector<double> read_all(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  std::vector<double> v;
  double buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(double), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

struct Reader {
  const std::vector<double>& v;
  size_t at = 0;
  const double* take(size_t n) {
    if (at + n > v.size()) {
      fprintf(stderr, "input ends early (%zu + %zu > %zu)\n", at, n, v.size());
      exit(2);
    }
    const double* p = v.data() + at;
    at += n;
    return p;
  }
  int count() { return (int)*take(1); }
};

struct Loop {
  int iterations, n_trial;
  double chi0, maxdiag;
  const double* trial;  // [n_trial][14]
};

// computeScale as the kernels spell it (lm6_dev.h, a device-only header): sum of x_j (lambda x_j + b_j), j = 0 .. 5
static double scale6(const double* x, double lambda, const double* b) {
  double scale = 0;
  for (int j = 0; j < 6; ++j) scale += x[j] * (lambda * x[j] + b[j]);
  return scale;
}

static void row(std::vector<double>& out, int it, int qmax, double lambda, const LmDecision& d, double trial_lambda) {
  const double r[6] = {(double)it, (double)qmax, lambda, d.accepted ? 1.0 : 0.0, (double)d.next, trial_lambda};
  out.insert(out.end(), r, r + 6);
}

// SparseOptimizer::optimize as lm_host.h drives it; the table is the device: a trial's chi2 is the next row, whatever the estimate
static void host_loop(const Loop& L, std::vector<double>& out) {
  int at = 0;
  double lambda = 0, ni = 2, current_chi = 0, est_chi = L.chi0;
  int qmax = 0;
  for (int it = 0; it < L.iterations; ++it) {
    lm_begin_iteration(lambda, ni, current_chi, qmax, est_chi, it, L.maxdiag);
    LmDecision d;
    do {
      if (at == L.n_trial) return;
      const double* t = L.trial + 14 * at++;
      const double used = lambda;
      d = lm_decide(lambda, ni, current_chi, qmax, t[0], scale6(t + 2, lambda, t + 8), t[1] != 0, false);
      if (d.accepted) est_chi = t[0];
      row(out, it, qmax, lambda, d, used);
    } while (d.next == LM_RETRY);
    if (d.next == LM_TERMINATE) break;
  }
}

// the same loop as ONE state machine with a single evaluation site (k_pose_only_reg, k_sim3_optimize): a pass either evaluates the current
// estimate (an iteration starts) or a trial, whose damping was fixed when the system was built
static void state_machine(const Loop& L, std::vector<double>& out) {
  int at = 0;
  double est_chi = L.chi0;  // chi2 at Tb
  int it = 0;
  bool do_solve = false;
  double chi_cur = 0, current_chi = 0, lambda = 0, ni = 2, lambda0 = 0, ni0 = 2;
  int qmax = 0;
  const double* t = nullptr;
  if (L.iterations <= 0) return;
  for (;;) {
    double chi = est_chi;
    if (do_solve) {
      if (at == L.n_trial) return;
      t = L.trial + 14 * at++;
      chi = t[0];
    }
    if (!do_solve) {
      chi_cur = chi;
    } else {
      const double used = lm6_trial_lambda(lambda0, ni0, qmax);  // trial qmax of this iteration: what lane qmax solved with
      const LmDecision d = lm_decide(lambda, ni, current_chi, qmax, chi, scale6(t + 2, lambda, t + 8), t[1] != 0, false);
      if (d.accepted) est_chi = chi;
      row(out, it, qmax, lambda, d, used);
      if (d.next == LM_RETRY) continue;
      if (d.next == LM_TERMINATE) break;
      if (++it == L.iterations) break;
      if (!d.accepted) {
        do_solve = false;
        continue;
      }
      chi_cur = chi;
    }
    lm_begin_iteration(lambda, ni, current_chi, qmax, chi_cur, it, L.maxdiag);
    lambda0 = lambda, ni0 = ni;
    do_solve = true;
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  const std::vector<double> in = read_all(argv[1]);
  Reader r{in};
  std::vector<double> out;
  const int n_case = r.count();
  for (int k = 0; k < n_case; ++k) {
    const double* p = r.take(9);
    double lambda = p[1], ni = p[2], current_chi = p[3];
    int qmax = (int)p[4];
    double accepted = -1, next = -1;
    if (p[0] == 0) {
      lm_begin_iteration(lambda, ni, current_chi, qmax, p[5], (int)p[6], p[7]);
    } else {
      const LmDecision d = lm_decide(lambda, ni, current_chi, qmax, p[5], p[6], p[7] != 0, p[8] != 0);
      accepted = d.accepted ? 1 : 0, next = d.next;
    }
    const double o[6] = {lambda, ni, current_chi, (double)qmax, accepted, next};
    out.insert(out.end(), o, o + 6);
  }
  const int n_damp = r.count();
  for (int k = 0; k < n_damp; ++k) {
    const double* p = r.take(2);
    for (int q = 0; q < LM_TRIALS; ++q) {
      double lambda = p[0], ni = p[1], current_chi = 1.0;
      int qmax = 0;
      for (int j = 0; j < q; ++j) lm_decide(lambda, ni, current_chi, qmax, 2.0, 1.0, true, false);  // chi2 rises: rejected
      const double o[3] = {lm6_trial_lambda(p[0], p[1], q), lambda, (double)qmax};
      out.insert(out.end(), o, o + 3);
    }
  }
  const int n_loop = r.count();
  for (int k = 0; k < n_loop; ++k) {
    const double* h = r.take(4);
    Loop L = {(int)h[0], (int)h[3], h[1], h[2], nullptr};
    L.trial = r.take((size_t)14 * L.n_trial);
    for (int form = 0; form < 2; ++form) {
      std::vector<double> rows;
      if (form == 0) host_loop(L, rows); else state_machine(L, rows);
      out.push_back((double)(rows.size() / 6));
      out.insert(out.end(), rows.begin(), rows.end());
    }
  }
  if (r.at != in.size()) return fprintf(stderr, "%zu doubles of input left over\n", in.size() - r.at), 2;
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return perror(argv[2]), 2;
  fclose(f);
  printf("OK %d cases, %d dampings, %d loops\n", n_case, n_damp, n_loop);
  return 0;
}
