// The edge model of the Sim3 optimiser (csrc/sim3_edge_dev.h), compiled by the host compiler alone and run on the cases
// tests/test_sim3_opt_host.py writes: the same source lines the gfx950 kernel inlines, to be compared with tests/sim3_opt_restatement.py
// bit for bit.
//   test_sim3_edge IN OUT
// IN  (little-endian doubles): fx fy cx cy | n_est | est [n_est][8] | n | pairs [n][12] = pc pm uv_c uv_m info_c info_m |
//     n_chi | chi2 [n_chi] | delta [n_chi] | n_exp | upd [n_exp][6] | n_mul | A [n_mul][8] | B [n_mul][8] | n_model | model [n_model][12]
// OUT (doubles): per estimate: inverse [8], then per pair err [4] | chi2 [2] | jac [4][6];  rho, rho' [n_chi][2];  exp(upd) [n_exp][8];
//     oplus(est 0, upd) [n_exp][8];  A * B [n_mul][8];  per model: from_model [8] | to_model(from_model) [12]
// Prints OK and returns 0 when everything ran.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sim3_edge_dev.h"

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

static Sim3Dev sim3_of(const double* p) {
  Sim3Dev S;
  for (int k = 0; k < 4; ++k) S.q[k] = p[k];
  for (int k = 0; k < 3; ++k) S.t[k] = p[4 + k];
  S.s = p[7];
  return S;
}
static void push(std::vector<double>& out, const Sim3Dev& S) {
  out.insert(out.end(), S.q, S.q + 4);
  out.insert(out.end(), S.t, S.t + 3);
  out.push_back(S.s);
}

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  const std::vector<double> in = read_all(argv[1]);
  Reader r{in};
  std::vector<double> out;
  const double* cam = r.take(4);
  const BaParamsDev prm = {cam[0], cam[1], cam[2], cam[3], 0.0};
  const int n_est = r.count();
  const double* ests = r.take(8 * (size_t)n_est);
  const int n = r.count();
  const double* pairs = r.take(12 * (size_t)n);
  for (int k = 0; k < n_est; ++k) {
    const Sim3Dev S = sim3_of(ests + 8 * k);
    Sim3Dev Si;
    sim3_inverse(S, Si);
    push(out, Si);
    for (int i = 0; i < n; ++i) {
      const double* p = pairs + 12 * (size_t)i;
      const Sim3Pair P = {{p[0], p[1], p[2]}, {p[3], p[4], p[5]}, {p[6], p[7]}, {p[8], p[9]}, p[10], p[11]};
      double e[4], c[2], J[4][6];
      sim3_pair_errors(S, Si, P, prm, e);
      sim3_pair_chi2(e, P, c);
      sim3_pair_jacobian(S, P, prm, J);
      out.insert(out.end(), e, e + 4);
      out.insert(out.end(), c, c + 2);
      out.insert(out.end(), &J[0][0], &J[0][0] + 24);
    }
  }
  const int n_chi = r.count();
  const double *chi = r.take((size_t)n_chi), *delta = r.take((size_t)n_chi);
  for (int i = 0; i < n_chi; ++i) {
    double rho, drho;
    huber_robustify(chi[i], delta[i], rho, drho);
    out.push_back(rho);
    out.push_back(drho);
  }
  const int n_exp = r.count();
  const double* upd = r.take(6 * (size_t)n_exp);
  for (int i = 0; i < n_exp; ++i) {
    Sim3Dev E;
    sim3_exp(upd + 6 * i, E);
    push(out, E);
  }
  for (int i = 0; i < n_exp && n_est > 0; ++i) {
    Sim3Dev E;
    sim3_oplus(sim3_of(ests), upd + 6 * i, E);
    push(out, E);
  }
  const int n_mul = r.count();
  const double *A = r.take(8 * (size_t)n_mul), *B = r.take(8 * (size_t)n_mul);
  for (int i = 0; i < n_mul; ++i) {
    Sim3Dev C;
    sim3_mul(sim3_of(A + 8 * i), sim3_of(B + 8 * i), C);
    push(out, C);
  }
  const int n_model = r.count();
  const double* models = r.take(12 * (size_t)n_model);
  for (int i = 0; i < n_model; ++i) {
    float m[12], back[12];
    for (int k = 0; k < 12; ++k) m[k] = (float)models[12 * i + k];
    Sim3Dev S;
    sim3_from_model(m, S);
    push(out, S);
    sim3_to_model(S, back);
    for (int k = 0; k < 12; ++k) out.push_back((double)back[k]);
  }
  if (r.at != in.size()) return fprintf(stderr, "%zu doubles of input left over\n", in.size() - r.at), 2;
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || fclose(f) != 0) return perror(argv[2]), 2;
  printf("OK %zu doubles\n", out.size());
  return 0;
}
