// The edge model of the pose-graph optimiser (csrc/posegraph_edge_dev.h), compiled by the host compiler alone and run on the cases
// tests/test_essential_graph_host.py writes: the same source lines the gfx950 kernels inline, to be compared with
// tests/essential_graph_restatement.py.
//   test_posegraph_edge IN OUT
// IN  (little-endian doubles): n_v | est [n_v][8] | n_e | edges [n_e][10] = v0 v1 meas[8] | n_log | S [n_log][8] | n_lu | M [n_lu][12]
// OUT (doubles): per edge err [6] | chi2 | J0 [6][6] | J1 [6][6] (pg_edge_jacobians) | the same two Jacobians again, column by column from
//     the 25 evaluations of pg_edge_eval as k_pg_build pairs them;  log(S) [n_log][6];  pg_lu3_solve(M) [n_lu][3]
// Prints OK and returns 0 when everything ran.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "posegraph_edge_dev.h"

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

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  const std::vector<double> in = read_all(argv[1]);
  Reader r{in};
  std::vector<double> out;
  const int n_v = r.count();
  const double* ests = r.take(8 * (size_t)n_v);
  const int n_e = r.count();
  const double* edges = r.take(10 * (size_t)n_e);
  for (int i = 0; i < n_e; ++i) {
    const double* p = edges + 10 * (size_t)i;
    const int v0 = (int)p[0], v1 = (int)p[1];
    if (v0 < 0 || v0 >= n_v || v1 < 0 || v1 >= n_v) return fprintf(stderr, "edge %d: vertex out of range\n", i), 2;
    const Sim3Dev C = sim3_of(p + 2), S0 = sim3_of(ests + 8 * (size_t)v0), S1 = sim3_of(ests + 8 * (size_t)v1);
    double e[6], J0[6][6], J1[6][6];
    pg_edge_error(C, S0, S1, e);
    pg_edge_jacobians(C, S0, S1, J0, J1);
    out.insert(out.end(), e, e + 6);
    out.push_back(pg_edge_chi2(e));
    out.insert(out.end(), &J0[0][0], &J0[0][0] + 36);
    out.insert(out.end(), &J1[0][0], &J1[0][0] + 36);
    double E[PG_N_EVAL][6];
    for (int k = 0; k < PG_N_EVAL; ++k) pg_edge_eval(C, S0, S1, k, E[k]);
    for (int w = 0; w < 2; ++w)
      for (int row = 0; row < 6; ++row)
        for (int d = 0; d < 6; ++d) out.push_back(sim3_num_diff(E[(w ? 13 : 1) + 2 * d][row], E[(w ? 14 : 2) + 2 * d][row]));
  }
  const int n_log = r.count();
  const double* Ss = r.take(8 * (size_t)n_log);
  for (int i = 0; i < n_log; ++i) {
    double l[6];
    sim3_log(sim3_of(Ss + 8 * (size_t)i), l);
    out.insert(out.end(), l, l + 6);
  }
  const int n_lu = r.count();
  const double* Ms = r.take(12 * (size_t)n_lu);
  for (int i = 0; i < n_lu; ++i) {
    double M[3][4], x[3];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 4; ++b) M[a][b] = Ms[12 * (size_t)i + 4 * a + b];
    pg_lu3_solve(M, x);
    out.insert(out.end(), x, x + 3);
  }
  if (r.at != in.size()) return fprintf(stderr, "%zu doubles of input left over\n", in.size() - r.at), 2;
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || fclose(f) != 0) return perror(argv[2]), 2;
  printf("OK %zu doubles\n", out.size());
  return 0;
}
