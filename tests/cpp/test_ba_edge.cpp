// The edge model of the optimiser kernels (csrc/ba_edge_dev.h) and the SE3 helpers under it (csrc/se3_dev.h), compiled by the host
// compiler alone and run on the problems tests/test_se3_general_rotations.py writes: the same source lines the gfx950 kernels inline.
//   test_ba_edge IN OUT
// IN  (little-endian doubles): n_problems, then per problem  NK NP E | fx fy cx cy bf | poses [NK][7] | points [NP][3] | edge_pose [E] |
//     edge_point [E] | meas [E][3] | is_stereo [E] | info [E] | huber_delta [E];  then n_oplus | poses [n][7] | updates [n][6]
// OUT (doubles): per problem  error [E][3] | chi2 [E] | rho [E][2] | j_point [E][9] | j_pose [E][18] | the pose-only j_pose [E][18] |
//     depth_positive [E] | outlier [E];  then the oplus results [n][7]
// The damped 3x3 inverse is checked here (it needs no reference).  Prints OK and returns 0 when everything ran.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ba_edge_dev.h"

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

static int check_inverse() {
  // well-conditioned symmetric blocks (a point's A^T W A plus damping); M * inv(M) = I to a few ulp of cond(M) ~ 10
  const double blocks[3][9] = {{4, 1, 0.5, 1, 3, 0.25, 0.5, 0.25, 2},
                               {2500, -300, 120, -300, 1800, 75, 120, 75, 900},
                               {1e-3, 2e-4, -1e-4, 2e-4, 3e-3, 5e-4, -1e-4, 5e-4, 2e-3}};
  const double lambdas[3] = {0.0, 12.5, 1e-4};
  for (int b = 0; b < 3; ++b) {
    double D[9];
    if (!inv3_damped(blocks[b], lambdas[b], D)) return fprintf(stderr, "inv3_damped refused block %d\n", b), 1;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += (blocks[b][3 * i + k] + (i == k ? lambdas[b] : 0.0)) * D[3 * k + j];
        if (!(std::fabs(s - (i == j ? 1.0 : 0.0)) < 1e-14)) return fprintf(stderr, "inv3_damped block %d: (M D)[%d][%d] = %.17g\n", b, i, j, s), 1;
      }
  }
  // det == 0 (a rank-1 block without damping, a zero block) and a non-finite determinant are refused, D untouched
  const double rank1[9] = {1, 2, 3, 2, 4, 6, 3, 6, 9}, zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, huge[9] = {1e200, 0, 0, 0, 1e200, 0, 0, 0, 1e200};
  double D[9] = {7, 7, 7, 7, 7, 7, 7, 7, 7};
  if (inv3_damped(rank1, 0.0, D) || inv3_damped(zero, 0.0, D) || inv3_damped(huge, 0.0, D)) return fprintf(stderr, "inv3_damped took a singular block\n"), 1;
  for (int i = 0; i < 9; ++i)
    if (D[i] != 7) return fprintf(stderr, "inv3_damped wrote a refused inverse\n"), 1;
  if (!inv3_damped(rank1, 0.5, D)) return fprintf(stderr, "inv3_damped refused a damped rank-1 block\n"), 1;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  if (check_inverse()) return 1;
  const std::vector<double> in = read_all(argv[1]);
  Reader r{in};
  std::vector<double> out;
  const int n_prob = r.count();
  for (int q = 0; q < n_prob; ++q) {
    const int NK = r.count(), NP = r.count(), E = r.count();
    const double* cam = r.take(5);
    const BaParamsDev prm = {cam[0], cam[1], cam[2], cam[3], cam[4]};
    const double *poses = r.take((size_t)NK * 7), *points = r.take((size_t)NP * 3), *ek = r.take(E), *ep = r.take(E), *meas = r.take((size_t)E * 3),
                 *st = r.take(E), *info = r.take(E), *delta = r.take(E);
    std::vector<double> err((size_t)E * 3), chi(E), rho((size_t)E * 2), jpt((size_t)E * 9), jps((size_t)E * 18), jpo((size_t)E * 18), dp(E), bad(E);
    for (int e = 0; e < E; ++e) {
      const int k = (int)ek[e], pt = (int)ep[e];
      if (k < 0 || k >= NK || pt < 0 || pt >= NP) return fprintf(stderr, "problem %d: edge %d names no vertex\n", q, e), 2;
      const double* T = poses + (size_t)k * 7;
      const bool stereo = st[e] != 0;
      double p[3];
      se3_map(T, T + 4, points + (size_t)pt * 3, p);
      ba_edge_error(p, meas + (size_t)e * 3, stereo, prm, &err[(size_t)e * 3]);
      chi[e] = ba_edge_chi2(&err[(size_t)e * 3], info[e], stereo);
      ba_edge_robustify(chi[e], delta[e], rho[(size_t)e * 2], rho[(size_t)e * 2 + 1]);
      ba_edge_jpoint(T, p, stereo, prm, &jpt[(size_t)e * 9]);
      ba_edge_jpose(p, stereo, prm, &jps[(size_t)e * 18]);
      pose_edge_jpose(p, stereo, prm, &jpo[(size_t)e * 18]);
      dp[e] = ba_depth_positive(p) ? 1.0 : 0.0;
      bad[e] = ba_edge_outlier(chi[e], stereo, ba_depth_positive(p)) ? 1.0 : 0.0;
    }
    for (const std::vector<double>* v : {&err, &chi, &rho, &jpt, &jps, &jpo, &dp, &bad}) out.insert(out.end(), v->begin(), v->end());
  }
  const int n_op = r.count();
  const double *op = r.take((size_t)n_op * 7), *ou = r.take((size_t)n_op * 6);
  for (int i = 0; i < n_op; ++i) {
    PoseDev T, Tn;
    for (int k = 0; k < 4; ++k) T.q[k] = op[(size_t)i * 7 + k];
    for (int k = 0; k < 3; ++k) T.t[k] = op[(size_t)i * 7 + 4 + k];
    pose_oplus(T, ou + (size_t)i * 6, Tn);
    out.insert(out.end(), Tn.q, Tn.q + 4);
    out.insert(out.end(), Tn.t, Tn.t + 3);
  }
  if (r.at != in.size()) return fprintf(stderr, "input has %zu doubles left over\n", in.size() - r.at), 2;
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || fclose(f) != 0) return perror(argv[2]), 2;
  printf("OK %d problems, %d exp-map cases\n", n_prob, n_op);
  return 0;
}
