// test_pg_symbolic.cpp -- csrc/pg_symbolic.h and csrc/pg_chol_dev.h in a stand-alone program (host compiler, address + undefined-behaviour
// sanitizers): the symbolic phase of the pose graph's block-sparse Cholesky, and a whole numeric factorisation and solve over that
// structure on the host, step for step what k_pgs_solve does on the device with the same block arithmetic (the kernel's fixed-step
// binary search for an update's target included).
// stdin: nb n_pairs n_low, then (i j)[n_pairs] in any orientation, then per given block: row col v[36] (row-major, row >= col), then
// rhs[6 nb] if n_low > 0.  stdout: the structure, one array a line; with n_low > 0 also `ok`, `L` (the factor's storage) and `x`, as
// hexadecimal floats.  tests/test_pg_sparse_host.py compares with its own restatement and with numpy.
#include <cstdio>
#include <vector>

#include "pg_chol_dev.h"
#include "pg_symbolic.h"

template <class T>
static void line(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (T x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}

static void line_f(const char* name, const std::vector<double>& v) {
  std::printf("%s", name);
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

// the target of an update as k_pgs_update finds it: block (ra, rb), ra > rb, among the rows below the diagonal of column rb
static int64_t find_fixed_steps(const PgSymbolic& s, int32_t ra, int32_t rb) {
  int64_t lo = s.col_off[(size_t)rb] + 1, hi = s.col_off[(size_t)rb + 1];
  for (int32_t step = 0; step < s.search_steps; ++step)
    if (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (s.row[(size_t)mid] < ra) lo = mid + 1;
      else hi = mid;
    }
  return lo;
}

int main() {
  int nb, np, n_low;
  if (std::scanf("%d %d %d", &nb, &np, &n_low) != 3) return 2;
  std::vector<int32_t> pi(np), pj(np);
  for (int q = 0; q < np; ++q)
    if (std::scanf("%d %d", &pi[q], &pj[q]) != 2) return 2;
  PgSymbolic s;
  pg_symbolic(nb, (size_t)np, pi.data(), pj.data(), &s);
  // twice: the structure does not depend on what the object held before
  pg_symbolic(nb, (size_t)np, pi.data(), pj.data(), &s);
  if (s.nb != nb || (int)s.col_off.size() != nb + 1 || s.l_blocks() != s.col_off[(size_t)nb]) return 3;
  std::vector<int64_t> pos(np);
  for (int q = 0; q < np; ++q) pos[q] = pg_symbolic_pos(s, std::max(pi[q], pj[q]), std::min(pi[q], pj[q]));
  line("parent", s.parent), line("col_off", s.col_off), line("row", s.row), line("pos", pos);
  std::printf("max_col %d\nsearch_steps %d\n", s.max_col, s.search_steps);
  if (nb > 0 && (pg_symbolic_pos(s, nb - 1, 0) >= 0) != (s.row[(size_t)s.col_off[1] - 1] == nb - 1)) return 3;
  if (n_low <= 0) return 0;

  using namespace orbfe;
  std::vector<double> L((size_t)s.l_blocks() * 36, 0.0), x((size_t)6 * nb);
  for (int q = 0; q < n_low; ++q) {
    int r, c;
    if (std::scanf("%d %d", &r, &c) != 2) return 2;
    const int64_t p = pg_symbolic_pos(s, r, c);
    if (p < 0) return 4;
    for (int k = 0; k < 36; ++k)
      if (std::scanf("%lf", &L[(size_t)p * 36 + k]) != 1) return 2;
  }
  for (double& v : x)
    if (std::scanf("%lf", &v) != 1) return 2;
  bool ok = true;
  for (int k = 0; k < nb && ok; ++k) {
    const int64_t q0 = s.col_off[(size_t)k];
    const int m = (int)(s.col_off[(size_t)k + 1] - q0 - 1);
    double* Lk = &L[(size_t)q0 * 36];
    if (!pg_chol6(Lk)) {  // F2
      ok = false;
      break;
    }
    for (int r = 0; r < 6 * m; ++r) pg_row_solve6(Lk, Lk + 36 + 6 * r, Lk + 36 + 6 * r);  // F3
    double* yk = &x[(size_t)6 * k];
    pg_row_solve6(Lk, yk, yk);
    const double* P = Lk + 36;
    const int32_t* rows = &s.row[(size_t)q0 + 1];
    for (int a = 0; a < m; ++a) {  // F4
      for (int b = 0; b <= a; ++b) {
        const int64_t t = a == b ? s.col_off[(size_t)rows[b]] : find_fixed_steps(s, rows[a], rows[b]);
        if (t >= s.l_blocks() || s.row[(size_t)t] != rows[a] || t < s.col_off[(size_t)rows[b]] || t >= s.col_off[(size_t)rows[b] + 1]) return 5;
        for (int i = 0; i < 6; ++i)
          for (int j = 0; j < 6; ++j)
            if (a != b || j <= i) L[(size_t)t * 36 + 6 * i + j] -= pg_dot6(P + 36 * a + 6 * i, P + 36 * b + 6 * j);
      }
      for (int i = 0; i < 6; ++i) x[(size_t)6 * rows[a] + i] -= pg_dot6(P + 36 * a + 6 * i, yk);  // F5
    }
  }
  std::printf("ok %d\n", ok ? 1 : 0);
  if (!ok) return 0;
  for (int k = nb - 1; k >= 0; --k) {  // F6
    const int64_t q0 = s.col_off[(size_t)k];
    const int m = (int)(s.col_off[(size_t)k + 1] - q0 - 1);
    double part[8][6] = {};
    for (int w = 0; w < 8; ++w)
      for (int c = 0; c < 6; ++c)
        for (int a = w; a < m; a += 8)
          for (int i = 0; i < 6; ++i) part[w][c] += L[(size_t)(q0 + 1 + a) * 36 + 6 * i + c] * x[(size_t)6 * s.row[(size_t)q0 + 1 + a] + i];
    double v[6];
    for (int c = 0; c < 6; ++c) {
      double g = part[0][c];
      for (int w = 1; w < 8; ++w) g += part[w][c];
      v[c] = x[(size_t)6 * k + c] - g;
    }
    pg_back6(&L[(size_t)q0 * 36], v);
    for (int c = 0; c < 6; ++c) x[(size_t)6 * k + c] = v[c];
  }
  line_f("L", L), line_f("x", x);
  return 0;
}
