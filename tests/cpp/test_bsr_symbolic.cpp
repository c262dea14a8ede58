// test_bsr_symbolic.cpp -- csrc/bsr_symbolic.h in a stand-alone program (host compiler, address + undefined-behaviour sanitizers).
// stdin: n_poses n_points n_edges, then slot[n_poses], then (edge_pose edge_point)[n_edges].  stdout: the structure, one array a line,
// for tests/test_global_ba_host.py to compare with the restatement.
#include <cstdio>
#include <vector>

#include "bsr_symbolic.h"

static void line(const char* name, const std::vector<int32_t>& v) {
  std::printf("%s", name);
  for (int32_t x : v) std::printf(" %d", x);
  std::printf("\n");
}

int main() {
  int nk, np, ne;
  if (std::scanf("%d %d %d", &nk, &np, &ne) != 3) return 2;
  std::vector<int32_t> slot(nk), ek(ne), ep(ne);
  int nf = 0;
  for (int k = 0; k < nk; ++k) {
    if (std::scanf("%d", &slot[k]) != 1) return 2;
    if (slot[k] >= 0) ++nf;
  }
  for (int e = 0; e < ne; ++e)
    if (std::scanf("%d %d", &ek[e], &ep[e]) != 2) return 2;
  // point -> edges lists, edges ascending (a counting sort, as the entry points build them)
  std::vector<int32_t> off(np + 1, 0), list(ne);
  for (int e = 0; e < ne; ++e) ++off[ep[e] + 1];
  for (int p = 0; p < np; ++p) off[p + 1] += off[p];
  std::vector<int32_t> cur(off.begin(), off.end() - 1);
  for (int e = 0; e < ne; ++e) list[cur[ep[e]]++] = e;
  BsrSymbolic s;
  bsr_symbolic(nf, np, off.data(), list.data(), ek.data(), slot.data(), &s);
  // twice: the structure does not depend on what the object held before
  bsr_symbolic(nf, np, off.data(), list.data(), ek.data(), slot.data(), &s);
  if (s.nb != nf || (int)s.row_off.size() != nf + 1 || s.nnzb() != s.row_off[nf]) return 3;
  line("row_off", s.row_off), line("col", s.col), line("twin", s.twin), line("low", s.low), line("low_row", s.low_row);
  line("pair_off", s.pair_off), line("pairs", s.pairs);
  return 0;
}
