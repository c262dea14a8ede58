// pg_symbolic.h -- the symbolic phase of the pose graph's block-sparse Cholesky (k_pgsparse.hip), built on the host once per call.  Host
// only: no HIP header, so tests/cpp/test_pg_symbolic.cpp compiles it with the host compiler alone.
//
// The matrix is Hpp + lambda I of Optimizer::optimizeEssentialGraph in 6x6 blocks: block row k is non-fixed vertex k in vertex order
// (no reordering: keyframe ids are nearly a time order, so the links of an essential graph make a band and a loop connection costs one
// long row), block (i, j), i > j, exists iff an edge joins the two.  Out comes the structure of its Cholesky factor L (rule F1 of DESIGN
// 4.26): the elimination tree, parent[k] = the first row below the diagonal of column k (-1: none), and every column's rows, the
// diagonal first and then ascending -- struct(k) = rows of column k of the matrix, united with struct(c) \ {c, k} of every child c
// of k.  L's storage is the columns one after another, 36 doubles a block; block (i, j) sits at pg_symbolic_pos(i, j).  The numeric
// kernel needs no further list: it finds the target of an update by a binary search in the target column's rows, `search_steps` steps.
// Memory is O(blocks of L): no nb x nb table.  Everything is deterministic: the input order of the pairs does not matter.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

struct PgSymbolic {
  int32_t nb = 0;                 // block rows
  std::vector<int32_t> parent;    // [nb] elimination tree
  std::vector<int64_t> col_off;   // [nb + 1] first block of every column in L's storage
  std::vector<int32_t> row;       // [l_blocks] block row of every stored block
  int32_t max_col = 0;            // blocks of the longest column, the diagonal included
  int32_t search_steps = 0;       // halvings that find any row in any column: the smallest s with 2^s >= max_col
  int64_t l_blocks() const { return (int64_t)row.size(); }
};

// the pairs (pi[q], pj[q]), q < n_pairs, in either orientation and any number of times each; pi[q] != pj[q], both in [0, nb)
inline void pg_symbolic(int32_t nb, size_t n_pairs, const int32_t* pi, const int32_t* pj, PgSymbolic* s) {
  const size_t NB = (size_t)std::max(nb, 0);
  // the matrix's own rows below the diagonal, column by column (a counting sort; duplicates go at the merge)
  std::vector<int64_t> a_off(NB + 1, 0);
  for (size_t q = 0; q < n_pairs; ++q) ++a_off[(size_t)std::min(pi[q], pj[q]) + 1];
  for (size_t k = 0; k < NB; ++k) a_off[k + 1] += a_off[k];
  std::vector<int32_t> a_row((size_t)a_off[NB]);
  {
    std::vector<int64_t> cur(a_off.begin(), a_off.end() - 1);
    for (size_t q = 0; q < n_pairs; ++q) a_row[(size_t)cur[(size_t)std::min(pi[q], pj[q])]++] = std::max(pi[q], pj[q]);
  }
  s->nb = nb, s->max_col = 0, s->search_steps = 0;
  s->parent.assign(NB, -1), s->col_off.assign(NB + 1, 0), s->row.clear();
  // the children of every vertex as linked lists (a child is always a smaller index: its column is complete when the parent's is built)
  std::vector<int32_t> first_child(NB, -1), next_sibling(NB, -1), mark(NB, -1), rows;
  for (size_t k = 0; k < NB; ++k) {
    rows.clear();
    mark[k] = (int32_t)k;
    auto take = [&](int32_t r) {
      if (mark[(size_t)r] != (int32_t)k) mark[(size_t)r] = (int32_t)k, rows.push_back(r);
    };
    for (int64_t q = a_off[k]; q < a_off[k + 1]; ++q) take(a_row[(size_t)q]);
    for (int32_t c = first_child[k]; c >= 0; c = next_sibling[(size_t)c])
      for (int64_t q = s->col_off[(size_t)c] + 1; q < s->col_off[(size_t)c + 1]; ++q) take(s->row[(size_t)q]);
    std::sort(rows.begin(), rows.end());
    s->row.push_back((int32_t)k);
    s->row.insert(s->row.end(), rows.begin(), rows.end());
    s->col_off[k + 1] = (int64_t)s->row.size();
    s->max_col = std::max(s->max_col, (int32_t)rows.size() + 1);
    if (!rows.empty()) {
      const size_t p = (size_t)rows[0];
      s->parent[k] = rows[0];
      next_sibling[k] = first_child[p], first_child[p] = (int32_t)k;
    }
  }
  while (((int64_t)1 << s->search_steps) < s->max_col) ++s->search_steps;
}

// the place of block (i, j), i >= j, in L's storage; -1: not in the structure
inline int64_t pg_symbolic_pos(const PgSymbolic& s, int32_t i, int32_t j) {
  const int32_t* b = s.row.data() + s.col_off[(size_t)j];
  const int32_t* e = s.row.data() + s.col_off[(size_t)j + 1];
  if (i == j) return s.col_off[(size_t)j];
  const int32_t* p = std::lower_bound(b + 1, e, i);
  return p != e && *p == i ? (int64_t)(p - s.row.data()) : -1;
}
