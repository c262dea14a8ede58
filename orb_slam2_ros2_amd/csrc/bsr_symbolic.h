// bsr_symbolic.h -- the block structure of the reduced camera system S = Hpp - Hpl Hll^-1 Hpl^T as 6x6 block-CSR, built on the host once
// per call.  Host only: no HIP header, so tests/cpp/test_bsr_symbolic.cpp compiles it with the host compiler alone.
//
// Block (i, j) of free keyframes exists iff i == j or the two observe a common point.  Both triangles are stored, a row's columns
// ascend, the diagonal is always there.  The blocks with i >= j ("lower" blocks, in (i, j) order) carry the edge pairs (e1, e2),
// pose(e1) = i, pose(e2) = j, same point, in the order the host-driven local BA enumerates them: points ascending, then e1, then e2, each
// in the point's edge list order.  A pose that observes a point twice simply contributes all four pairs to its diagonal block.
// Memory is O(pairs + blocks): no nf x nf table.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

struct BsrSymbolic {
  int32_t nb = 0;                  // block rows = free keyframes
  std::vector<int32_t> row_off;    // [nb + 1]
  std::vector<int32_t> col;        // [nnzb]
  std::vector<int32_t> twin;       // [nnzb] index of block (col, row); a diagonal block is its own twin
  std::vector<int32_t> low;        // [n_low] the stored blocks with row >= col, ascending index
  std::vector<int32_t> low_row;    // [n_low] their rows
  std::vector<int32_t> pair_off;   // [n_low + 1]
  std::vector<int32_t> pairs;      // [2 * n_pairs] e1, e2
  int32_t nnzb() const { return (int32_t)col.size(); }
};

// slot[pose] = index among the free keyframes, -1 for a fixed one; pt_off / pt_edges = the point -> edges lists (edges ascending)
inline void bsr_symbolic(int32_t nf, int32_t n_points, const int32_t* pt_off, const int32_t* pt_edges, const int32_t* edge_pose,
                         const int32_t* slot, BsrSymbolic* s) {
  struct Key {
    int64_t blk;  // i * nf + j, i >= j
    int64_t seq;  // position in the enumeration (-1: the diagonal's own entry, no pair)
    int32_t e1, e2;
  };
  std::vector<Key> keys;
  for (int32_t i = 0; i < nf; ++i) keys.push_back({(int64_t)i * nf + i, -1, -1, -1});
  int64_t seq = 0;
  for (int32_t pt = 0; pt < n_points; ++pt)
    for (int32_t q1 = pt_off[pt]; q1 < pt_off[pt + 1]; ++q1) {
      const int32_t e1 = pt_edges[q1], i = slot[edge_pose[e1]];
      if (i < 0) continue;
      for (int32_t q2 = pt_off[pt]; q2 < pt_off[pt + 1]; ++q2) {
        const int32_t e2 = pt_edges[q2], j = slot[edge_pose[e2]];
        if (j >= 0 && i >= j) keys.push_back({(int64_t)i * nf + j, seq++, e1, e2});
      }
    }
  std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.blk != b.blk ? a.blk < b.blk : a.seq < b.seq; });
  // the lower blocks and their pair lists
  std::vector<std::pair<int32_t, int32_t>> lower;  // (i, j)
  s->pair_off.clear(), s->pairs.clear();
  for (size_t k = 0; k < keys.size(); ++k) {
    if (k == 0 || keys[k].blk != keys[k - 1].blk) {
      lower.push_back({(int32_t)(keys[k].blk / nf), (int32_t)(keys[k].blk % nf)});
      s->pair_off.push_back((int32_t)(s->pairs.size() / 2));
    }
    if (keys[k].seq >= 0) s->pairs.push_back(keys[k].e1), s->pairs.push_back(keys[k].e2);
  }
  s->pair_off.push_back((int32_t)(s->pairs.size() / 2));
  // both triangles, rows in order, columns ascending: count, then place (the lower blocks arrive sorted by (i, j), so row r receives its
  // columns below the diagonal in ascending order first and the ones above it -- the transposes, sorted by (column = i) -- afterwards)
  s->nb = nf;
  s->row_off.assign((size_t)nf + 1, 0);
  for (const auto& b : lower) {
    ++s->row_off[b.first + 1];
    if (b.first != b.second) ++s->row_off[b.second + 1];
  }
  for (int32_t i = 0; i < nf; ++i) s->row_off[i + 1] += s->row_off[i];
  const size_t nnz = (size_t)s->row_off[nf];
  s->col.assign(nnz, 0), s->twin.assign(nnz, 0);
  s->low.assign(lower.size(), 0), s->low_row.assign(lower.size(), 0);
  std::vector<int32_t> cur(s->row_off.begin(), s->row_off.end() - 1);
  for (size_t l = 0; l < lower.size(); ++l) {  // j <= i entries of row i: ascending j within the row
    const int32_t i = lower[l].first, j = lower[l].second;
    s->low[l] = cur[i], s->low_row[l] = i;
    s->col[cur[i]++] = j;
  }
  // the transposes (j, i), j < i: lower is sorted by i first, so every row j receives its columns i > j ascending
  for (size_t l = 0; l < lower.size(); ++l) {
    const int32_t i = lower[l].first, j = lower[l].second;
    if (i == j) {
      s->twin[s->low[l]] = s->low[l];
      continue;
    }
    const int32_t q = cur[j]++;
    s->col[q] = i;
    s->twin[q] = s->low[l], s->twin[s->low[l]] = q;
  }
}
