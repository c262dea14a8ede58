// orbfe_posegraph.hip -- host side of orbfe_pose_graph_optimize and orbfe_debug_pose_graph_edges (include/orbfe.h): the graph checked,
// the incidence lists of the block assembly built, one upload, g2o's Levenberg-Marquardt control on the host with a few scalars down per
// trial (as the local bundle adjustment's host loop, orbfe_ba.hip), one download.  The kernels: k_posegraph.hip; the linear solver:
// launch_lba_chol (k_lba.hip), dense, or the block-sparse Cholesky over the essential graph's own structure (pg_symbolic.h,
// k_pgsparse.hip) behind orbfe_pose_graph_optimize_ex; the edge model: posegraph_edge_dev.h.  Rules G1 .. G9 of DESIGN 4.24, F1 .. F6 of
// 4.26.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <new>

#include "lm_host.h"
#include "orbfe_ctx.h"
#include "pg_symbolic.h"
#include "posegraph_edge_dev.h"

namespace {

// what both entry points refuse (ORBFE_EBADARG): NULL arrays with a count, indices out of range, self edges, entries that are not finite,
// a scale other than 1
orbfe_status pg_check(orbfe_ctx* c, const char* who, const orbfe_pose_graph* g) {
  if (!c || !g) return fail(c, ORBFE_EBADARG, "%s: NULL argument", who);
  const int NV = g->n_vertices, NE = g->n_edges;
  if (NV < 0 || NE < 0) return fail(c, ORBFE_EBADARG, "%s: negative count (%d vertices, %d edges)", who, NV, NE);
  if ((NV && (!g->estimates || !g->fixed)) || (NE && (!g->edge_v0 || !g->edge_v1 || !g->meas)))
    return fail(c, ORBFE_EBADARG, "%s: NULL array", who);
  auto sim3_ok = [](const double* p) {
    for (int k = 0; k < 8; ++k)
      if (!std::isfinite(p[k])) return false;
    return p[7] == 1.0;
  };
  for (int v = 0; v < NV; ++v)
    if (!sim3_ok(g->estimates + (size_t)v * 8))
      return fail(c, ORBFE_EBADARG, "%s: estimate %d is not finite or its scale is not 1 (fixed scale only)", who, v);
  for (int e = 0; e < NE; ++e) {
    const int a = g->edge_v0[e], b = g->edge_v1[e];
    if (a < 0 || a >= NV || b < 0 || b >= NV || a == b) return fail(c, ORBFE_EBADARG, "%s: edge %d joins vertices %d and %d of %d", who, e, a, b, NV);
    if (!sim3_ok(g->meas + (size_t)e * 8))
      return fail(c, ORBFE_EBADARG, "%s: measurement %d is not finite or its scale is not 1 (fixed scale only)", who, e);
  }
  return ORBFE_OK;
}

// the arrays of the graph in one upload region
struct GraphArrays {
  size_t o_est, o_fix, o_v0, o_v1, o_meas;
  void take(ScratchLayout& L, size_t NV, size_t NE) {
    o_est = L.take<double>(NV * 8), o_fix = L.take(NV), o_v0 = L.take<int32_t>(NE), o_v1 = L.take<int32_t>(NE), o_meas = L.take<double>(NE * 8);
  }
  void put(StagedIo& io, const orbfe_pose_graph* g, size_t NV, size_t NE) const {
    io.put(o_est, g->estimates, NV * 64);
    io.put(o_fix, g->fixed, NV);
    io.put(o_v0, g->edge_v0, NE * 4);
    io.put(o_v1, g->edge_v1, NE * 4);
    io.put(o_meas, g->meas, NE * 64);
  }
};

// ORBFE_PG_PHASES=1: the stream is synchronised after every phase of the loop and the wall time of each is added up (build | assemble |
// solve | evaluate, milliseconds, of the last call): what orbfe_debug_pose_graph_phases returns.  Off, nothing is synchronised or timed.
double g_pg_phase_ms[4] = {0, 0, 0, 0};
struct PhaseClock {
  bool on;
  hipStream_t st;
  std::chrono::steady_clock::time_point t0;
  PhaseClock(hipStream_t s) : on(std::getenv("ORBFE_PG_PHASES") != nullptr), st(s) {
    if (on) {
      for (double& v : g_pg_phase_ms) v = 0;
      (void)hipStreamSynchronize(st);
      t0 = std::chrono::steady_clock::now();
    }
  }
  void lap(int phase) {
    if (!on) return;
    (void)hipStreamSynchronize(st);
    const auto t1 = std::chrono::steady_clock::now();
    g_pg_phase_ms[phase] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

// k_pg_build's waves per workgroup: launch geometry only (an edge's wave computes the same whichever workgroup holds it)
int pg_waves() {
  const char* s = std::getenv("ORBFE_PG_WAVES");
  const int w = s ? std::atoi(s) : pg_max_waves();
  return std::min(std::max(w, 1), pg_max_waves());
}

// the structure of L as the device takes it, and the auto rule of orbfe_pose_graph_optimize_ex.  Block rows, joined pairs (i > j, each
// once) -> sym; ORBFE_ENOMEM where the structure does not fit the host or 32-bit block indices.
orbfe_status pg_structure(orbfe_ctx* c, const char* who, int nb, const std::vector<int32_t>& pi, const std::vector<int32_t>& pj, PgSymbolic* sym,
                          std::vector<int32_t>* col_off) {
  try {
    pg_symbolic(nb, pi.size(), pi.data(), pj.data(), sym);
    if (sym->l_blocks() > std::numeric_limits<int32_t>::max() / 2) throw std::bad_alloc();
    col_off->assign(sym->col_off.begin(), sym->col_off.end());
  } catch (const std::bad_alloc&) {
    return fail(c, ORBFE_ENOMEM, "%s: the factor's structure of %d block rows does not fit", who, nb);
  }
  return ORBFE_OK;
}

// solver 0: sparse past the dense solver's bound; below it from ORBFE_PG_SPARSE_MIN_FREE block rows on, unless the factor has more than
// ORBFE_PG_SPARSE_MAX_COL_BLOCKS blocks a column on average (the measured crossovers, DESIGN 4.26: the single workgroup's rank-6
// updates grow with the square of a column's length, and where they outgrow the dense solver's many workgroups is a column length, 24
// to 43 blocks from 100 to 1000 block rows, not a fraction of the dense triangle -- that fraction moves from 49 % to 9 % meanwhile)
bool pg_auto_sparse(int nf, int64_t l_blocks) {
  if (nf > ORBFE_PG_MAX_FREE) return true;
  if (nf < ORBFE_PG_SPARSE_MIN_FREE) return false;
  return l_blocks <= (int64_t)ORBFE_PG_SPARSE_MAX_COL_BLOCKS * nf;
}

// both entry points.  solver: 0 auto, 1 dense, 2 sparse; n_stats: 2 (orbfe_pose_graph_optimize) or 4
orbfe_status pg_optimize(orbfe_ctx* c, const char* who, const orbfe_pose_graph* g, int32_t iterations, int32_t solver, double* estimates_out,
                         double* chi2_out, int32_t* stats, int n_stats) {
  TRY(pg_check(c, who, g));
  if (iterations < 0) return fail(c, ORBFE_EBADARG, "%s: %d iterations", who, iterations);
  if (solver < 0 || solver > 2) return fail(c, ORBFE_EBADARG, "%s: solver %d (0 auto, 1 dense, 2 sparse)", who, solver);
  const int NV = g->n_vertices, NE = g->n_edges;
  if (NV && !estimates_out) return fail(c, ORBFE_EBADARG, "%s: NULL estimates_out", who);
  // slots of the non-fixed vertices: the block rows of the system, in vertex order
  std::vector<int32_t> slot((size_t)NV, -1);
  int nf = 0;
  for (int v = 0; v < NV; ++v)
    if (!g->fixed[v]) slot[(size_t)v] = nf++;
  if (solver == 1 && nf > ORBFE_PG_MAX_FREE)
    return fail(c, ORBFE_EBADSIZE, "%s: %d non-fixed vertices, at most %d (a dense system of 6 x that many rows)", who, nf, ORBFE_PG_MAX_FREE);
  auto put_stats = [&](int32_t its, int32_t trials, int32_t used, int64_t l_blocks) {
    if (!stats) return;
    stats[0] = its, stats[1] = trials;
    if (n_stats == 4) stats[2] = used, stats[3] = (int32_t)std::min<int64_t>(l_blocks, std::numeric_limits<int32_t>::max());
  };
  if (NE == 0 || iterations == 0 || nf == 0) {
    put_stats(0, 0, solver, 0);
    if (NV && estimates_out != g->estimates) std::memcpy(estimates_out, g->estimates, (size_t)NV * 64);
    return ORBFE_OK;
  }
  // the incidence lists (G6): block k < nf is the diagonal block of slot k; one more block per joined pair of slots (i > j); every
  // list in ascending edge index.  Entry = 4 * edge + code (k_pg_assemble).
  struct Off {
    int64_t key;
    int32_t ent;
  };
  std::vector<std::vector<int32_t>> diag((size_t)nf);
  std::vector<Off> off;
  for (int e = 0; e < NE; ++e) {
    const int s0 = slot[(size_t)g->edge_v0[e]], s1 = slot[(size_t)g->edge_v1[e]];
    if (s0 >= 0) diag[(size_t)s0].push_back(4 * e);
    if (s1 >= 0) diag[(size_t)s1].push_back(4 * e + 1);
    if (s0 >= 0 && s1 >= 0) off.push_back({(int64_t)std::max(s0, s1) * nf + std::min(s0, s1), 4 * e + (s0 > s1 ? 2 : 3)});
  }
  std::stable_sort(off.begin(), off.end(), [](const Off& a, const Off& b) { return a.key < b.key; });
  std::vector<int2> blk;
  std::vector<int32_t> blk_off, ent;
  for (int k = 0; k < nf; ++k) {
    blk.push_back(make_int2(k, k));
    blk_off.push_back((int32_t)ent.size());
    ent.insert(ent.end(), diag[(size_t)k].begin(), diag[(size_t)k].end());
  }
  for (size_t q = 0; q < off.size(); ++q) {
    if (q == 0 || off[q].key != off[q - 1].key) {
      blk.push_back(make_int2((int)(off[q].key / nf), (int)(off[q].key % nf)));
      blk_off.push_back((int32_t)ent.size());
    }
    ent.push_back(off[q].ent);
  }
  blk_off.push_back((int32_t)ent.size());
  const int n_blocks = (int)blk.size();
  // the sparse solver's structure: the factor's columns and the place of every block of Hpp in them
  PgSymbolic sym;
  std::vector<int32_t> col_off(1, 0), pos(1, 0);
  if (solver != 1) {
    std::vector<int32_t> pi, pj;
    for (int k = nf; k < n_blocks; ++k) pi.push_back(blk[(size_t)k].x), pj.push_back(blk[(size_t)k].y);
    TRY(pg_structure(c, who, nf, pi, pj, &sym, &col_off));
    if (solver == 0) solver = pg_auto_sparse(nf, sym.l_blocks()) ? 2 : 1;
  }
  const bool sparse = solver == 2;
  if (sparse) {
    pos.resize((size_t)n_blocks);
    for (int k = 0; k < n_blocks; ++k) pos[(size_t)k] = (int32_t)pg_symbolic_pos(sym, blk[(size_t)k].x, blk[(size_t)k].y);
  } else {
    sym.row.clear(), col_off.assign(1, 0);  // (auto took the dense solver: nothing of the structure goes up)
  }
  const size_t l_doubles = sparse ? (size_t)sym.l_blocks() * 36 : 0;

  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t NVs = (size_t)NV, NEs = (size_t)NE, n = (size_t)6 * nf;
  ScratchLayout L;
  ScratchRegion up, down;
  GraphArrays A;
  L.open(up);
  A.take(L, NVs, NEs);
  const size_t o_slot = L.take<int32_t>(NVs), o_blk = L.take<int2>(blk.size()), o_boff = L.take<int32_t>(blk_off.size()),
               o_ent = L.take<int32_t>(ent.size()), o_coff = L.take<int32_t>(col_off.size()), o_row = L.take<int32_t>(sym.row.size() + 1),
               o_pos = L.take<int32_t>(pos.size()), o_out = L.close(up).open(down).take<double>(NVs * 8), o_chi = L.take<double>(NEs),
               o_trial = L.close(down).take<double>(NVs * 8), o_hee = L.take<double>(NEs * 108), o_be = L.take<double>(NEs * 12),
               o_err = L.take<double>(NEs * 6), o_chi_t = L.take<double>(NEs), o_s = L.take<double>(sparse ? l_doubles : n * n), o_rhs = L.take<double>(n),
               o_x = L.take<double>(n), o_sc = L.take<double>(5),
               o_big = L.take(!sparse && nf > LBA_MAX_FREE ? ((n + 1) * 6 + (size_t)nf * 36 + n) * 8 : 8);  // launch_lba_chol's panel in global memory
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes())));
  A.put(io, g, NVs, NEs);
  io.put(o_slot, slot.data(), NVs * 4);
  io.put(o_blk, blk.data(), blk.size() * 8);
  io.put(o_boff, blk_off.data(), blk_off.size() * 4);
  io.put(o_ent, ent.data(), ent.size() * 4);
  io.put(o_coff, col_off.data(), col_off.size() * 4);
  io.put(o_row, sym.row.data(), sym.row.size() * 4);
  io.put(o_pos, pos.data(), pos.size() * 4);
  HIP_TRY(c, io.upload(up));
  hipStream_t st = c->stream;
  const int waves = pg_waves();
  // the current estimates and the trial's alternate between two buffers: accepting a trial is a swap, rejecting it nothing
  double* d_est[2] = {io.dev<double>(A.o_est), io.dev<double>(o_trial)};
  int cur = 0;
  const uint8_t* d_fix = io.dev<uint8_t>(A.o_fix);
  const int32_t *d_v0 = io.dev<int32_t>(A.o_v0), *d_v1 = io.dev<int32_t>(A.o_v1), *d_boff = io.dev<int32_t>(o_boff), *d_ent = io.dev<int32_t>(o_ent);
  const double* d_meas = io.dev<double>(A.o_meas);
  double *d_hee = io.dev<double>(o_hee), *d_be = io.dev<double>(o_be), *d_s = io.dev<double>(o_s), *d_rhs = io.dev<double>(o_rhs),
         *d_x = io.dev<double>(o_x), *d_chi_t = io.dev<double>(o_chi_t);
  double* d_sc = io.dev<double>(o_sc);  // the loop's five scalars (lm_host.h)
  int32_t done = 0, trials = 0;
  {
    StageTimer tm(c, ORBFE_STAGE_BA, st);
    // SparseOptimizer::optimize(iterations) + OptimizationAlgorithmLevenberg::solve (G7): lm_host.h
    PhaseClock clk(st);
    auto linearize = [&](int it) -> orbfe_status {
      // computeActiveErrors + linearizeOplus + constructQuadraticForm of every edge at the current estimates
      launch_pg_build(st, NE, waves, d_est[cur], d_fix, d_v0, d_v1, d_meas, d_hee, d_be, io.dev<double>(o_err), d_chi_t, nullptr);
      launch_pg_reduce(st, NE, d_chi_t, 0, d_x, d_rhs, d_sc + 2, d_sc);
      if (it == 0) launch_pg_maxdiag(st, nf, d_boff, d_ent, d_hee, d_sc + 1);
      HIP_TRY(c, hipGetLastError());
      return ORBFE_OK;
    };
    auto trial = [&](double lambda, bool&) -> orbfe_status {
      HIP_TRY(c, lm_host_upload(st, d_sc, lambda));
      // (the factorisation works in place: the system is assembled for every trial)
      HIP_TRY(c, hipMemsetAsync(d_s, 0, (sparse ? l_doubles : n * n) * 8, st));
      if (sparse) {
        launch_pgs_assemble(st, n_blocks, io.dev<int2>(o_blk), d_boff, d_ent, io.dev<int32_t>(o_pos), d_hee, d_be, d_sc + 2, d_s, d_rhs);
        clk.lap(1);
        launch_pgs_solve(st, nf, io.dev<int32_t>(o_coff), io.dev<int32_t>(o_row), sym.search_steps, d_s, d_rhs, d_x, (int*)(d_sc + 3));
      } else {
        launch_pg_assemble(st, nf, n_blocks, io.dev<int2>(o_blk), d_boff, d_ent, d_hee, d_be, d_sc + 2, d_s, d_rhs);
        clk.lap(1);
        launch_lba_chol(st, nf, d_s, d_rhs, d_x, (int*)(d_sc + 3), io.dev<double>(o_big));
      }
      clk.lap(2);
      launch_pg_update(st, NV, io.dev<int32_t>(o_slot), d_x, d_est[cur], d_est[cur ^ 1]);
      launch_pg_chi2(st, NE, d_est[cur ^ 1], d_v0, d_v1, d_meas, d_chi_t);
      launch_pg_reduce(st, NE, d_chi_t, (int)n, d_x, d_rhs, d_sc + 2, d_sc);
      HIP_TRY(c, hipGetLastError());
      return ORBFE_OK;
    };
    auto on_accept = [&]() -> orbfe_status {
      cur ^= 1;  // the trial estimates are the current ones
      return ORBFE_OK;
    };
    auto on_reject = [&](bool) -> orbfe_status { return ORBFE_OK; };
    TRY(lm_host_optimize(c, st, d_sc, iterations, nullptr, done, trials, linearize, trial, on_accept, on_reject, [&](int phase) { clk.lap(phase); }));
    // the results: the current estimates and the chi2 of every edge at them
    HIP_TRY(c, hipMemcpyAsync(io.dev<double>(o_out), d_est[cur], NVs * 64, hipMemcpyDeviceToDevice, st));
    launch_pg_chi2(st, NE, d_est[cur], d_v0, d_v1, d_meas, io.dev<double>(o_chi));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down));
  drain_timers(c);
  io.get(estimates_out, o_out, NVs * 64);
  io.get(chi2_out, o_chi, NEs * 8);
  put_stats(done, trials, solver, sparse ? sym.l_blocks() : 0);
  return ORBFE_OK;
}

}  // namespace

extern "C" {

orbfe_status orbfe_pose_graph_optimize(orbfe_ctx* c, const orbfe_pose_graph* g, int32_t iterations, double* estimates_out, double* chi2_out,
                                       int32_t* stats) {
  ApiLock api_lk(c);
  return pg_optimize(c, "pose_graph_optimize", g, iterations, 1, estimates_out, chi2_out, stats, 2);
}

orbfe_status orbfe_pose_graph_optimize_ex(orbfe_ctx* c, const orbfe_pose_graph* g, int32_t iterations, const orbfe_pose_graph_options* opt,
                                          double* estimates_out, double* chi2_out, int32_t* stats) {
  ApiLock api_lk(c);
  return pg_optimize(c, "pose_graph_optimize_ex", g, iterations, opt ? opt->solver : 0, estimates_out, chi2_out, stats, 4);
}

// One block-sparse system through pg_symbolic and k_pgs_solve, in the layout orbfe_pose_graph_optimize_ex gives them: the lower blocks at
// their places in L's storage, everything else zero.
orbfe_status orbfe_debug_pg_sparse_solve(orbfe_ctx* c, int32_t nb, int32_t n_low, const int32_t* low_row, const int32_t* low_col, const double* blocks,
                                         const double* rhs, double* x, int32_t* ok, int64_t* l_blocks) {
  ApiLock api_lk(c);
  if (!c || !low_row || !low_col || !blocks || !rhs || !x || !ok) return fail(c, ORBFE_EBADARG, "debug_pg_sparse_solve: NULL argument");
  if (nb < 1 || n_low < 0 || nb > std::numeric_limits<int32_t>::max() / 6)
    return fail(c, ORBFE_EBADARG, "debug_pg_sparse_solve: %d block rows, %d blocks", nb, n_low);
  std::vector<int32_t> pi, pj;
  for (int q = 0; q < n_low; ++q) {
    if (low_col[q] < 0 || low_row[q] < low_col[q] || low_row[q] >= nb)
      return fail(c, ORBFE_EBADARG, "debug_pg_sparse_solve: block %d is (%d, %d) of %d block rows (lower blocks only)", q, low_row[q], low_col[q], nb);
    if (low_row[q] != low_col[q]) pi.push_back(low_row[q]), pj.push_back(low_col[q]);
  }
  PgSymbolic sym;
  std::vector<int32_t> col_off;
  TRY(pg_structure(c, "debug_pg_sparse_solve", nb, pi, pj, &sym, &col_off));
  const size_t l_doubles = (size_t)sym.l_blocks() * 36, n = (size_t)6 * nb;
  std::vector<double> lv;
  std::vector<uint8_t> seen;
  try {
    lv.assign(l_doubles, 0.0), seen.assign((size_t)sym.l_blocks(), 0);
  } catch (const std::bad_alloc&) {
    return fail(c, ORBFE_ENOMEM, "debug_pg_sparse_solve: a factor of %lld blocks does not fit", (long long)sym.l_blocks());
  }
  for (int q = 0; q < n_low; ++q) {
    const size_t p = (size_t)pg_symbolic_pos(sym, low_row[q], low_col[q]);
    if (seen[p]) return fail(c, ORBFE_EBADARG, "debug_pg_sparse_solve: block (%d, %d) is given twice", low_row[q], low_col[q]);
    seen[p] = 1;
    std::memcpy(lv.data() + p * 36, blocks + (size_t)q * 36, 288);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  ScratchLayout L;
  ScratchRegion up, down;
  const size_t o_lv = L.open(up).take<double>(l_doubles), o_rhs = L.take<double>(n), o_coff = L.take<int32_t>(col_off.size()),
               o_row = L.take<int32_t>(sym.row.size()), o_ok = L.open(down).take<int32_t>(1), o_x = L.close(up).take<double>(n);
  L.close(down);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes()), up.end + down.bytes() <= ((size_t)16 << 20)));
  const int32_t ok_init = 1;
  int32_t ok_fin = 0;
  io.put(o_lv, lv.data(), l_doubles * 8);
  io.put(o_rhs, rhs, n * 8);
  io.put(o_coff, col_off.data(), col_off.size() * 4);
  io.put(o_row, sym.row.data(), sym.row.size() * 4);
  io.put(o_ok, &ok_init, 4);
  HIP_TRY(c, io.upload(up));
  launch_pgs_solve(c->stream, nb, io.dev<int32_t>(o_coff), io.dev<int32_t>(o_row), sym.search_steps, io.dev<double>(o_lv), io.dev<double>(o_rhs),
                   io.dev<double>(o_x), io.dev<int>(o_ok));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.download(down));
  if (io.staged) HIP_TRY(c, io.wait());
  io.get(&ok_fin, o_ok, 4);
  io.get(x, o_x, n * 8);
  if (!io.staged) HIP_TRY(c, io.wait());
  *ok = ok_fin;
  if (l_blocks) *l_blocks = sym.l_blocks();
  return ORBFE_OK;
}

orbfe_status orbfe_debug_pose_graph_phases(double* ms) {
  if (!ms) return ORBFE_EBADARG;
  for (int k = 0; k < 4; ++k) ms[k] = g_pg_phase_ms[k];
  return ORBFE_OK;
}

orbfe_status orbfe_debug_pose_graph_edges(orbfe_ctx* c, const orbfe_pose_graph* g, double* err, double* chi2, double* jac) {
  ApiLock api_lk(c);
  TRY(pg_check(c, "debug_pose_graph_edges", g));
  const int NE = g->n_edges;
  if (NE == 0) return ORBFE_OK;
  if (!err || !chi2 || !jac) return fail(c, ORBFE_EBADARG, "debug_pose_graph_edges: NULL output");
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t NVs = (size_t)g->n_vertices, NEs = (size_t)NE;
  ScratchLayout L;
  ScratchRegion up, down;
  GraphArrays A;
  L.open(up);
  A.take(L, NVs, NEs);
  const size_t o_err = L.close(up).open(down).take<double>(NEs * 6), o_chi = L.take<double>(NEs), o_jac = L.take<double>(NEs * 72),
               o_hee = L.close(down).take<double>(NEs * 108), o_be = L.take<double>(NEs * 12);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes())));
  A.put(io, g, NVs, NEs);
  HIP_TRY(c, io.upload(up));
  launch_pg_build(c->stream, NE, pg_waves(), io.dev<double>(A.o_est), io.dev<uint8_t>(A.o_fix), io.dev<int32_t>(A.o_v0), io.dev<int32_t>(A.o_v1),
                  io.dev<double>(A.o_meas), io.dev<double>(o_hee), io.dev<double>(o_be), io.dev<double>(o_err), io.dev<double>(o_chi),
                  io.dev<double>(o_jac));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down));
  io.get(err, o_err, NEs * 48);
  io.get(chi2, o_chi, NEs * 8);
  io.get(jac, o_jac, NEs * 576);
  return ORBFE_OK;
}

}  // extern "C"
