// orbfe_gba.hip -- the global bundle adjustment (Optimizer::globalOptimization, Optimizer.cc:934-1043, from the point where the graph is
// built): one optimize(n) of the local BA's graph type with the reduced camera system as 6x6 block-CSR and a block-Jacobi preconditioned
// conjugate gradient in place of the dense Cholesky (k_bsr.hip).  The Levenberg control is the host-driven loop of the local BA
// (orbfe_ba.hip, host_lm) with its builders, update and sums; only the solver step differs.
#include "ba_host.h"
#include "lm_host.h"
#include "bsr_symbolic.h"
namespace {

// ORBFE_GBA_PHASES=1: the stream is synchronised after every phase and the wall time of each is added up (build | Schur | PCG | evaluate,
// milliseconds, of the last call; [4] = launches and copies enqueued): what orbfe_debug_ba_global_phases returns.
double g_gba_phase_ms[5] = {0, 0, 0, 0, 0};
struct GbaClock {
  bool on;
  hipStream_t st;
  std::chrono::steady_clock::time_point t0;
  GbaClock(hipStream_t s) : on(std::getenv("ORBFE_GBA_PHASES") != nullptr), st(s) {
    if (on) {
      for (double& v : g_gba_phase_ms) v = 0;
      (void)hipStreamSynchronize(st);
      t0 = std::chrono::steady_clock::now();
    }
  }
  void lap(int phase, int launches) {
    if (!on) return;
    (void)hipStreamSynchronize(st);
    const auto t1 = std::chrono::steady_clock::now();
    g_gba_phase_ms[phase] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    g_gba_phase_ms[4] += launches;
    t0 = t1;
  }
};

// Iterations enqueued between two reads of {iterations, state}.  After convergence the rest of a chunk is three empty launches per
// iteration; a short chunk costs a synchronisation and a 56-byte download each.  DESIGN 4.25 has the measurement behind the default
// (ORBFE_PCG_CHUNK overrides it, for that measurement: read at every solve).
#define GBA_PCG_CHUNK 64
int pcg_chunk() {
  const char* e = std::getenv("ORBFE_PCG_CHUNK");
  const int n = e ? std::atoi(e) : 0;
  return n > 0 ? n : GBA_PCG_CHUNK;
}

struct PcgResult {
  int32_t iters = 0, state = PCG_RUNNING;
  bool ok() const { return state == PCG_CONVERGED; }
};
// the whole solve of the system P describes (Minv and *ok are in place): enqueue in chunks, read the verdict between them
orbfe_status run_pcg(orbfe_ctx* c, hipStream_t st, const BsrPcgLaunch& P, double tol, int max_iter, PcgResult* res, int* launches = nullptr) {
  launch_pcg_begin(st, P, tol);
  if (launches) *launches += 2;
  const int chunk = pcg_chunk();
  for (int k = 0;;) {
    const int n = std::min(chunk, max_iter - k);
    if (n > 0) launch_pcg_iterations(st, P, k, n), k += n;
    if (launches) *launches += 3 * std::max(n, 0) + 1;
    HIP_TRY(c, hipGetLastError());
    PcgState h;
    HIP_TRY(c, hipMemcpyAsync(&h, P.state, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    res->iters = h.iters, res->state = h.done;
    if (h.done != PCG_RUNNING || k >= max_iter) return ORBFE_OK;
  }
}

// the solver's vectors behind a system of nb block rows
struct PcgOffsets {
  size_t minv, x, r, z, p, q, part_pq, part_rz, state;
  void take(ScratchLayout& L, size_t nb) {
    minv = L.take<double>(nb * 36), x = L.take<double>(nb * 6), r = L.take<double>(nb * 6), z = L.take<double>(nb * 6), p = L.take<double>(nb * 6),
    q = L.take<double>(nb * 6), part_pq = L.take<double>(nb), part_rz = L.take<double>(nb), state = L.take(sizeof(PcgState));
  }
  void fill(BsrPcgLaunch& P, const StagedIo& io) const {
    P.Minv = io.dev<double>(minv), P.x = io.dev<double>(x), P.r = io.dev<double>(r), P.z = io.dev<double>(z), P.p = io.dev<double>(p),
    P.q = io.dev<double>(q), P.part_pq = io.dev<double>(part_pq), P.part_rz = io.dev<double>(part_rz), P.state = io.dev<PcgState>(state);
  }
};

// the block-CSR structure in the scratch
struct BsrOffsets {
  size_t row_off, col, twin, low, low_row, pair_off, pairs;
  void take(ScratchLayout& L, const BsrSymbolic& s) {
    row_off = L.take<int32_t>(s.row_off.size()), col = L.take<int32_t>(s.col.size()), twin = L.take<int32_t>(s.twin.size()),
    low = L.take<int32_t>(s.low.size()), low_row = L.take<int32_t>(s.low_row.size()), pair_off = L.take<int32_t>(s.pair_off.size()),
    pairs = L.take<int32_t>(s.pairs.size());
  }
  void put(StagedIo& io, const BsrSymbolic& s) const {
    io.put(row_off, s.row_off.data(), s.row_off.size() * 4), io.put(col, s.col.data(), s.col.size() * 4);
    io.put(twin, s.twin.data(), s.twin.size() * 4), io.put(low, s.low.data(), s.low.size() * 4);
    io.put(low_row, s.low_row.data(), s.low_row.size() * 4), io.put(pair_off, s.pair_off.data(), s.pair_off.size() * 4);
    io.put(pairs, s.pairs.data(), s.pairs.size() * 4);
  }
};

orbfe_status gba_check(orbfe_ctx* c, const char* who, const orbfe_ba_problem* p) {
  if (p->n_edges < 0 || p->n_poses < 0 || p->n_points < 0) return fail(c, ORBFE_EBADARG, "%s: negative size", who);
  if ((p->n_poses && !p->poses) || (p->n_points && !p->points) ||
      (p->n_edges && (!p->edge_pose || !p->edge_point || !p->meas || !p->is_stereo || !p->info || !p->huber_delta)))
    return fail(c, ORBFE_EBADARG, "%s: NULL array", who);
  return ba_check_problem(c, who, p);
}

// free keyframes in index order
void gba_slots(const orbfe_ba_problem* p, const uint8_t* pose_fixed, std::vector<int32_t>* slot, std::vector<int32_t>* free_pose) {
  slot->assign(p->n_poses, -1), free_pose->clear();
  for (int k = 0; k < p->n_poses; ++k)
    if (!(pose_fixed && pose_fixed[k])) {
      (*slot)[k] = (int32_t)free_pose->size();
      free_pose->push_back(k);
    }
}

// what launch_bsr_schur needs besides the system builder's record
struct SchurAt {
  const BsrSymbolic* sym;
  const BsrOffsets* so;
  size_t free_pose, hpp, bp, bl, hpl, w, lambda, blocks, rhs, minv, ok;
};
void gba_schur(hipStream_t st, const StagedIo& io, const BaInputs& in, const SchurAt& a) {
  launch_bsr_schur(st, (int)a.sym->low.size(), io.dev<int32_t>(a.so->low), io.dev<int32_t>(a.so->low_row), io.dev<int32_t>(a.so->col),
                   io.dev<int32_t>(a.so->twin), io.dev<int32_t>(a.so->pair_off), io.dev<int2>(a.so->pairs), io.dev<int32_t>(a.free_pose),
                   io.dev<int32_t>(in[BA_PSO]), io.dev<int32_t>(in[BA_PSE]), io.dev<int32_t>(in[BA_ET]), io.dev<double>(a.hpp), io.dev<double>(a.bp),
                   io.dev<double>(a.bl), io.dev<double>(a.hpl), io.dev<double>(a.w), io.dev<double>(a.lambda), io.dev<double>(a.blocks),
                   io.dev<double>(a.rhs), io.dev<double>(a.minv), io.dev<int>(a.ok));
}

orbfe_status gba_sparse(orbfe_ctx* c, const orbfe_ba_problem* p, const uint8_t* pose_fixed, int32_t iterations, const volatile uint8_t* stop_flag,
                        double tol, int32_t max_iter_opt, const orbfe_ba_global_out* o) {
  const int E = p->n_edges, NK = p->n_poses, NP = p->n_points;
  BaVertexLists v;
  ba_vertex_lists(p, &v);
  std::vector<int32_t> slot, free_pose;
  gba_slots(p, pose_fixed, &slot, &free_pose);
  const int nf = (int)free_pose.size();
  BsrSymbolic sym;
  bsr_symbolic(nf, NP, v.pt_off.data(), v.pt_edges.data(), p->edge_pose, slot.data(), &sym);
  const int max_iter = max_iter_opt > 0 ? max_iter_opt : (int)std::min<int64_t>((int64_t)24 * nf, std::numeric_limits<int32_t>::max());
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t n = (size_t)6 * nf, NE = (size_t)E, NKs = (size_t)NK, NPs = (size_t)NP, NZ = sym.col.size();
  ScratchLayout L;
  ScratchRegion up, zero;
  BaInputs in;
  BsrOffsets so;
  PcgOffsets po;
  ba_take(L.open(up), p, pose_fixed, &v, &in);
  const size_t o_free = L.take<int32_t>((size_t)nf), o_slot = L.take<int32_t>(NKs);
  so.take(L, sym);
  const size_t o_pose_bk = L.close(up).take<double>(NKs * 7), o_pt_bk = L.take<double>(NPs * 3), o_hpp = L.take<double>(NKs * 36),
               o_bp = L.take<double>(NKs * 6), o_hll = L.take<double>(NPs * 9), o_bl = L.take<double>(NPs * 3), o_hpl = L.take<double>(NE * 18),
               o_w = L.take<double>(NE * 18), o_blocks = L.take<double>(NZ * 36), o_rhs = L.take<double>(n), o_dxp = L.take<double>(NKs * 6),
               o_dxl = L.take<double>(NPs * 3), o_err = L.take<double>(NE * 3), o_chi2 = L.take<double>(NE), o_rho = L.take<double>(NE * 2),
               o_terms = L.take<double>(NE * 32), o_chipart = L.take<double>((NPs + 31) / 32);
  po.take(L, (size_t)nf);
  // zero: one block that starts as zeros (ONE fill): edge levels (all active) | chi2 of the last linearisation | point inverses | the
  // system builder's control state (buffer 0 current)
  const size_t o_level = L.open(zero).take(NE), o_last = L.take<double>(NE), o_dinv = L.take<double>(NPs * 9), o_lmstate = L.take(sizeof(LmState)),
               o_depth = L.close(zero).take(NE), o_sc = L.take<double>(5);
  StagedIo io;
  TRY(io.reserve(c, L.end(), up.end));
  uint8_t* b = io.d;
  hipStream_t st = c->stream;
  ba_put(io, in);
  io.put(o_free, free_pose.data(), (size_t)nf * 4);
  io.put(o_slot, slot.data(), NKs * 4);
  so.put(io, sym);
  HIP_TRY(c, io.upload(up));
  HIP_TRY(c, hipMemsetAsync(b + zero.begin, 0, zero.bytes(), st));

  const BaParamsDev prm = {p->fx, p->fy, p->cx, p->cy, p->bf};
  LmLaunch K{};
  lm_fill_inputs(K, io, in, p);
  lm_fill_one_system(K, io, {o_lmstate, o_level, in[BA_INFO], o_hpp, o_bp, o_hll, o_bl, o_hpl, o_terms, o_chipart});
  BsrPcgLaunch P{};
  P.nb = nf, P.row_off = io.dev<int32_t>(so.row_off), P.col = io.dev<int32_t>(so.col), P.blocks = io.dev<double>(o_blocks),
  P.rhs = io.dev<double>(o_rhs);
  po.fill(P, io);
  double* d_poses = io.dev<double>(in[BA_POSE]);
  double* d_points = io.dev<double>(in[BA_PT]);
  const int32_t* d_ek = io.dev<int32_t>(in[BA_EP]);
  const int32_t* d_ep = io.dev<int32_t>(in[BA_ET]);
  double* d_sc = io.dev<double>(o_sc);  // the loop's five scalars (lm_host.h)
  P.ok = (int*)(d_sc + 3);
  const SchurAt sa = {&sym, &so, o_free, o_hpp, o_bp, o_bl, o_hpl, o_w, o_sc + 16, o_blocks, o_rhs, po.minv, o_sc + 24};
  auto evaluate = [&]() {  // computeActiveErrors + activeRobustChi2 (no edge is ever excluded here: the information is the problem's)
    launch_ba_edges(st, E, d_poses, d_points, d_ek, d_ep, io.dev<double>(in[BA_MEAS]), io.dev<uint8_t>(in[BA_ST]), io.dev<double>(in[BA_INFO]),
                    io.dev<double>(in[BA_DELTA]), prm, io.dev<double>(o_err), io.dev<double>(o_chi2), io.dev<double>(o_rho), nullptr, nullptr,
                    io.dev<uint8_t>(o_depth));
    launch_lba_chi2_sum(st, E, io.dev<double>(o_chi2), io.dev<double>(o_rho), io.dev<uint8_t>(o_level), io.dev<double>(o_last), d_sc);
  };
  StageTimer tm(c, ORBFE_STAGE_BA, st);
  GbaClock clk(st);
  int64_t cg_iters = 0, rejected = 0;
  int32_t done = 0, trials = 0;
  // SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve (lm_host.h): the local BA's host loop with the solver step
  // exchanged and no classification round
  auto linearize = [&](int it) -> orbfe_status {
    evaluate();
    launch_lm_build(st, K, 0, 0, 0, true);
    if (it == 0) launch_lba_maxdiag(st, NK, NP, io.dev<double>(o_hpp), io.dev<double>(o_hll), io.dev<uint8_t>(in[BA_FIX]), d_sc + 1);
    return ORBFE_OK;
  };
  auto trial = [&](double lambda, bool& solver_ok) -> orbfe_status {
    HIP_TRY(c, hipMemcpyAsync(b + o_pose_bk, d_poses, NKs * 56, hipMemcpyDeviceToDevice, st));  // push()
    HIP_TRY(c, hipMemcpyAsync(b + o_pt_bk, d_points, NPs * 24, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, lm_host_upload(st, d_sc, lambda));
    launch_lba_pre(st, NP, E, d_ep, io.dev<double>(o_hll), io.dev<double>(o_hpl), d_sc + 2, io.dev<double>(o_dinv), io.dev<double>(o_w),
                   (int*)(d_sc + 3));
    gba_schur(st, io, in, sa);
    clk.lap(1, 6);
    PcgResult pr;
    pr.state = PCG_CONVERGED;  // (no free keyframe: nothing to solve)
    int launches = 0;
    if (nf > 0) TRY(run_pcg(c, st, P, tol, max_iter, &pr, &launches));
    clk.lap(2, launches);
    cg_iters += pr.iters;
    solver_ok = pr.ok();
    launch_lba_post(st, NK, NP, io.dev<int32_t>(o_slot), io.dev<int32_t>(in[BA_PTO]), io.dev<int32_t>(in[BA_PTE]), d_ek, io.dev<uint8_t>(in[BA_FIX]),
                    io.dev<double>(o_bp), io.dev<double>(o_bl), io.dev<double>(o_hpl), d_sc + 2, io.dev<double>(o_dinv), P.x, d_poses, d_points,
                    io.dev<double>(o_dxp), io.dev<double>(o_dxl), d_sc + 4);
    evaluate();
    return ORBFE_OK;
  };
  auto on_accept = [&]() -> orbfe_status {
    clk.lap(3, 7);
    return ORBFE_OK;
  };
  auto on_reject = [&](bool ok) -> orbfe_status {
    if (!ok) ++rejected;
    HIP_TRY(c, hipMemcpyAsync(d_poses, b + o_pose_bk, NKs * 56, hipMemcpyDeviceToDevice, st));  // pop()
    HIP_TRY(c, hipMemcpyAsync(d_points, b + o_pt_bk, NPs * 24, hipMemcpyDeviceToDevice, st));
    clk.lap(3, 7);
    return ORBFE_OK;
  };
  TRY(lm_host_optimize(c, st, d_sc, iterations, stop_flag, done, trials, linearize, trial, on_accept, on_reject, [&](int phase) {
    if (phase == 0) clk.lap(0, 6);  // (a trial's clock stops behind its pop copies: on_accept / on_reject)
  }));
  // computeError() on every edge with the final estimates (Optimizer.cc:1000-1043 reads the vertices only; chi2 is this call's extra)
  launch_ba_edges(st, E, d_poses, d_points, d_ek, d_ep, io.dev<double>(in[BA_MEAS]), io.dev<uint8_t>(in[BA_ST]), io.dev<double>(in[BA_INFO]),
                  io.dev<double>(in[BA_DELTA]), prm, io.dev<double>(o_err), io.dev<double>(o_chi2), io.dev<double>(o_rho), nullptr, nullptr,
                  io.dev<uint8_t>(o_depth));
  HIP_TRY(c, hipGetLastError());
  io.staged = false;  // the results go straight from the scratch to the caller's arrays
  io.get(o->poses, in[BA_POSE], NKs * 56);
  io.get(o->points, in[BA_PT], NPs * 24);
  io.get(o->chi2, o_chi2, NE * 8);
  HIP_TRY(c, io.wait());
  clk.lap(3, 4);
  if (o->iterations) o->iterations[0] = done;
  if (o->cg_stats) o->cg_stats[0] = trials, o->cg_stats[1] = cg_iters, o->cg_stats[2] = rejected;
  return ORBFE_OK;
}

}  // namespace

extern "C" {

orbfe_status orbfe_ba_global_optimize(orbfe_ctx* c, const orbfe_ba_problem* p, const uint8_t* pose_fixed, int32_t iterations,
                                      const volatile uint8_t* stop_flag, const orbfe_ba_global_options* opt, const orbfe_ba_global_out* o) {
  if (!c || !p || !o) return fail(c, ORBFE_EBADARG, "ba_global_optimize: NULL argument");
  const int32_t solver = opt ? opt->solver : 0;
  if (solver < 0 || solver > 2) return fail(c, ORBFE_EBADARG, "ba_global_optimize: solver %d (0 auto, 1 dense, 2 block-sparse PCG)", solver);
  if (iterations < 0) return fail(c, ORBFE_EBADARG, "ba_global_optimize: negative size");
  if (!o->poses || !o->points) return fail(c, ORBFE_EBADARG, "ba_global_optimize: NULL output");
  {
    ApiLock api_lk(c);
    TRY(gba_check(c, "ba_global_optimize", p));
  }
  int nf = 0;
  for (int k = 0; k < p->n_poses; ++k) nf += !(pose_fixed && pose_fixed[k]);
  if (o->cg_stats) o->cg_stats[0] = o->cg_stats[1] = o->cg_stats[2] = 0;
  if (p->n_edges == 0) {  // nothing to optimise: the inputs
    if (o->poses != p->poses && p->n_poses) std::memcpy(o->poses, p->poses, (size_t)p->n_poses * 56);
    if (o->points != p->points && p->n_points) std::memcpy(o->points, p->points, (size_t)p->n_points * 24);
    if (o->iterations) o->iterations[0] = 0;
    return ORBFE_OK;
  }
  if (solver == 1 || (solver == 0 && nf <= ORBFE_GBA_DENSE_MAX_FREE)) {
    // the local BA's first optimize() is this optimisation; its second, of zero iterations, changes no estimate
    int32_t its[2] = {0, 0};
    const orbfe_ba_optimize_out lo = {o->poses, o->points, nullptr, o->chi2, nullptr, its};
    TRY(orbfe_ba_local_optimize(c, p, pose_fixed, iterations, 0, stop_flag, &lo));
    if (o->iterations) o->iterations[0] = its[0];
    return ORBFE_OK;
  }
  ApiLock api_lk(c);
  const double tol = opt && opt->pcg_tol > 0 ? opt->pcg_tol : 1e-10;
  return gba_sparse(c, p, pose_fixed, iterations, stop_flag, tol, opt ? opt->pcg_max_iter : 0, o);
}

orbfe_status orbfe_debug_ba_reduced_bsr(orbfe_ctx* c, const orbfe_ba_problem* p, const uint8_t* pose_fixed, double lambda, int32_t cap_blocks,
                                        int32_t* nnzb, int32_t* row_off, int32_t* col, double* blocks, double* rhs) {
  ApiLock api_lk(c);
  if (!c || !p || !nnzb || !row_off) return fail(c, ORBFE_EBADARG, "debug_ba_reduced_bsr: NULL argument");
  TRY(gba_check(c, "debug_ba_reduced_bsr", p));
  BaVertexLists v;
  ba_vertex_lists(p, &v);
  std::vector<int32_t> slot, free_pose;
  gba_slots(p, pose_fixed, &slot, &free_pose);
  const int nf = (int)free_pose.size();
  BsrSymbolic sym;
  bsr_symbolic(nf, p->n_points, v.pt_off.data(), v.pt_edges.data(), p->edge_pose, slot.data(), &sym);
  *nnzb = sym.nnzb();
  std::memcpy(row_off, sym.row_off.data(), sym.row_off.size() * 4);
  if (cap_blocks < sym.nnzb()) return ORBFE_OK;
  if (nf == 0) return ORBFE_OK;
  if (!col || !blocks || !rhs) return fail(c, ORBFE_EBADARG, "debug_ba_reduced_bsr: NULL output");
  std::memcpy(col, sym.col.data(), sym.col.size() * 4);
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t E = (size_t)p->n_edges, NK = (size_t)p->n_poses, NP = (size_t)p->n_points, NZ = sym.col.size(), n = (size_t)6 * nf;
  ScratchLayout L;
  ScratchRegion up, zero, out;
  BaInputs in;
  BsrOffsets so;
  ba_take(L.open(up), p, pose_fixed, &v, &in);
  const size_t o_free = L.take<int32_t>((size_t)nf);
  so.take(L, sym);
  // the tail of the upload: lambda | ok | control state (buffer 0 current) and edge levels (all active), zeros
  const size_t o_lambda = L.take(8), o_ok = L.take(8), o_state = L.open(zero).take(sizeof(LmState)), o_level = L.take(E),
               o_hpp = L.close(zero).close(up).take<double>(NK * 36), o_bp = L.take<double>(NK * 6), o_hll = L.take<double>(NP * 9),
               o_bl = L.take<double>(NP * 3), o_hpl = L.take<double>(E * 18), o_terms = L.take<double>(E * 32), o_chi = L.take<double>((NP + 31) / 32),
               o_dinv = L.take<double>(NP * 9), o_w = L.take<double>(E * 18), o_minv = L.take<double>((size_t)nf * 36),
               o_blocks = L.open(out).take<double>(NZ * 36), o_rhs = L.take<double>(n);
  L.close(out);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, out.bytes())));
  hipStream_t st = c->stream;
  ba_put(io, in);
  io.put(o_free, free_pose.data(), (size_t)nf * 4);
  so.put(io, sym);
  const int32_t one = 1;
  io.put(o_lambda, &lambda, 8), io.put(o_ok, &one, 4);
  std::memset(io.host<uint8_t>(zero.begin), 0, zero.bytes());
  HIP_TRY(c, io.upload(up));
  LmLaunch K{};
  lm_fill_inputs(K, io, in, p);
  lm_fill_one_system(K, io, {o_state, o_level, in[BA_INFO], o_hpp, o_bp, o_hll, o_bl, o_hpl, o_terms, o_chi});
  launch_lm_build(st, K, 0, 0, 0, true);
  launch_lba_pre(st, p->n_points, p->n_edges, io.dev<int32_t>(in[BA_ET]), io.dev<double>(o_hll), io.dev<double>(o_hpl), io.dev<double>(o_lambda),
                 io.dev<double>(o_dinv), io.dev<double>(o_w), io.dev<int>(o_ok));
  gba_schur(st, io, in, {&sym, &so, o_free, o_hpp, o_bp, o_bl, o_hpl, o_w, o_lambda, o_blocks, o_rhs, o_minv, o_ok});
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(out));
  io.get(blocks, o_blocks, NZ * 288);
  io.get(rhs, o_rhs, n * 8);
  return ORBFE_OK;
}

orbfe_status orbfe_debug_bsr_pcg(orbfe_ctx* c, int32_t nb, const int32_t* row_off, const int32_t* col, const double* blocks, const double* rhs,
                                 double tol, int32_t max_iter, double* x, int32_t* iters, int32_t* ok) {
  ApiLock api_lk(c);
  if (!c || !row_off || !col || !blocks || !rhs || !x || !iters || !ok) return fail(c, ORBFE_EBADARG, "debug_bsr_pcg: NULL argument");
  if (nb < 1 || nb > std::numeric_limits<int32_t>::max() / 36) return fail(c, ORBFE_EBADARG, "debug_bsr_pcg: %d block rows", nb);
  if (row_off[0] != 0) return fail(c, ORBFE_EBADARG, "debug_bsr_pcg: row_off[0] is not 0");
  for (int i = 0; i < nb; ++i) {
    if (row_off[i + 1] < row_off[i]) return fail(c, ORBFE_EBADARG, "debug_bsr_pcg: row_off descends at row %d", i);
    for (int q = row_off[i]; q < row_off[i + 1]; ++q)
      if (col[q] < 0 || col[q] >= nb || (q > row_off[i] && col[q] <= col[q - 1]))
        return fail(c, ORBFE_EBADARG, "debug_bsr_pcg: row %d: column out of range or not ascending", i);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t NB = (size_t)nb, NZ = (size_t)row_off[nb], n = 6 * NB;
  ScratchLayout L;
  ScratchRegion up;
  PcgOffsets po;
  const size_t o_ro = L.open(up).take<int32_t>(NB + 1), o_col = L.take<int32_t>(NZ), o_blk = L.take<double>(NZ * 36), o_rhs = L.take<double>(n),
               o_ok = L.take(8);
  L.close(up);
  po.take(L, NB);
  StagedIo io;
  TRY(io.reserve(c, L.end(), up.end, up.end <= ((size_t)16 << 20)));
  hipStream_t st = c->stream;
  const int32_t one = 1;
  io.put(o_ro, row_off, (NB + 1) * 4), io.put(o_col, col, NZ * 4), io.put(o_blk, blocks, NZ * 288), io.put(o_rhs, rhs, n * 8), io.put(o_ok, &one, 4);
  HIP_TRY(c, io.upload(up));
  BsrPcgLaunch P{};
  P.nb = nb, P.row_off = io.dev<int32_t>(o_ro), P.col = io.dev<int32_t>(o_col), P.blocks = io.dev<double>(o_blk), P.rhs = io.dev<double>(o_rhs),
  P.ok = io.dev<int>(o_ok);
  po.fill(P, io);
  launch_bsr_diag_inv(st, P);
  PcgResult res;
  TRY(run_pcg(c, st, P, tol > 0 ? tol : 1e-10, max_iter > 0 ? max_iter : (int)std::min<int64_t>(24 * (int64_t)nb, std::numeric_limits<int32_t>::max()), &res));
  HIP_TRY(c, hipMemcpyAsync(x, P.x, n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  *iters = res.iters, *ok = res.ok() ? 1 : 0;
  return ORBFE_OK;
}

orbfe_status orbfe_debug_ba_global_phases(double* ms) {
  if (!ms) return ORBFE_EBADARG;
  for (int k = 0; k < 5; ++k) ms[k] = g_gba_phase_ms[k];
  return ORBFE_OK;
}

}  // extern "C"
