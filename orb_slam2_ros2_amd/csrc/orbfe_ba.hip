// orbfe_ba.hip -- the optimiser entry points: g2o edge evaluation and normal equations (diagnostic), the local BA
// (Optimizer::OptimizeLocalMap, Optimizer.cc:336-391) and Optimizer::OptimizePoseOnly (:33-178).  (Split from orbfe_api.hip in r5.)
#include "ba_host.h"
#include "lm_host.h"
namespace {

// one orbfe_ba_local_optimize call: the arguments, what the entry point derived from them, and its ORBFE_LBA_TRACE marks
struct LbaCall {
  orbfe_ctx* c;
  const orbfe_ba_problem* p;
  const uint8_t* pose_fixed;
  int32_t iters_first, iters_second;
  const volatile uint8_t* stop_flag;
  const orbfe_ba_optimize_out* o;
  bool trace;  // ORBFE_LBA_TRACE (diagnostic): host phases of this call on stderr
  BaVertexLists v;
  std::vector<int32_t> slot, free_pose;  // pose -> index among the free poses (-1: fixed) and back
  int nf = 0, pair_cap = 1;              // free poses | the most edges any free pose has
  std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
  orbfe_status device_lm(), host_lm();
  void mark(const char* what) {
    if (!trace) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[orbfe lba] %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(now - t_prev).count());
    t_prev = now;
  }
};

// ---- Levenberg-Marquardt control on the device (k_lm.hip): enqueue the whole optimisation, synchronise once --------------------------
orbfe_status LbaCall::device_lm() {
  const size_t E = (size_t)p->n_edges, NK = (size_t)p->n_poses, NP = (size_t)p->n_points, n = (size_t)6 * nf, NF = (size_t)nf;
  const bool big_solver = nf > LM_CHOL_MAX_NB;  // the blocked multi-workgroup Cholesky of k_lmbig.hip
  mark("pair lists");  // (built on the device: k_lm_pairs)
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  // ONE upload: the inputs and the lists are laid out in page-locked staging memory exactly as in the device scratch and go up as a
  // single asynchronous copy -- eighteen copies from pageable memory were staged by the runtime one by one, ~0.3 ms of a 4 ms call
  ScratchLayout L;
  ScratchRegion up, zero, big_zero, out;
  BaInputs in;
  ba_take(L.open(up), p, pose_fixed, &v, &in);
  const size_t o_info_eff = L.take<double>(E), o_free = L.take<int32_t>(NF), o_slot = L.take<int32_t>(NK),
               o_lmstate = L.take(sizeof(LmState)),  // (the initial control state rides in the one upload)
               // the second estimate, both system buffers, per-edge terms, the blocked reduced system
               o_pose1 = L.close(up).take<double>(NK * 7), o_pt1 = L.take<double>(NP * 3);
  const size_t chi_blocks = (NP + 31) / 32, scale_blocks = (NP + 31) / 32 + (NK + 255) / 256;  // (k_lm_linpoints: a partial sum per block of 32 points)
  size_t o_terms[2], o_hpl[2], o_hpp[2], o_bp[2], o_hll[2], o_bl[2], o_chi[2];
  for (int k = 0; k < 2; ++k)
    o_terms[k] = L.take<double>(E * 32), o_hpl[k] = L.take<double>(E * 18), o_hpp[k] = L.take<double>(NK * 36), o_bp[k] = L.take<double>(NK * 6),
    o_hll[k] = L.take<double>(NP * 9), o_bl[k] = L.take<double>(NP * 3), o_chi[k] = L.take<double>(chi_blocks);
  const size_t KT = big_solver ? (size_t)lm_big_ld(nf) / 48 : 0;
  const size_t o_w = L.take<double>(E * 18), o_rhs = L.take<double>(n),
               o_x = L.take<double>(big_solver ? KT * 48 : n),  // k_lmb_back_mw writes and reads the ld entries of the padded system
               o_ptable = L.take<int32_t>(NF * NP), o_pairs = L.take<int2>(NF * (NF + 1) / 2 * pair_cap), o_paircnt = L.take<int32_t>(NF * (NF + 1) / 2),
               o_sblk = L.take(big_solver ? 8 : NF * (NF + 1) / 2 * 288), o_scale = L.take<double>(scale_blocks),
               o_big = L.open(big_zero).take(big_solver ? lm_big_bytes(nf) : 8),  // big_zero: the matrix and the flags behind it
               o_bigflags = L.take<int32_t>(2 * KT + 1),  // k_lmb_step / k_lmb_back_mw: [KT] bad pivot, [KT + 1, 2 KT + 1) column flags
               o_biginv = L.close(big_zero).take(big_solver ? lm_big_inv_bytes(nf) : 8),
               // zero: one block that starts as zeros (ONE fill): edge levels | chi2 of the last linearisation | point inverses
               o_level = L.open(zero).take(E), o_last = L.take<double>(E), o_dinv = L.take<double>(NP * 9),
               // out: the results as ONE block (one download): poses | points | chi2 | level | bad | the control state as the last control step left it
               o_pose_out = L.close(zero).open(out).take<double>(NK * 7), o_pt_out = L.take<double>(NP * 3), o_chi2_out = L.take<double>(E),
               o_level_out = L.take(E), o_bad_out = L.take(E), o_state_out = L.take(sizeof(LmState));
  L.close(out);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, out.bytes())));  // (the staging buffer is also the target of the one result download)
  hipStream_t st = c->stream;
  ba_put(io, in);
  io.put(o_info_eff, p->info, E * 8);
  io.put(o_free, free_pose.data(), NF * 4);
  io.put(o_slot, slot.data(), NK * 4);
  LmState init{};
  init.iters[0] = iters_first, init.iters[1] = iters_second, init.need_chi = 1, init.ok = 1;
  io.put(o_lmstate, &init, sizeof init);
  mark("stage inputs");
  HIP_TRY(c, io.upload(up));
  HIP_TRY(c, hipMemsetAsync(io.dev<uint8_t>(zero.begin), 0, zero.bytes(), st));  // (every memset is a launch of 4.6 us: six of them preceded the first kernel)
  if (!c->h_abort) HIP_TRY(c, hipHostMalloc((void**)&c->h_abort, 64, hipHostMallocMapped));
  void* d_abort = nullptr;
  HIP_TRY(c, hipHostGetDevicePointer(&d_abort, (void*)c->h_abort, 0));
  *c->h_abort = (stop_flag && *stop_flag) ? 1 : 0;
  LmLaunch K{};
  lm_fill_inputs(K, io, in, p);
  K.nf = nf;
  K.B.poses[1] = io.dev<double>(o_pose1), K.B.points[1] = io.dev<double>(o_pt1);
  for (int k = 0; k < 2; ++k)
    K.B.terms[k] = io.dev<double>(o_terms[k]), K.B.Hpl[k] = io.dev<double>(o_hpl[k]), K.B.Hpp[k] = io.dev<double>(o_hpp[k]),
    K.B.bp[k] = io.dev<double>(o_bp[k]), K.B.Hll[k] = io.dev<double>(o_hll[k]), K.B.bl[k] = io.dev<double>(o_bl[k]),
    K.B.chi_part[k] = io.dev<double>(o_chi[k]);
  K.state = io.dev<LmState>(o_lmstate);
  K.free_pose = io.dev<int32_t>(o_free), K.pose_slot = io.dev<int32_t>(o_slot);
  K.pairs = io.dev<int2>(o_pairs), K.pair_cnt = io.dev<int32_t>(o_paircnt), K.pair_table = io.dev<int32_t>(o_ptable), K.pair_cap = pair_cap;
  K.info_eff = io.dev<double>(o_info_eff), K.chi2_last = io.dev<double>(o_last), K.level = io.dev<uint8_t>(o_level);
  K.Dinv = io.dev<double>(o_dinv), K.W = io.dev<double>(o_w), K.Sblk = io.dev<double>(o_sblk), K.rhs = io.dev<double>(o_rhs), K.x = io.dev<double>(o_x);
  K.scale_part = io.dev<double>(o_scale), K.chi2_out = io.dev<double>(o_chi2_out), K.poses_out = io.dev<double>(o_pose_out);
  K.points_out = io.dev<double>(o_pt_out), K.bad = io.dev<uint8_t>(o_bad_out), K.level_out = io.dev<uint8_t>(o_level_out);
  K.abort_flag = (const volatile uint8_t*)d_abort;
  // (the initial state went up with the inputs; the ticket and the point inverses -- read by a trial whose point block was singular --
  //  are part of the one zero fill)
  K.state_out = io.dev<LmState>(o_state_out);
  K.M = big_solver ? io.dev<double>(o_big) : nullptr, K.ld = big_solver ? lm_big_ld(nf) : 0, K.lmb_flags = io.dev<int32_t>(o_bigflags),
  K.lmb_inv = io.dev<double>(o_biginv);
  StageTimer tm(c, ORBFE_STAGE_BA, st);
  if (big_solver) {
    HIP_TRY(c, hipMemsetAsync(io.dev<uint8_t>(big_zero.begin), 0, big_zero.bytes(), st));
    launch_lm_big_init(st, K);
  }
  HIP_TRY(c, hipMemsetAsync(K.pair_table, 0xFF, NF * NP * 4, st));
  launch_lm_pairs(st, K);
  launch_lm_build(st, K, 0, 0, iters_first > 0 ? 1 : 0, true);  // computeActiveErrors + buildSystem at the initial estimate
  launch_lm_maxdiag(st, K, 0);
  // trials provisioned per pass: every iteration needs at least one, a rejected trial costs one more; what is left over runs as no-ops
  // (a few microseconds each), what is missing is enqueued in the next pass, after the one synchronisation of this one
  // (measured: a provisioned trial that turns out not to be needed is six empty launches of 4.6 us; one spare
  // -- in round 0, where coming up one short would leave the ten trials of round 1 as no-ops in this pass; round 1 gets none: if a trial
  // of it is rejected, the second pass enqueues what is missing)
  int steps_a = std::min(iters_first + 1, 24), steps_b = std::min(iters_second, 24);
  LmState fin{};
  for (int pass = 0;; ++pass) {
    launch_lm_steps(st, K, steps_a);
    launch_lm_switch(st, K);
    launch_lm_steps(st, K, steps_b);
    launch_lm_final(st, K);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, io.download(out));  // the upload from the staging buffer finished long ago (stream order)
    if (stop_flag) {
      // the device polls the mapped byte between the trials; the caller's flag (LocalMapping::mbAbortBA, written by the Tracking
      // thread) is mirrored into it while this thread waits
      hipEvent_t ev = nullptr;
      HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      hipError_t er = hipEventRecord(ev, st);
      while (er == hipSuccess) {
        if (*stop_flag) *c->h_abort = 1;
        er = hipEventQuery(ev);
        if (er == hipErrorNotReady) {
          (void)hipGetLastError();
          er = hipSuccess;
          sched_yield();
          continue;
        }
        break;
      }
      (void)hipEventDestroy(ev);
      HIP_TRY(c, er);
    }
    mark("enqueue");
    HIP_TRY(c, io.wait());
    mark("device (wait)");
    io.get(&fin, o_state_out, sizeof fin);
    if (fin.finalized) {
      io.get(o->poses, o_pose_out, NK * 56);
      io.get(o->points, o_pt_out, NP * 24);
      io.get(o->chi2, o_chi2_out, E * 8);
      io.get(o->level, o_level_out, E);
      io.get(o->bad, o_bad_out, E);
      break;
    }
    if (pass >= 4096) return fail(c, ORBFE_EDEVICE, "ba_local_optimize: the device-side Levenberg-Marquardt loop did not finish (round %d, phase %d)", fin.round, fin.phase);
    // more trials were needed than provisioned: continue where the state stands
    steps_a = fin.switched || fin.round == 2 ? 0 : std::min(std::max(iters_first - fin.it, 0) + 2, 24);
    steps_b = std::min((fin.switched ? std::max(iters_second - fin.it, 0) : iters_second) + 2, 24);
  }
  if (o->iterations) {
    o->iterations[0] = fin.done[0];
    o->iterations[1] = fin.done[1];
  }
  drain_timers(c);
  mark("results out");
  return ORBFE_OK;
}

// ---- g2o's Levenberg-Marquardt control on the host (a handful of scalars per trial), every vertex / edge / block operation on the device:
// ORBFE_LBA_HOST_LM=1, more than LM_BIG_MAX_NB free keyframes, or a pose that observes a point twice ------------------------------------
orbfe_status LbaCall::host_lm() {
  const int E = p->n_edges, NK = p->n_poses, NP = p->n_points;
  // pose-pair lists of the Schur complement: for every pair (i, j) of free poses, the edge pairs (e1, e2) through a common point
  auto each_pair = [&](auto&& f) {
    for (int pt = 0; pt < NP; ++pt)
      for (int q1 = v.pt_off[pt]; q1 < v.pt_off[pt + 1]; ++q1) {
        const int e1 = v.pt_edges[q1], i = slot[p->edge_pose[e1]];
        if (i < 0) continue;
        for (int q2 = v.pt_off[pt]; q2 < v.pt_off[pt + 1]; ++q2) {
          const int e2 = v.pt_edges[q2], j = slot[p->edge_pose[e2]];
          if (j >= 0) f((size_t)i * nf + j, e1, e2);
        }
      }
  };
  std::vector<int32_t> pair_off((size_t)nf * nf + 1, 0);
  each_pair([&](size_t q, int, int) { ++pair_off[q + 1]; });
  for (size_t q = 0; q < (size_t)nf * nf; ++q) pair_off[q + 1] += pair_off[q];
  std::vector<int2> pairs(pair_off.back());
  std::vector<int32_t> cur(pair_off.begin(), pair_off.end() - 1);
  each_pair([&](size_t q, int e1, int e2) { pairs[cur[q]++] = make_int2(e1, e2); });
  mark("pair lists");
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t n = (size_t)6 * nf, NE = (size_t)E, NKs = (size_t)NK, NPs = (size_t)NP;
  ScratchLayout L;
  ScratchRegion up, zero;
  BaInputs in;
  ba_take(L.open(up), p, pose_fixed, &v, &in);
  const size_t o_info_eff = L.take<double>(NE), o_free = L.take<int32_t>((size_t)nf), o_slot = L.take<int32_t>(NKs),
               o_pairoff = L.take<int32_t>(pair_off.size()), o_pairs = L.take<int2>(pairs.size()), o_pose_bk = L.close(up).take<double>(NKs * 7),
               o_pt_bk = L.take<double>(NPs * 3), o_hpp = L.take<double>(NKs * 36), o_bp = L.take<double>(NKs * 6), o_hll = L.take<double>(NPs * 9),
               o_bl = L.take<double>(NPs * 3), o_hpl = L.take<double>(NE * 18), o_w = L.take<double>(NE * 18), o_s = L.take<double>(n * n),
               o_rhs = L.take<double>(n), o_x = L.take<double>(n), o_dxp = L.take<double>(NKs * 6), o_dxl = L.take<double>(NPs * 3),
               o_err = L.take<double>(NE * 3), o_chi2 = L.take<double>(NE), o_rho = L.take<double>(NE * 2),
               o_terms = L.take<double>(NE * 32), o_chipart = L.take<double>((NPs + 31) / 32),  // the system builder's (k_lm_linpoints)
               // zero: one block that starts as zeros (ONE fill): edge levels | chi2 of the last linearisation | point inverses | the
               // system builder's control state (buffer 0 current)
               o_level = L.open(zero).take(NE), o_last = L.take<double>(NE), o_dinv = L.take<double>(NPs * 9), o_lmstate = L.take(sizeof(LmState)),
               o_depth = L.close(zero).take(NE),
               o_bad = L.take(NE), o_sc = L.take<double>(5),
               o_big = L.take(nf > LBA_MAX_FREE ? ((n + 1) * 6 + (size_t)nf * 36 + n) * 8 : 8);  // launch_lba_solve's panel in global memory
  const size_t o_pose = in[BA_POSE], o_pt = in[BA_PT], o_meas = in[BA_MEAS], o_st = in[BA_ST], o_info = in[BA_INFO], o_delta = in[BA_DELTA],
               o_fix = in[BA_FIX], o_pto = in[BA_PTO], o_pte = in[BA_PTE], o_pso = in[BA_PSO], o_pse = in[BA_PSE];
  StagedIo io;
  TRY(io.reserve(c, L.end(), up.end));
  uint8_t* b = io.d;
  hipStream_t st = c->stream;
  ba_put(io, in);
  io.put(o_info_eff, p->info, NE * 8);
  io.put(o_free, free_pose.data(), (size_t)nf * 4);
  io.put(o_slot, slot.data(), NKs * 4);
  io.put(o_pairoff, pair_off.data(), pair_off.size() * 4);
  io.put(o_pairs, pairs.data(), pairs.size() * 8);
  mark("stage inputs");
  HIP_TRY(c, io.upload(up));
  HIP_TRY(c, hipMemsetAsync(b + zero.begin, 0, zero.bytes(), st));  // (every memset is a launch of 4.6 us: six of them preceded the first kernel)

  const BaParamsDev prm = {p->fx, p->fy, p->cx, p->cy, p->bf};
  // buildSystem: the builders of the device-side path (k_lm.hip) at the one estimate this loop keeps
  LmLaunch K{};
  lm_fill_inputs(K, io, in, p);
  lm_fill_one_system(K, io, {o_lmstate, o_level, o_info_eff, o_hpp, o_bp, o_hll, o_bl, o_hpl, o_terms, o_chipart});
  double* d_poses = (double*)(b + o_pose);
  double* d_points = (double*)(b + o_pt);
  const int32_t* d_ek = (const int32_t*)(b + in[BA_EP]);
  const int32_t* d_ep = (const int32_t*)(b + in[BA_ET]);
  double* d_sc = (double*)(b + o_sc);  // the loop's five scalars (lm_host.h)
  auto edges = [&](size_t o_inf) {  // computeError() on every edge, with the given information values
    launch_ba_edges(st, E, d_poses, d_points, d_ek, d_ep, (const double*)(b + o_meas), b + o_st, (const double*)(b + o_inf),
                    (const double*)(b + o_delta), prm, (double*)(b + o_err), (double*)(b + o_chi2), (double*)(b + o_rho), nullptr, nullptr,
                    b + o_depth);
  };
  auto evaluate = [&]() {  // computeActiveErrors + activeRobustChi2
    edges(o_info_eff);
    launch_lba_chi2_sum(st, E, (const double*)(b + o_chi2), (const double*)(b + o_rho), b + o_level, (double*)(b + o_last), d_sc);
  };
  auto stopped = [&]() { return stop_flag && *stop_flag; };
  StageTimer tm(c, ORBFE_STAGE_BA, st);
  auto optimize = [&](int iterations, int32_t& done) -> orbfe_status {  // SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve (lm_host.h)
    done = 0;
    if (E == 0) return ORBFE_OK;
    auto linearize = [&](int it) -> orbfe_status {
      evaluate();
      launch_lm_build(st, K, 0, 0, 0, true);
      if (it == 0) launch_lba_maxdiag(st, NK, NP, (const double*)(b + o_hpp), (const double*)(b + o_hll), b + o_fix, d_sc + 1);
      return ORBFE_OK;
    };
    auto trial = [&](double lambda, bool&) -> orbfe_status {
      HIP_TRY(c, hipMemcpyAsync(b + o_pose_bk, d_poses, (size_t)NK * 56, hipMemcpyDeviceToDevice, st));  // push()
      HIP_TRY(c, hipMemcpyAsync(b + o_pt_bk, d_points, (size_t)NP * 24, hipMemcpyDeviceToDevice, st));
      HIP_TRY(c, lm_host_upload(st, d_sc, lambda));
      launch_lba_solve(st, NK, NP, E, nf, (const int32_t*)(b + o_free), (const int32_t*)(b + o_slot), (const int32_t*)(b + o_pairoff),
                       (const int2*)(b + o_pairs), (const int32_t*)(b + o_pso), (const int32_t*)(b + o_pse), (const int32_t*)(b + o_pto),
                       (const int32_t*)(b + o_pte), d_ek, d_ep, b + o_fix, (const double*)(b + o_hpp), (const double*)(b + o_bp),
                       (const double*)(b + o_hll), (const double*)(b + o_bl), (const double*)(b + o_hpl), d_sc + 2, (double*)(b + o_dinv),
                       (double*)(b + o_w), (double*)(b + o_s), (double*)(b + o_rhs), (double*)(b + o_x), (int*)(d_sc + 3), d_poses, d_points,
                       (double*)(b + o_dxp), (double*)(b + o_dxl), d_sc + 4, (double*)(b + o_big));
      evaluate();
      return ORBFE_OK;
    };
    auto on_accept = [&]() -> orbfe_status { return ORBFE_OK; };
    auto on_reject = [&](bool) -> orbfe_status {
      HIP_TRY(c, hipMemcpyAsync(d_poses, b + o_pose_bk, (size_t)NK * 56, hipMemcpyDeviceToDevice, st));  // pop()
      HIP_TRY(c, hipMemcpyAsync(d_points, b + o_pt_bk, (size_t)NP * 24, hipMemcpyDeviceToDevice, st));
      return ORBFE_OK;
    };
    int32_t trials;
    return lm_host_optimize(c, st, d_sc, iterations, stop_flag, done, trials, linearize, trial, on_accept, on_reject, [](int) {});
  };
  int32_t it1 = 0, it2 = 0;
  TRY(optimize(iters_first, it1));
  if (!stopped()) {
    // edge->chi2() is the chi2 of the last evaluated trial; isDepthPositive() reads the current estimates (Optimizer.cc:338-359)
    edges(o_info);
    launch_lba_classify(st, E, (const double*)(b + o_last), b + o_depth, b + o_st, b + o_level, (double*)(b + o_info_eff),
                        (double*)(b + o_delta));
    TRY(optimize(iters_second, it2));
  }
  // final computeError() on every edge with the final estimates (Optimizer.cc:364-391)
  edges(o_info);
  launch_lba_final(st, E, (const double*)(b + o_chi2), b + o_depth, b + o_st, b + o_bad);
  HIP_TRY(c, hipGetLastError());
  io.staged = false;  // the results go straight from the scratch to the caller's arrays
  io.get(o->poses, o_pose, NKs * 56);
  io.get(o->points, o_pt, NPs * 24);
  io.get(o->level, o_level, NE);
  io.get(o->chi2, o_chi2, NE * 8);
  io.get(o->bad, o_bad, NE);
  HIP_TRY(c, io.wait());
  if (o->iterations) {
    o->iterations[0] = it1;
    o->iterations[1] = it2;
  }
  return ORBFE_OK;
}

}  // namespace

extern "C" {

orbfe_status orbfe_ba_eval_edges(orbfe_ctx* c, const orbfe_ba_problem* p, const orbfe_ba_edge_out* o) {
  ApiLock api_lk(c);
  if (!c || !p || !o) return fail(c, ORBFE_EBADARG, "ba_eval_edges: NULL argument");
  const int E = p->n_edges;
  if (E < 0 || p->n_poses < 0 || p->n_points < 0) return fail(c, ORBFE_EBADARG, "ba_eval_edges: negative size");
  if (E == 0) return ORBFE_OK;
  if (!p->poses || !p->points || !p->edge_pose || !p->edge_point || !p->meas || !p->is_stereo || !p->info || !p->huber_delta || !o->error ||
      !o->chi2 || !o->rho)
    return fail(c, ORBFE_EBADARG, "ba_eval_edges: NULL array");
  TRY(ba_check_problem(c, "ba_eval_edges", p));
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t NE = (size_t)E;
  ScratchLayout L;
  ScratchRegion up, out;
  BaInputs in;
  ba_take(L.open(up), p, nullptr, nullptr, &in);
  const size_t o_err = L.close(up).open(out).take<double>(NE * 3), o_chi = L.take<double>(NE), o_rho = L.take<double>(NE * 2), o_dp = L.take(NE),
               o_jpt = L.take<double>(NE * 9), o_jps = L.take<double>(NE * 18);
  L.close(out);
  // up to 16 MB in all: inputs as ONE upload through the page-locked staging buffer and the results as one download (eight copies from
  // and six to pageable memory otherwise -- each staged by the runtime on its own)
  const ScratchRegion down = o->j_pose ? out : out.upto(o->j_point ? o_jps : o_jpt);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes()), up.end + down.bytes() <= ((size_t)16 << 20)));
  ba_put(io, in);
  HIP_TRY(c, io.upload(up));
  BaParamsDev prm = {p->fx, p->fy, p->cx, p->cy, p->bf};
  {
    StageTimer tm(c, ORBFE_STAGE_BA, c->stream);
    launch_ba_edges(c->stream, E, io.dev<double>(in[BA_POSE]), io.dev<double>(in[BA_PT]), io.dev<int32_t>(in[BA_EP]), io.dev<int32_t>(in[BA_ET]),
                    io.dev<double>(in[BA_MEAS]), io.dev<uint8_t>(in[BA_ST]), io.dev<double>(in[BA_INFO]), io.dev<double>(in[BA_DELTA]), prm,
                    io.dev<double>(o_err), io.dev<double>(o_chi), io.dev<double>(o_rho), o->j_point ? io.dev<double>(o_jpt) : nullptr,
                    o->j_pose ? io.dev<double>(o_jps) : nullptr, o->depth_positive ? io.dev<uint8_t>(o_dp) : nullptr);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.download(down));
  if (io.staged) HIP_TRY(c, io.wait());  // (staged: get reads the downloaded block; unstaged: get is the copy, waited for below)
  io.get(o->error, o_err, NE * 24);
  io.get(o->chi2, o_chi, NE * 8);
  io.get(o->rho, o_rho, NE * 16);
  io.get(o->j_point, o_jpt, NE * 72);
  io.get(o->j_pose, o_jps, NE * 144);
  io.get(o->depth_positive, o_dp, NE);
  if (!io.staged) HIP_TRY(c, io.wait());
  drain_timers(c);
  return ORBFE_OK;
}

orbfe_status orbfe_ba_build_system(orbfe_ctx* c, const orbfe_ba_problem* p, const uint8_t* pose_fixed, const orbfe_ba_system_out* o) {
  ApiLock api_lk(c);
  if (!c || !p || !o) return fail(c, ORBFE_EBADARG, "ba_build_system: NULL argument");
  const size_t E = (size_t)p->n_edges, NK = (size_t)p->n_poses, NP = (size_t)p->n_points;
  if (p->n_edges < 0 || p->n_poses < 0 || p->n_points < 0) return fail(c, ORBFE_EBADARG, "ba_build_system: negative size");
  if (!o->Hpp || !o->bp || !o->Hll || !o->bl) return fail(c, ORBFE_EBADARG, "ba_build_system: NULL output");
  if (E && (!p->poses || !p->points || !p->edge_pose || !p->edge_point || !p->meas || !p->is_stereo || !p->info || !p->huber_delta))
    return fail(c, ORBFE_EBADARG, "ba_build_system: NULL array");
  TRY(ba_check_problem(c, "ba_build_system", p));
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  BaVertexLists v;
  ba_vertex_lists(p, &v);
  // r3: the system is built by the kernels of the device-side Levenberg-Marquardt path (k_lm.hip: every edge linearised once, eight lanes
  // per point, a workgroup per pose -- 22 us where round 1's three kernels, each recomputing every edge's Jacobians, took 171); inputs
  // and lists go up as ONE block through the page-locked staging buffer, the blocks come back as one
  ScratchLayout L;
  ScratchRegion up, zero, out;  // zero: control state (buffer 0 current) and the edge levels (all active), the tail of the upload
  BaInputs in;
  ba_take(L.open(up), p, pose_fixed, &v, &in);
  const size_t o_state = L.open(zero).take(sizeof(LmState)), o_level = L.take(E), o_hpp = L.close(zero).close(up).open(out).take<double>(NK * 36),
               o_bp = L.take<double>(NK * 6), o_hll = L.take<double>(NP * 9), o_bl = L.take<double>(NP * 3), o_hpl = L.take<double>(E * 18),
               o_terms = L.close(out).take<double>(E * 32), o_chi = L.take<double>((NP + 31) / 32);
  const ScratchRegion down = o->Hpl ? out : out.upto(o_hpl);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes())));
  ba_put(io, in);
  std::memset(io.host<uint8_t>(zero.begin), 0, zero.bytes());
  HIP_TRY(c, io.upload(up));
  {
    LmLaunch K{};
    lm_fill_inputs(K, io, in, p);
    lm_fill_one_system(K, io, {o_state, o_level, in[BA_INFO], o_hpp, o_bp, o_hll, o_bl, o_hpl, o_terms, o_chi});
    StageTimer tm(c, ORBFE_STAGE_BA, c->stream);
    launch_lm_build(c->stream, K, 0, 0, 0, true);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down));
  drain_timers(c);
  io.get(o->Hpp, o_hpp, NK * 288);
  io.get(o->bp, o_bp, NK * 48);
  io.get(o->Hll, o_hll, NP * 72);
  io.get(o->bl, o_bl, NP * 24);
  io.get(o->Hpl, o_hpl, E * 144);
  return ORBFE_OK;
}

// Optimizer::OptimizeLocalMap's two optimize() calls (Optimizer.cc:336-362): validate, build the vertex lists, then one of the two
// optimisers above.
orbfe_status orbfe_ba_local_optimize(orbfe_ctx* c, const orbfe_ba_problem* p, const uint8_t* pose_fixed, int32_t iters_first,
                                     int32_t iters_second, const volatile uint8_t* stop_flag, const orbfe_ba_optimize_out* o) {
  ApiLock api_lk(c);
  static const bool trace_host = getenv("ORBFE_LBA_TRACE") != nullptr;
  LbaCall a{c, p, pose_fixed, iters_first, iters_second, stop_flag, o, trace_host};
  if (!c || !p || !o) return fail(c, ORBFE_EBADARG, "ba_local_optimize: NULL argument");
  const int E = p->n_edges, NK = p->n_poses, NP = p->n_points;
  if (E < 0 || NK < 0 || NP < 0 || iters_first < 0 || iters_second < 0) return fail(c, ORBFE_EBADARG, "ba_local_optimize: negative size");
  if (!o->poses || !o->points) return fail(c, ORBFE_EBADARG, "ba_local_optimize: NULL output");
  if ((NK && !p->poses) || (NP && !p->points) ||
      (E && (!p->edge_pose || !p->edge_point || !p->meas || !p->is_stereo || !p->info || !p->huber_delta)))
    return fail(c, ORBFE_EBADARG, "ba_local_optimize: NULL array");
  TRY(ba_check_problem(c, "ba_local_optimize", p));
  a.slot.assign(NK, -1);
  for (int k = 0; k < NK; ++k)
    if (!(pose_fixed && pose_fixed[k])) {
      a.slot[k] = (int32_t)a.free_pose.size();
      a.free_pose.push_back(k);
    }
  a.nf = (int)a.free_pose.size();
  // (no bound on nf.  The reduced system is factorised by one of four solvers:
  //    device-side control, 1..LM_CHOL_MAX_NB free keyframes             k_lm_chol (k_lm.hip): one workgroup, the matrix in registers
  //    device-side control, LM_CHOL_MAX_NB + 1..LM_BIG_MAX_NB            k_lmb_step / k_lmb_back_mw (k_lmbig.hip): 48 x 48 tiles, fp64 MFMA
  //    host-driven loop, up to LBA_MAX_FREE                              k_lba_chol_solve (k_lba.hip): one workgroup out of LDS
  //    host-driven loop, past LBA_MAX_FREE                               k_lba_chol_panel / _trail / _back: the panel in global memory
  //  the host-driven loop runs when a pose observes a point twice, past LM_BIG_MAX_NB free keyframes, or under ORBFE_LBA_HOST_LM=1)
  ba_vertex_lists(p, &a.v);
  // The device-side Levenberg-Marquardt path (k_lm.hip) builds the pair lists of the reduced system itself, from a (pose, point) -> edge
  // table: that needs a pose to observe a point at most once (as every map of the reference does); anything else takes the host-driven path.
  bool single_obs = true;
  {
    std::vector<int32_t> seen(NK, -1);
    for (int pt = 0; pt < NP && single_obs; ++pt)
      for (int q = a.v.pt_off[pt]; q < a.v.pt_off[pt + 1]; ++q) {
        const int k = p->edge_pose[a.v.pt_edges[q]];
        if (seen[k] == pt) {
          single_obs = false;
          break;
        }
        seen[k] = pt;
      }
    for (int k = 0; k < NK; ++k)
      if (a.slot[k] >= 0) a.pair_cap = std::max(a.pair_cap, a.v.ps_off[k + 1] - a.v.ps_off[k]);
  }
  a.mark("validate + vertex lists");
  const bool dev_lm = c->lm_on_device && E > 0 && a.nf <= LM_BIG_MAX_NB && single_obs;
  return dev_lm ? a.device_lm() : a.host_lm();
}

orbfe_status orbfe_pose_only_optimize(orbfe_ctx* c, int32_t n, const double* xw, const double* meas, const double* info, const float* sigma2,
                                      const double* pose_in, double fx, double fy, double cx, double cy, double bf, double* pose_out,
                                      uint8_t* inlier_out, int32_t* n_good) {
  ApiLock api_lk(c);
  if (!c || n < 0 || !pose_in || !pose_out || !n_good || (n && (!xw || !meas || !info || !sigma2)))
    return fail(c, ORBFE_EBADARG, "pose_only_optimize: NULL argument");
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t N = (size_t)n;
  // inputs as ONE upload through the page-locked staging buffer, results as one download (five copies from pageable memory up and three down
  // were a fifth of the call)
  ScratchLayout L;
  ScratchRegion up, out;
  const size_t o_x = L.open(up).take<double>(N * 3), o_m = L.take<double>(N * 3), o_i = L.take<double>(N), o_s = L.take<float>(N), o_p = L.take(56),
               o_po = L.close(up).open(out).take(56), o_ng = L.take(8), o_in = L.take(N), o_e = L.close(out).take<double>(N * 3), o_l = L.take(N),
               o_r = L.take(N);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, out.bytes())));
  io.put(o_x, xw, N * 24);
  io.put(o_m, meas, N * 24);
  io.put(o_i, info, N * 8);
  io.put(o_s, sigma2, N * 4);
  io.put(o_p, pose_in, 56);
  HIP_TRY(c, io.upload(up));
  BaParamsDev prm = {fx, fy, cx, cy, bf};
  {
    StageTimer tm(c, ORBFE_STAGE_BA, c->stream);
    launch_pose_only(c->stream, n, io.dev<double>(o_x), io.dev<double>(o_m), io.dev<double>(o_i), io.dev<float>(o_s), io.dev<double>(o_p), prm,
                     (double)(float)std::sqrt(5.991), (double)(float)std::sqrt(7.815), io.dev<double>(o_e), io.dev<uint8_t>(o_l),
                     io.dev<uint8_t>(o_r), io.dev<uint8_t>(o_in), io.dev<double>(o_po), io.dev<int32_t>(o_ng));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(out.upto(inlier_out ? o_in + N : o_in)));  // (the inlier flags only if the caller wants them, and only n of them)
  drain_timers(c);
  io.get(pose_out, o_po, 56);
  io.get(n_good, o_ng, 4);
  io.get(inlier_out, o_in, N);
  return ORBFE_OK;
}

orbfe_status orbfe_debug_se3_oplus(orbfe_ctx* c, int32_t n, const double* poses, const double* upd, double* out) {
  ApiLock api_lk(c);
  if (!c || n < 0 || !poses || !upd || !out) return fail(c, ORBFE_EBADARG, "debug_se3_oplus: bad argument");
  if (n == 0) return ORBFE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t N = (size_t)n;
  ScratchLayout L;
  ScratchRegion up, down;
  const size_t o_p = L.open(up).take<double>(N * 7), o_u = L.take<double>(N * 6), o_o = L.close(up).open(down).take<double>(N * 7);
  L.close(down);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes())));
  io.put(o_p, poses, N * 56);
  io.put(o_u, upd, N * 48);
  HIP_TRY(c, io.upload(up));
  launch_debug_se3_oplus(c->stream, n, io.dev<double>(o_p), io.dev<double>(o_u), io.dev<double>(o_o));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down));
  io.get(out, o_o, N * 56);
  return ORBFE_OK;
}

// One reduced camera system through one of the four Cholesky solvers of the local BA, each in the layout and through the launch code
// orbfe_ba_local_optimize gives it (launch_lm_chol: k_lm_chol | k_lmbig; launch_lba_chol: LDS-resident | panel).
orbfe_status orbfe_debug_reduced_solve(orbfe_ctx* c, int32_t solver, int32_t nb, const double* S, const double* rhs, double* x, int32_t* ok) {
  ApiLock api_lk(c);
  if (!c || !S || !rhs || !x || !ok) return fail(c, ORBFE_EBADARG, "debug_reduced_solve: NULL argument");
  // the block rows production gives each solver (solver 3: as many as 6 nb indexes as an int)
  static const int32_t lo[4] = {1, LM_CHOL_MAX_NB + 1, 1, LBA_MAX_FREE + 1};
  static const int32_t hi[4] = {LM_CHOL_MAX_NB, LM_BIG_MAX_NB, LBA_MAX_FREE, std::numeric_limits<int32_t>::max() / 6};
  if (solver < 0 || solver > 3) return fail(c, ORBFE_EBADARG, "debug_reduced_solve: solver %d (0 registers, 1 blocked, 2 LDS, 3 panel)", solver);
  if (nb < lo[solver] || nb > hi[solver])
    return fail(c, ORBFE_EBADARG, "debug_reduced_solve: solver %d takes %d..%d block rows, not %d", solver, lo[solver], hi[solver], nb);
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t NB = (size_t)nb, n = 6 * NB;
  const bool lm = solver < 2, big = solver == 1, panel = solver == 3;
  const size_t ld = big ? (size_t)lm_big_ld(nb) : 0, KT = ld / 48;
  // the system as the solver's Schur kernel leaves it.  Solvers 0 and 1 (k_lm_schur): the 6x6 blocks (I, J), I >= J, whole -- packed
  // row-major for solver 0; for solver 1 an n x n row-major square (blocks above the diagonal zero) that is copied into the zero-filled,
  // padded matrix.  Solvers 2 and 3 (k_lba_schur): all of S, column-major.
  std::vector<double> pack(solver == 0 ? NB * (NB + 1) / 2 * 36 : n * n, 0.0);
  for (size_t I = 0; I < NB; ++I)
    for (size_t J = 0; J < (lm ? I + 1 : NB); ++J)
      for (size_t a = 0; a < 6; ++a)
        for (size_t b = 0; b < 6; ++b) {
          const size_t r = 6 * I + a, q = 6 * J + b;
          pack[solver == 0 ? (I * (I + 1) / 2 + J) * 36 + 6 * a + b : (big ? r * n + q : r + q * n)] = S[r * n + q];
        }
  ScratchLayout L;
  ScratchRegion up, down;
  const size_t o_s = L.open(up).take<double>(pack.size()), o_rhs = L.take<double>(n),
               o_st = L.open(down).take(lm ? sizeof(LmState) : sizeof(int32_t)),  // the control state | the host-driven loop's ok word
               o_x = L.close(up).take<double>(big ? KT * 48 : n),                 // (k_lmb_back_mw writes the ld entries of the padded system)
               o_m = L.close(down).take(big ? lm_big_bytes(nb) : 8), o_inv = L.take(big ? lm_big_inv_bytes(nb) : 8),
               o_panel = L.take(panel ? ((n + 1) * 6 + NB * 36 + n) * 8 : 8);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes()), up.end + down.bytes() <= ((size_t)16 << 20)));
  hipStream_t st = c->stream;
  LmState init{};
  init.run_step = 1, init.ok = 1;
  const int32_t ok_init = 1;
  LmState fin{};
  int32_t ok_fin = 0;
  io.put(o_s, pack.data(), pack.size() * 8);
  io.put(o_rhs, rhs, n * 8);
  if (lm) io.put(o_st, &init, sizeof init);
  else io.put(o_st, &ok_init, sizeof ok_init);
  HIP_TRY(c, io.upload(up));
  if (lm) {
    LmLaunch K{};
    K.nf = nb, K.state = io.dev<LmState>(o_st), K.Sblk = io.dev<double>(o_s), K.rhs = io.dev<double>(o_rhs), K.x = io.dev<double>(o_x);
    if (big) {
      // the flags outlive the call: a bad pivot's flag is cleared by the first launch of the NEXT factorisation, here as between two trials
      if (!c->d_dbg_lmb_flags) TRY(dev_alloc(c, &c->d_dbg_lmb_flags, (size_t)2 * (lm_big_ld(LM_BIG_MAX_NB) / 48) + 1));
      if (c->dbg_lmb_kt != (int)KT) HIP_TRY(c, hipMemsetAsync(c->d_dbg_lmb_flags, 0, (2 * KT + 1) * 4, st));
      c->dbg_lmb_kt = (int)KT;
      K.M = io.dev<double>(o_m), K.ld = (int)ld, K.lmb_flags = c->d_dbg_lmb_flags, K.lmb_inv = io.dev<double>(o_inv);
      // as device_lm: zero fill, unit padding diagonal; then what k_lm_schur writes: the blocks into rows [0, n), the right-hand side into row ld
      HIP_TRY(c, hipMemsetAsync(K.M, 0, lm_big_bytes(nb), st));
      launch_lm_big_init(st, K);
      HIP_TRY(c, hipMemcpy2DAsync(K.M, ld * 8, io.dev<double>(o_s), n * 8, n * 8, n, hipMemcpyDeviceToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(K.M + ld * ld, K.rhs, n * 8, hipMemcpyDeviceToDevice, st));
    }
    launch_lm_chol(st, K);
  } else {
    launch_lba_chol(st, nb, io.dev<double>(o_s), io.dev<double>(o_rhs), io.dev<double>(o_x), io.dev<int>(o_st), io.dev<double>(o_panel));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.download(big ? down.upto(o_x + n * 8) : down));
  if (io.staged) HIP_TRY(c, io.wait());
  if (lm) io.get(&fin, o_st, sizeof fin);
  else io.get(&ok_fin, o_st, sizeof ok_fin);
  io.get(x, o_x, n * 8);
  if (!io.staged) HIP_TRY(c, io.wait());
  *ok = lm ? fin.ok : ok_fin;
  return ORBFE_OK;
}

}  // extern "C"
