// orbfe_sim3opt.hip -- host side of orbfe_sim3_optimize and orbfe_debug_sim3_edges (include/orbfe.h): the arguments checked, one upload,
// one launch, one download through the context's scratch block and staging.  The kernel: k_sim3opt.hip; the edge model: sim3_edge_dev.h.
#include "orbfe_ctx.h"
#include "sim3_edge_dev.h"

namespace {

// the six input arrays of both entry points, laid out in one upload region
struct PairArrays {
  size_t o_pc, o_pm, o_uc, o_um, o_wc, o_wm;
  void take(ScratchLayout& L, size_t N) {
    o_pc = L.take<float>(N * 3), o_pm = L.take<float>(N * 3), o_uc = L.take<float>(N * 2), o_um = L.take<float>(N * 2);
    o_wc = L.take<double>(N), o_wm = L.take<double>(N);
  }
  void put(StagedIo& io, size_t N, const float* pc, const float* pm, const float* uv_c, const float* uv_m, const double* info_c,
           const double* info_m) const {
    io.put(o_pc, pc, N * 12);
    io.put(o_pm, pm, N * 12);
    io.put(o_uc, uv_c, N * 8);
    io.put(o_um, uv_m, N * 8);
    io.put(o_wc, info_c, N * 8);
    io.put(o_wm, info_m, N * 8);
  }
};

}  // namespace

extern "C" {

orbfe_status orbfe_sim3_optimize(orbfe_ctx* c, int32_t n, const float* pc, const float* pm, const float* uv_c, const float* uv_m,
                                 const double* info_c, const double* info_m, float fx, float fy, float cx, float cy, float* model,
                                 uint8_t* inlier_out, int32_t* n_inliers, double* est_out) {
  ApiLock api_lk(c);
  if (!c || n < 0 || n > ORBFE_BOW_MAX_FEATURES || !model || !n_inliers || (n && (!pc || !pm || !uv_c || !uv_m || !info_c || !info_m || !inlier_out)))
    return fail(c, ORBFE_EBADARG, "sim3_optimize: bad argument (n = %d of 0 .. %d)", n, ORBFE_BOW_MAX_FEATURES);
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(model[k])) return fail(c, ORBFE_EBADARG, "sim3_optimize: model[%d] is not finite", k);
  const size_t N = (size_t)n;
  *n_inliers = 0;
  Sim3Dev est0;
  sim3_from_model(model, est0);
  auto early = [&] {  // Optimizer.cc:584: return 0, the model and the match list untouched
    if (N) std::memset(inlier_out, 1, N);
    if (est_out) {
      std::memcpy(est_out, est0.q, 32);
      std::memcpy(est_out + 4, est0.t, 24);
      est_out[7] = est0.s;
    }
    return ORBFE_OK;
  };
  if (n < SIM3_MIN_PAIRS) return early();  // (O7: nothing observable happens)
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const bool mem = n > sim3_optimize_register_capacity();
  ScratchLayout L;
  ScratchRegion up, down;
  PairArrays A;
  L.open(up);
  A.take(L, N);
  const size_t o_mi = L.take<float>(12), o_ret = L.close(up).open(down).take<int32_t>(2), o_mo = L.take<float>(12), o_est = L.take<double>(8),
               o_in = L.take(N), o_e = L.close(down).take<double>(mem ? N * 4 : 1), o_act = L.take(mem ? N : 1);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes())));
  A.put(io, N, pc, pm, uv_c, uv_m, info_c, info_m);
  io.put(o_mi, model, 48);
  HIP_TRY(c, io.upload(up));
  const BaParamsDev prm = {(double)fx, (double)fy, (double)cx, (double)cy, 0.0};
  {
    StageTimer tm(c, ORBFE_STAGE_BA, c->stream);
    launch_sim3_optimize(c->stream, n, io.dev<float>(A.o_pc), io.dev<float>(A.o_pm), io.dev<float>(A.o_uc), io.dev<float>(A.o_um),
                         io.dev<double>(A.o_wc), io.dev<double>(A.o_wm), io.dev<float>(o_mi), prm, (double)(float)std::sqrt(9.210),
                         io.dev<double>(o_e), io.dev<uint8_t>(o_act), io.dev<float>(o_mo), io.dev<uint8_t>(o_in), io.dev<int32_t>(o_ret),
                         io.dev<double>(o_est));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down));
  drain_timers(c);
  int32_t ret[2];
  io.get(ret, o_ret, 8);
  if (!ret[1]) return early();
  *n_inliers = ret[0];
  io.get(model, o_mo, 48);
  io.get(inlier_out, o_in, N);
  io.get(est_out, o_est, 64);
  return ORBFE_OK;
}

orbfe_status orbfe_debug_sim3_edges(orbfe_ctx* c, int32_t n, const float* pc, const float* pm, const float* uv_c, const float* uv_m,
                                    const double* info_c, const double* info_m, float fx, float fy, float cx, float cy, const double* est,
                                    double* err, double* chi2, double* jac) {
  ApiLock api_lk(c);
  if (!c || n < 0 || n > ORBFE_BOW_MAX_FEATURES || !est || (n && (!pc || !pm || !uv_c || !uv_m || !info_c || !info_m || !err || !chi2 || !jac)))
    return fail(c, ORBFE_EBADARG, "debug_sim3_edges: bad argument");
  if (n == 0) return ORBFE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t N = (size_t)n;
  ScratchLayout L;
  ScratchRegion up, down;
  PairArrays A;
  L.open(up);
  A.take(L, N);
  const size_t o_est = L.take<double>(8), o_err = L.close(up).open(down).take<double>(N * 4), o_chi = L.take<double>(N * 2),
               o_jac = L.take<double>(N * 24);
  L.close(down);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes())));
  A.put(io, N, pc, pm, uv_c, uv_m, info_c, info_m);
  io.put(o_est, est, 64);
  HIP_TRY(c, io.upload(up));
  const BaParamsDev prm = {(double)fx, (double)fy, (double)cx, (double)cy, 0.0};
  launch_debug_sim3_edges(c->stream, n, io.dev<float>(A.o_pc), io.dev<float>(A.o_pm), io.dev<float>(A.o_uc), io.dev<float>(A.o_um),
                          io.dev<double>(A.o_wc), io.dev<double>(A.o_wm), prm, io.dev<double>(o_est), io.dev<double>(o_err),
                          io.dev<double>(o_chi), io.dev<double>(o_jac));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down));
  io.get(err, o_err, N * 32);
  io.get(chi2, o_chi, N * 16);
  io.get(jac, o_jac, N * 192);
  return ORBFE_OK;
}

}  // extern "C"
