// orbfe_sim3.hip -- host side of the Sim3 RANSAC sets (include/orbfe.h): what Sim3Solver adds to Ransac<Sim3Ret> -- its constructor (the
// camera-frame points, their projections, the thresholds), the one launch, and the optional events around it.  The set, the speculated
// schedule and the exact replay of every iterate call are ransac_host.h's and ransac_replay.h's, shared with orbfe_pnp.hip.  The kernel:
// k_sim3.hip.
#include "orbfe_ctx.h"
#include "ransac_host.h"

void launch_sim3(hipStream_t st, const Sim3Hyp* hyps, int n_hyp, const RansacProb* probs, const float* pq, const float* px, const float* thr,
                 const float cam[4], Sim3Out* out, uint64_t* masks, uint64_t* ref_masks);

namespace {

struct Sim3Traits {
  using Policy = ransac::Sim3Policy;
  using Hyp = Sim3Hyp;
  using Out = Sim3Out;
  using Set = ransac::Set<Sim3Traits>;
  static ransac::HypView view(const Sim3Out& o, const uint64_t* mask, const uint64_t* ref_mask) {
    return {false, o.model, mask, o.count, o.refined != 0, o.ref_model, ref_mask, o.ref_count};
  }
  struct Plan {  // a call is its hypotheses and nothing else: the entry model and list are not read (S2)
    Plan(const float*, bool, const int32_t*, int64_t) {}
    int32_t open_call(std::vector<Sim3Hyp>&, const ransac::Prob&, int32_t, bool, int32_t) { return -1; }
    size_t take(ScratchLayout&) { return 0; }
    void put(StagedIo&) const {}
    void launch(Set& s, StagedIo& io, size_t o_h, int nh, size_t o_out, size_t o_m, size_t o_rm, size_t) const {
      launch_sim3(s.stream, io.dev<Sim3Hyp>(o_h), nh, s.d_probs, s.d_pts[0], s.d_pts[1], s.d_pts[2], s.cam, io.dev<Sim3Out>(o_out),
                  io.dev<uint64_t>(o_m), io.dev<uint64_t>(o_rm));
    }
  };
  static orbfe_status before_launch(Set& s, size_t up_bytes);
  static orbfe_status after_launch(Set& s);
};

}  // namespace

// d_pts: per correspondence (P3d, Q3d), (P2d, Q2d), (mvfErrorsP, mvfErrorsQ)
struct orbfe_sim3 : ransac::Set<Sim3Traits> {
  int64_t bytes_uploaded = 0;  // create's arrays and every speculation's upload
  bool profile = false;        // orbfe_sim3_profile: events around every launch from then on
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool ev_pending = false;     // ev0 and ev1 hold a launch not yet added to device_us
  double device_us = 0;
  void settle() {  // (every speculation ends with its download, so the events have completed)
    float ms = 0;
    if (ev_pending && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) device_us += (double)ms * 1e3;
    ev_pending = false;
  }
  ~orbfe_sim3() {
    DeviceScope dev(device);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

namespace {

orbfe_status Sim3Traits::before_launch(Set& set, size_t up_bytes) {
  orbfe_sim3& s = static_cast<orbfe_sim3&>(set);
  s.bytes_uploaded += (int64_t)up_bytes;
  s.settle();
  if (s.profile) HIP_TRY(nullptr, hipEventRecord(s.ev0, s.stream));
  return ORBFE_OK;
}
orbfe_status Sim3Traits::after_launch(Set& set) {
  orbfe_sim3& s = static_cast<orbfe_sim3&>(set);
  if (s.profile) HIP_TRY(nullptr, hipEventRecord(s.ev1, s.stream));
  s.ev_pending = s.profile;
  return ORBFE_OK;
}

// (float)((double)(r . x) + (double)t), the row sum in float left to right
inline float affine_row(const float* r, const float* x, float t) {
  const float s = (r[0] * x[0] + r[1] * x[1]) + r[2] * x[2];
  return (float)((double)s + (double)t);
}

}  // namespace

extern "C" {

orbfe_status orbfe_sim3_create(int32_t device_id, int32_t n_problems, const int64_t* offsets, const float* pos_p, const float* pos_q,
                               const int32_t* octave_p, const int32_t* octave_q, const float* pose_p, const float* pose_q,
                               const float* level_sigma2, int32_t n_levels, const orbfe_camera* cam, const orbfe_sim3_params* params,
                               orbfe_sim3** out) {
  const char* who = "orbfe_sim3_create";
  if (!out || n_problems < 0 || !offsets || !cam || (n_levels > 0 && !level_sigma2) || n_levels < 0 ||
      (n_problems > 0 && (!pose_p || !pose_q)))
    return fail(nullptr, ORBFE_EBADARG, "%s: bad arguments", who);
  *out = nullptr;
  const orbfe_sim3_params prm = params ? *params : orbfe_sim3_params{3, 100, 0.4f, 0.99f};
  if (prm.min_set != 3) return fail(nullptr, ORBFE_EBADARG, "%s: min_set %d (Sim3Solver::create samples 3 pairs)", who, prm.min_set);
  TRY(orbfe_sim3::check_create(who, "correspondences", ORBFE_BOW_MAX_FEATURES, 0x0FFFFFFF, device_id, n_problems, offsets,
                               pos_p && pos_q && octave_p && octave_q, {octave_p, octave_q}, n_levels));
  // Sim3Solver's constructor: p3d = Rpw * pos + tpw and q3d, Camera::project of both, mvfErrorsP / Q = (float)(9.210 * sigma2[octave])
  const size_t total = (size_t)offsets[n_problems];
  std::vector<float> pq(total * 6), px(total * 4), thr(total * 2);
  for (int32_t i = 0; i < n_problems; ++i) {
    const float *Tp = pose_p + 12 * (size_t)i, *Tq = pose_q + 12 * (size_t)i;
    for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
      float* c = &pq[(size_t)j * 6];
      for (int r = 0; r < 3; ++r) {
        c[r] = affine_row(Tp + 3 * r, pos_p + 3 * j, Tp[9 + r]);
        c[3 + r] = affine_row(Tq + 3 * r, pos_q + 3 * j, Tq[9 + r]);
      }
      float* x = &px[(size_t)j * 4];
      x[0] = cam->fx * (c[0] / c[2]) + cam->cx;
      x[1] = cam->fy * (c[1] / c[2]) + cam->cy;
      x[2] = cam->fx * (c[3] / c[5]) + cam->cx;
      x[3] = cam->fy * (c[4] / c[5]) + cam->cy;
      thr[(size_t)j * 2] = (float)(9.210 * (double)level_sigma2[octave_p[j]]);
      thr[(size_t)j * 2 + 1] = (float)(9.210 * (double)level_sigma2[octave_q[j]]);
    }
  }
  std::unique_ptr<orbfe_sim3> s(new (std::nothrow) orbfe_sim3());
  if (!s) return fail(nullptr, ORBFE_ENOMEM, "%s: out of memory", who);
  const float* const pts[3] = {pq.data(), px.data(), thr.data()};
  const int width[3] = {6, 4, 2};
  TRY(s->open(who, "correspondences", device_id, *cam, n_problems, offsets, prm.max_iterations, prm.ratio, prm.prob, pts, width));
  s->bytes_uploaded = (int64_t)(total * 48 + (size_t)n_problems * sizeof(RansacProb));
  *out = s.release();
  return ORBFE_OK;
}

void orbfe_sim3_destroy(orbfe_sim3* s) { delete s; }

orbfe_status orbfe_sim3_iterate(orbfe_sim3* s, int32_t problem, int32_t n_iterations, float* model, int32_t* has_model, int32_t* inliers,
                                int64_t* n_inliers, int64_t cap, int32_t* ret, int32_t* no_more) {
  const char* who = "orbfe_sim3_iterate";
  if (!s || !model || !has_model || !n_inliers || !ret || !no_more || cap < 0 || *n_inliers < 0 || *n_inliers > cap || (cap > 0 && !inliers))
    return fail(nullptr, ORBFE_EBADARG, "%s: bad arguments", who);
  if (problem < 0 || problem >= (int32_t)s->probs.size()) return fail(nullptr, ORBFE_EBADARG, "%s: problem %d of %zu", who, problem, s->probs.size());
  std::lock_guard<std::mutex> lk(orbfe_sim3::mu);
  return s->iterate(who, problem, n_iterations, model, has_model, inliers, n_inliers, cap, ret, no_more);
}

orbfe_status orbfe_sim3_engine(uint32_t* get, const uint32_t* set) { return orbfe_sim3::engine_access("orbfe_sim3_engine", get, set); }

orbfe_status orbfe_sim3_stats(orbfe_sim3* s, int64_t* launches, int64_t* hypotheses) {
  return orbfe_sim3::stats("orbfe_sim3_stats", s, launches, hypotheses);
}

orbfe_status orbfe_sim3_profile(orbfe_sim3* s, int32_t enable, double* device_us, int64_t* bytes_uploaded) {
  if (!s) return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_profile: NULL set");
  std::lock_guard<std::mutex> lk(orbfe_sim3::mu);
  if (enable > 0 && !s->ev0) {
    DeviceScope dev(s->device);
    if (dev.err != hipSuccess || hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess)
      return fail(nullptr, ORBFE_EDEVICE, "orbfe_sim3_profile: cannot create events on device %d", s->device);
  }
  s->settle();
  if (enable >= 0) s->profile = enable > 0;
  if (device_us) *device_us = s->device_us;
  if (bytes_uploaded) *bytes_uploaded = s->bytes_uploaded;
  return ORBFE_OK;
}

}  // extern "C"
