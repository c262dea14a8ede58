// orbfe_pnp.hip -- host side of the EPnP RANSAC sets (include/orbfe.h): what PnPSolver adds to Ransac<PnPRet> -- the thresholds, the
// entry pose as a hypothesis to count, the calls' list scratch, the launch of Phase A + B.  The set, the speculated schedule and the exact
// replay of every iterate call are ransac_host.h's and ransac_replay.h's, shared with orbfe_sim3.hip.  The kernels: k_pnp.hip.
#include "orbfe_ctx.h"
#include "ransac_host.h"

void launch_pnp(hipStream_t st, const PnpHyp* hyps, int n_hyp, const PnpCall* calls, int n_calls, const RansacProb* probs, const float* xyz,
                const float* uv, const float* thr, const float cam[4], const int* entry, PnpOut* out, uint64_t* masks, uint64_t* ref_masks,
                int* lists);

namespace {

struct PnpTraits : ransac::NoHooks {
  using Policy = ransac::PnpPolicy;
  using Hyp = PnpHyp;
  using Out = PnpOut;
  static ransac::HypView view(const PnpOut& o, const uint64_t* mask, const uint64_t* ref_mask) {
    return {o.degen != 0, o.pose, mask, o.count, o.refined && !o.err, o.ref_pose, ref_mask, o.ref_count};
  }
  // one speculation's calls: the first one carries the caller's entry pose (a "given" hypothesis, P2) and entry list (P1)
  struct Plan {
    const float* pose;
    bool has_pose;
    const int32_t* entry;
    int64_t entry_len, list_total = 0;
    std::vector<PnpCall> calls;
    size_t o_calls = 0, o_entry = 0;
    Plan(const float* m, bool has, const int32_t* e, int64_t ne) : pose(m), has_pose(has), entry(e), entry_len(ne) {}
    int32_t open_call(std::vector<PnpHyp>& hyps, const ransac::Prob& pr, int32_t q, bool first, int32_t k) {
      PnpCall c{q, 0, k, -1, 0, first ? (int32_t)entry_len : 0, list_total, 0};
      if (first && has_pose && pr.n >= Policy::kMinSet) {
        PnpHyp h{};
        h.prob = q;
        h.given = 1;
        std::memcpy(h.pose, pose, sizeof h.pose);
        c.entry_hyp = (int32_t)hyps.size();
        hyps.push_back(h);
      }
      c.h0 = (int32_t)hyps.size();
      c.list_cap = c.entry_len + (int64_t)(k + 1) * pr.n;
      list_total += c.list_cap;
      calls.push_back(c);
      return c.entry_hyp;
    }
    size_t take(ScratchLayout& L) {  // uploaded behind the hypotheses: calls | entry list;  device only: the calls' list scratch
      o_calls = L.take<PnpCall>(calls.size()), o_entry = L.take<int32_t>((size_t)entry_len);
      return (size_t)list_total * sizeof(int32_t);
    }
    void put(StagedIo& io) const {
      io.put(o_calls, calls.data(), calls.size() * sizeof(PnpCall));
      io.put(o_entry, entry, (size_t)entry_len * 4);
    }
    void launch(ransac::Set<PnpTraits>& s, StagedIo& io, size_t o_h, int nh, size_t o_out, size_t o_m, size_t o_rm, size_t o_lists) const {
      launch_pnp(s.stream, io.dev<PnpHyp>(o_h), nh, io.dev<PnpCall>(o_calls), (int)calls.size(), s.d_probs, s.d_pts[0], s.d_pts[1], s.d_pts[2],
                 s.cam, io.dev<int>(o_entry), io.dev<PnpOut>(o_out), io.dev<uint64_t>(o_m), io.dev<uint64_t>(o_rm), io.dev<int>(o_lists));
    }
  };
};

}  // namespace

struct orbfe_pnp : ransac::Set<PnpTraits> {};  // d_pts: xyz, uv, mvfErrors

extern "C" {

orbfe_status orbfe_pnp_create(int32_t device_id, int32_t n_problems, const int64_t* offsets, const float* xyz, const float* uv,
                              const int32_t* octave, const float* level_sigma2, int32_t n_levels, const orbfe_camera* cam,
                              const orbfe_pnp_params* params, orbfe_pnp** out) {
  const char* who = "orbfe_pnp_create";
  if (!out || n_problems < 0 || !offsets || !cam || (n_levels > 0 && !level_sigma2) || n_levels < 0)
    return fail(nullptr, ORBFE_EBADARG, "%s: bad arguments", who);
  *out = nullptr;
  const orbfe_pnp_params prm = params ? *params : orbfe_pnp_params{4, 100, 0.4f, 0.99f};
  if (prm.min_set != 4) return fail(nullptr, ORBFE_EBADARG, "%s: min_set %d (EPnP samples 4 points)", who, prm.min_set);
  TRY(orbfe_pnp::check_create(who, "points", ORBFE_PNP_MAX_POINTS, 0x3FFFFFFF, device_id, n_problems, offsets, xyz && uv && octave, {octave},
                              n_levels));
  // mvfErrors: (float)(5.991 * Frame::getScaledFactor2(octave))
  std::vector<float> thr((size_t)offsets[n_problems]);
  for (size_t i = 0; i < thr.size(); ++i) thr[i] = (float)(5.991 * (double)level_sigma2[octave[i]]);
  std::unique_ptr<orbfe_pnp> s(new (std::nothrow) orbfe_pnp());
  if (!s) return fail(nullptr, ORBFE_ENOMEM, "%s: out of memory", who);
  const float* const pts[3] = {xyz, uv, thr.data()};
  const int width[3] = {3, 2, 1};
  TRY(s->open(who, "points", device_id, *cam, n_problems, offsets, prm.max_iterations, prm.ratio, prm.prob, pts, width));
  *out = s.release();
  return ORBFE_OK;
}

void orbfe_pnp_destroy(orbfe_pnp* s) { delete s; }

orbfe_status orbfe_pnp_iterate(orbfe_pnp* s, int32_t problem, int32_t n_iterations, float* pose, int32_t* has_pose, int32_t* inliers,
                               int64_t* n_inliers, int64_t cap, int32_t* ret, int32_t* no_more) {
  const char* who = "orbfe_pnp_iterate";
  if (!s || !pose || !has_pose || !n_inliers || !ret || !no_more || cap < 0 || *n_inliers < 0 || *n_inliers > cap || (cap > 0 && !inliers))
    return fail(nullptr, ORBFE_EBADARG, "%s: bad arguments", who);
  if (problem < 0 || problem >= (int32_t)s->probs.size()) return fail(nullptr, ORBFE_EBADARG, "%s: problem %d of %zu", who, problem, s->probs.size());
  std::lock_guard<std::mutex> lk(orbfe_pnp::mu);
  const int32_t n_points = s->probs[(size_t)problem].n;
  for (int64_t i = 0; i < *n_inliers; ++i)
    if (inliers[i] < 0 || inliers[i] >= n_points) return fail(nullptr, ORBFE_EBADARG, "%s: inlier %d of %d points", who, inliers[i], n_points);
  return s->iterate(who, problem, n_iterations, pose, has_pose, inliers, n_inliers, cap, ret, no_more);
}

orbfe_status orbfe_pnp_engine(uint32_t* get, const uint32_t* set) { return orbfe_pnp::engine_access("orbfe_pnp_engine", get, set); }

orbfe_status orbfe_pnp_stats(orbfe_pnp* s, int64_t* launches, int64_t* hypotheses) {
  return orbfe_pnp::stats("orbfe_pnp_stats", s, launches, hypotheses);
}

}  // extern "C"
