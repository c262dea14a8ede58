// orbfe_pnp.hip -- host side of the EPnP RANSAC sets (include/orbfe.h): setRansacParams, the process-wide sampling engine, the speculated
// schedule (one upload, two launches, one download) and the exact replay of every Ransac<PnPRet>::iterate call from its records.
// The kernels: k_pnp.hip.
#include "orbfe_ctx.h"
#include "ransac_host.h"

void launch_pnp(hipStream_t st, const PnpHyp* hyps, int n_hyp, const PnpCall* calls, int n_calls, const PnpProb* probs, const float* xyz,
                const float* uv, const float* thr, const float cam[4], const int* entry, PnpOut* out, uint64_t* masks, uint64_t* ref_masks,
                int* lists);

namespace {

// Ransac<PnPRet>'s function-local static std::default_random_engine (P6): one per process, shared by every set, behind one lock that
// also serialises every set's iterate.
std::mutex g_pnp_mu;
uint32_t g_engine = 1;

struct Prob {
  int32_t off = 0, n = 0, words = 0, min_inlier = 0, max_it = 0;
  int32_t cur = 0, best = 0;
  bool called = false;
  float best_pose[12] = {};
  std::vector<int32_t> best_list;
};

// what one speculated call found: its hypotheses [h0, h0 + nh) of the download, the engine before it and after each hypothesis
struct CallRec {
  int32_t prob, n, h0, nh, entry_hyp;
  uint32_t engine_start;
  std::vector<uint32_t> after;
};

}  // namespace

struct orbfe_pnp {
  int device = 0;
  hipStream_t stream = nullptr;
  float cam[4] = {};
  std::vector<Prob> probs;
  // device: the problems' points, thresholds and records
  float *d_xyz = nullptr, *d_uv = nullptr, *d_thr = nullptr;
  PnpProb* d_probs = nullptr;
  ransac::Io io;  // a speculation's upload, results and list scratch, and its page-locked staging
  // the speculation being replayed
  std::vector<CallRec> recs;
  size_t next = 0;
  std::vector<PnpHyp> hyps;
  std::vector<PnpOut> out;
  std::vector<uint64_t> masks, ref_masks;
  int64_t launches = 0, hypotheses = 0;
};

namespace {

bool alive(const Prob& p, int32_t cur, bool called) { return ransac::alive(p.n, 4, cur, p.max_it, called); }

constexpr size_t kMaxHyps = 1 << 17;  // one speculation covers at most this many hypotheses (the rest: a later one)

// Speculate from the call (p, n, entry state): the schedule Tracking will most likely run -- round-robin over the live problems,
// ascending, n each, no refine success -- its samples drawn from a copy of the engine, then one upload, Phase A + B, one download.
orbfe_status speculate(orbfe_pnp* s, int32_t p, int32_t n, const float* pose, bool has_pose, const int32_t* entry, int64_t entry_len) {
  s->recs.clear();
  s->next = 0;
  s->hyps.clear();
  const int P = (int)s->probs.size();
  std::vector<int32_t> cur(P);
  std::vector<char> called(P);
  for (int q = 0; q < P; ++q) {
    cur[q] = s->probs[q].cur;
    called[q] = s->probs[q].called;
  }
  uint32_t eng = g_engine;
  std::vector<PnpCall> calls;
  int64_t list_total = 0;
  auto add_call = [&](int32_t q, bool first) {
    const Prob& pr = s->probs[q];
    CallRec r{q, n, 0, 0, -1, eng, {}};
    PnpCall c{q, 0, 0, -1, 0, 0, 0, 0};
    if (first && has_pose && pr.n >= 4) {
      PnpHyp h{};
      h.prob = q;
      h.given = 1;
      std::memcpy(h.pose, pose, sizeof h.pose);
      r.entry_hyp = c.entry_hyp = (int32_t)s->hyps.size();
      s->hyps.push_back(h);
    }
    r.h0 = c.h0 = (int32_t)s->hyps.size();
    const int32_t k = pr.n >= 4 ? std::max(0, std::min(n, pr.max_it - cur[q])) : 0;
    for (int32_t i = 0; i < k; ++i) {
      PnpHyp h{};
      h.prob = q;
      ransac::random_sample(eng, (uint32_t)pr.n, 4, h.idx);
      r.after.push_back(eng);
      s->hyps.push_back(h);
    }
    r.nh = c.nh = k;
    c.entry_off = 0;
    c.entry_len = first ? (int32_t)entry_len : 0;
    c.list_off = list_total;
    c.list_cap = c.entry_len + (int64_t)(k + 1) * pr.n;
    list_total += c.list_cap;
    cur[q] += k;
    called[q] = 1;
    s->recs.push_back(std::move(r));
    calls.push_back(c);
  };
  ransac::round_robin(
      P, p, [&](int q) { return alive(s->probs[q], cur[q], called[q]); }, add_call, [&] { return s->hyps.size() >= kMaxHyps; });
  // mask offsets
  int64_t words = 0;
  for (PnpHyp& h : s->hyps) {
    h.mask_off = (int32_t)words;
    words += s->probs[h.prob].words;
  }
  if (words > 0x7FFFFFFF) return fail(nullptr, ORBFE_ECAPACITY, "pnp_iterate: speculation too large");
  const size_t nh = s->hyps.size(), nc = calls.size();
  // upload: hyps | calls | entry list;  download: out | masks | refine masks;  device only: list scratch
  ScratchLayout L;
  ScratchRegion up, down;
  const size_t o_h = L.open(up).take<PnpHyp>(nh), o_c = L.take<PnpCall>(nc), o_e = L.take<int32_t>((size_t)entry_len),
               o_out = L.close(up).open(down).take<PnpOut>(nh), o_m = L.take<uint64_t>((size_t)words), o_rm = L.take<uint64_t>((size_t)words),
               o_l = L.close(down).take<int32_t>((size_t)list_total);
  HIP_TRY(nullptr, hipSetDevice(s->device));  // before the block is (re)allocated: it belongs to the set's device
  TRY(ransac::io_reserve(&s->io, L.end(), down.end));
  StagedIo io(s->io.d_io, s->io.h_io, s->stream);
  io.put(o_h, s->hyps.data(), nh * sizeof(PnpHyp));
  io.put(o_c, calls.data(), nc * sizeof(PnpCall));
  io.put(o_e, entry, (size_t)entry_len * 4);
  HIP_TRY(nullptr, io.upload(up));
  launch_pnp(s->stream, io.dev<PnpHyp>(o_h), (int)nh, io.dev<PnpCall>(o_c), (int)nc, s->d_probs, s->d_xyz, s->d_uv, s->d_thr, s->cam,
             io.dev<int>(o_e), io.dev<PnpOut>(o_out), io.dev<uint64_t>(o_m), io.dev<uint64_t>(o_rm), io.dev<int>(o_l));
  HIP_TRY(nullptr, hipGetLastError());
  HIP_TRY(nullptr, io.fetch(down, down.begin));
  s->out.resize(nh);
  s->masks.resize((size_t)words);
  s->ref_masks.resize((size_t)words);
  io.get(s->out.data(), o_out, nh * sizeof(PnpOut));
  io.get(s->masks.data(), o_m, (size_t)words * 8);
  io.get(s->ref_masks.data(), o_rm, (size_t)words * 8);
  s->launches += 1;
  s->hypotheses += (int64_t)nh;
  return ORBFE_OK;
}

using ransac::append_bits;

}  // namespace

extern "C" {

orbfe_status orbfe_pnp_create(int32_t device_id, int32_t n_problems, const int64_t* offsets, const float* xyz, const float* uv,
                              const int32_t* octave, const float* level_sigma2, int32_t n_levels, const orbfe_camera* cam,
                              const orbfe_pnp_params* params, orbfe_pnp** out) {
  if (!out || n_problems < 0 || !offsets || !cam || (n_levels > 0 && !level_sigma2) || n_levels < 0)
    return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_create: bad arguments");
  *out = nullptr;
  const orbfe_pnp_params prm = params ? *params : orbfe_pnp_params{4, 100, 0.4f, 0.99f};
  if (prm.min_set != 4) return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_create: min_set %d (EPnP samples 4 points)", prm.min_set);
  if (offsets[0] != 0) return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_create: offsets[0] must be 0");
  for (int32_t i = 0; i < n_problems; ++i)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > ORBFE_PNP_MAX_POINTS)
      return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_create: problem %d has %lld points (0 .. %d)", i, (long long)(offsets[i + 1] - offsets[i]),
                  ORBFE_PNP_MAX_POINTS);
  const int64_t total = offsets[n_problems];
  if (total > 0x3FFFFFFF) return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_create: %lld points in all", (long long)total);
  if (total > 0 && (!xyz || !uv || !octave)) return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_create: NULL points");
  for (int64_t i = 0; i < total; ++i)
    if (octave[i] < 0 || octave[i] >= n_levels)
      return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_create: point %lld has octave %d of %d levels", (long long)i, octave[i], n_levels);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, ORBFE_EDEVICE, "orbfe_pnp_create: no HIP device (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_create: device %d of %d", device_id, ndev);
  std::unique_ptr<orbfe_pnp> s(new (std::nothrow) orbfe_pnp());
  if (!s) return fail(nullptr, ORBFE_ENOMEM, "orbfe_pnp_create: out of memory");
  s->device = device_id;
  s->cam[0] = cam->fx;
  s->cam[1] = cam->fy;
  s->cam[2] = cam->cx;
  s->cam[3] = cam->cy;
  s->probs.resize((size_t)n_problems);
  std::vector<PnpProb> dp((size_t)n_problems);
  for (int32_t i = 0; i < n_problems; ++i) {
    Prob& p = s->probs[(size_t)i];
    p.off = (int32_t)offsets[i];
    p.n = (int32_t)(offsets[i + 1] - offsets[i]);
    p.words = (p.n + 63) / 64;
    ransac::ransac_params(p.n, prm.min_set, prm.max_iterations, prm.ratio, prm.prob, &p.min_inlier, &p.max_it);
    dp[(size_t)i] = PnpProb{p.off, p.n, p.words, p.min_inlier};
  }
  // mvfErrors: (float)(5.991 * Frame::getScaledFactor2(octave))
  std::vector<float> thr((size_t)total);
  for (int64_t i = 0; i < total; ++i) thr[(size_t)i] = (float)(5.991 * (double)level_sigma2[octave[i]]);
  int cur = -1;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  orbfe_status st = ORBFE_OK;
  const size_t nb = (size_t)std::max<int64_t>(total, 1);
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess)
    st = fail(nullptr, ORBFE_EDEVICE, "orbfe_pnp_create: cannot create a stream on device %d", device_id);
  else if (hipMalloc((void**)&s->d_xyz, nb * 12) != hipSuccess || hipMalloc((void**)&s->d_uv, nb * 8) != hipSuccess ||
           hipMalloc((void**)&s->d_thr, nb * 4) != hipSuccess ||
           hipMalloc((void**)&s->d_probs, std::max<size_t>(dp.size(), 1) * sizeof(PnpProb)) != hipSuccess)
    st = fail(nullptr, ORBFE_ENOMEM, "orbfe_pnp_create: cannot allocate %lld points on device %d", (long long)total, device_id);
  else if ((total && (hipMemcpy(s->d_xyz, xyz, (size_t)total * 12, hipMemcpyHostToDevice) != hipSuccess ||
                      hipMemcpy(s->d_uv, uv, (size_t)total * 8, hipMemcpyHostToDevice) != hipSuccess ||
                      hipMemcpy(s->d_thr, thr.data(), (size_t)total * 4, hipMemcpyHostToDevice) != hipSuccess)) ||
           (!dp.empty() && hipMemcpy(s->d_probs, dp.data(), dp.size() * sizeof(PnpProb), hipMemcpyHostToDevice) != hipSuccess))
    st = fail(nullptr, ORBFE_EDEVICE, "orbfe_pnp_create: upload failed");
  if (have_cur) (void)hipSetDevice(cur);
  if (st != ORBFE_OK) {
    orbfe_pnp_destroy(s.release());
    return st;
  }
  *out = s.release();
  return ORBFE_OK;
}

void orbfe_pnp_destroy(orbfe_pnp* s) {
  if (!s) return;
  int cur = -1;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  (void)hipSetDevice(s->device);
  for (void* p : {(void*)s->d_xyz, (void*)s->d_uv, (void*)s->d_thr, (void*)s->d_probs})
    if (p) (void)hipFree(p);
  ransac::io_release(&s->io);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  if (have_cur) (void)hipSetDevice(cur);
  delete s;
}

orbfe_status orbfe_pnp_iterate(orbfe_pnp* s, int32_t problem, int32_t n_iterations, float* pose, int32_t* has_pose, int32_t* inliers,
                               int64_t* n_inliers, int64_t cap, int32_t* ret, int32_t* no_more) {
  if (!s || !pose || !has_pose || !n_inliers || !ret || !no_more || cap < 0 || *n_inliers < 0 || *n_inliers > cap || (cap > 0 && !inliers))
    return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_iterate: bad arguments");
  if (problem < 0 || problem >= (int32_t)s->probs.size())
    return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_iterate: problem %d of %zu", problem, s->probs.size());
  std::lock_guard<std::mutex> lk(g_pnp_mu);
  Prob& pr = s->probs[(size_t)problem];
  for (int64_t i = 0; i < *n_inliers; ++i)
    if (inliers[i] < 0 || inliers[i] >= pr.n) return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_iterate: inlier %d of %d points", inliers[i], pr.n);
  *ret = 0;
  const bool entry_empty = !*has_pose && *n_inliers == 0;
  const int32_t k = pr.n >= 4 ? std::max(0, std::min(n_iterations, pr.max_it - pr.cur)) : 0;
  // the next record serves this call if the call is the predicted one: same problem and n, empty entry state, engine untouched
  bool hit = s->next > 0 && s->next < s->recs.size() && entry_empty;
  if (hit) {
    const CallRec& r = s->recs[s->next];
    hit = r.prob == problem && r.n == n_iterations && r.engine_start == g_engine && r.nh == k;
  }
  if (pr.n < 4) {  // P5
    if (hit) {
      s->next += 1;
    } else {
      s->recs.clear();
      s->next = 0;
    }
    pr.called = true;
    *no_more = 1;
    return ORBFE_OK;
  }
  CallRec r;
  if (hit) {
    r = s->recs[s->next];
    s->next += 1;
  } else if (k == 0) {  // the budget is spent: nothing for the device
    s->recs.clear();
    s->next = 0;
    r = CallRec{problem, n_iterations, 0, 0, -1, g_engine, {}};
  } else {
    int cur = -1;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    const orbfe_status st = speculate(s, problem, n_iterations, pose, *has_pose != 0, inliers, *n_inliers);
    if (have_cur) (void)hipSetDevice(cur);
    if (st != ORBFE_OK) {
      s->recs.clear();
      s->next = 0;
      return st;
    }
    r = s->recs[0];
    s->next = 1;
  }
  if (r.nh != k || r.prob != problem) {
    s->recs.clear();
    s->next = 0;
    return fail(nullptr, ORBFE_EDEVICE, "orbfe_pnp_iterate: inconsistent speculation");
  }
  // replay Ransac::iterate from the records on copies, committed when the result fits
  std::vector<int32_t> list(inliers, inliers + *n_inliers);
  float cur_pose[12];
  std::memcpy(cur_pose, pose, sizeof cur_pose);
  bool has = *has_pose != 0;
  int32_t cur = pr.cur, best = pr.best;
  bool best_changed = false;
  float best_pose[12];
  std::vector<int32_t> best_list;
  const uint64_t* st_mask = nullptr;
  int32_t st_cnt = 0;
  if (r.entry_hyp >= 0) {
    st_mask = s->masks.data() + s->hyps[(size_t)r.entry_hyp].mask_off;
    st_cnt = s->out[(size_t)r.entry_hyp].count;
  }
  bool success = false;
  uint32_t eng = g_engine;
  for (int32_t i = 0; i < r.nh && !success; ++i) {
    const size_t h = (size_t)(r.h0 + i);
    const PnpOut& o = s->out[h];
    if (!o.degen) {
      std::memcpy(cur_pose, o.pose, sizeof cur_pose);
      has = true;
      st_mask = s->masks.data() + s->hyps[h].mask_off;
      st_cnt = o.count;
    }
    eng = r.after[(size_t)i];
    if (has) {
      if (!st_mask) return fail(nullptr, ORBFE_EDEVICE, "orbfe_pnp_iterate: no record of the entry pose");
      append_bits(st_mask, pr.words, list);
      if (st_cnt > pr.min_inlier) {
        if (st_cnt > best) {
          best = st_cnt;
          best_changed = true;
          std::memcpy(best_pose, cur_pose, sizeof best_pose);
          best_list = list;
        }
        if (!o.refined || o.err) {
          s->recs.clear();
          return fail(nullptr, ORBFE_EDEVICE, "orbfe_pnp_iterate: refine record missing");
        }
        std::memcpy(cur_pose, o.ref_pose, sizeof cur_pose);
        st_mask = s->ref_masks.data() + s->hyps[h].mask_off;
        st_cnt = o.ref_count;
        list.clear();
        append_bits(st_mask, pr.words, list);
        if (st_cnt > pr.min_inlier) {
          success = true;  // P3: the budget is not spent
          break;
        }
      }
    }
    ++cur;
  }
  bool set_no_more = false;
  const std::vector<int32_t>* res = &list;
  const float* res_pose = cur_pose;
  bool res_has = has;
  if (success) {
    *ret = 1;
  } else {
    set_no_more = cur >= pr.max_it;
    const int32_t b = best_changed ? best : pr.best;
    if (b > 0) {
      *ret = 1;
      res = best_changed ? &best_list : &pr.best_list;
      res_pose = best_changed ? best_pose : pr.best_pose;
      res_has = true;
    }
  }
  if ((int64_t)res->size() > cap) {
    *n_inliers = (int64_t)res->size();
    *ret = 0;
    s->recs.clear();
    s->next = 0;
    return fail(nullptr, ORBFE_ECAPACITY, "orbfe_pnp_iterate: %zu inliers, room for %lld", res->size(), (long long)cap);
  }
  // commit
  std::copy(res->begin(), res->end(), inliers);
  *n_inliers = (int64_t)res->size();
  std::memcpy(pose, res_pose, 12 * sizeof(float));
  *has_pose = res_has ? 1 : 0;
  if (set_no_more) *no_more = 1;
  pr.cur = cur;
  pr.called = true;
  if (best_changed) {
    pr.best = best;
    std::memcpy(pr.best_pose, best_pose, sizeof best_pose);
    pr.best_list = std::move(best_list);
  }
  g_engine = eng;
  if (success) {
    s->recs.clear();
    s->next = 0;
  }
  return ORBFE_OK;
}

orbfe_status orbfe_pnp_engine(uint32_t* get, const uint32_t* set) {
  return ransac::engine_access(g_pnp_mu, g_engine, get, set, "orbfe_pnp_engine");
}

orbfe_status orbfe_pnp_stats(orbfe_pnp* s, int64_t* launches, int64_t* hypotheses) {
  if (!s) return fail(nullptr, ORBFE_EBADARG, "orbfe_pnp_stats: NULL set");
  std::lock_guard<std::mutex> lk(g_pnp_mu);
  if (launches) *launches = s->launches;
  if (hypotheses) *hypotheses = s->hypotheses;
  return ORBFE_OK;
}

}  // extern "C"
