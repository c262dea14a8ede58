// orbfe_sim3.hip -- host side of the Sim3 RANSAC sets (include/orbfe.h): Sim3Solver's constructor (the camera-frame points, their
// projections, the thresholds, setRansacParams), Ransac<Sim3Ret>'s own sampling engine, the speculated schedule (one upload, one launch,
// one download) and the exact replay of every Ransac<Sim3Ret>::iterate call from its records.  The kernel: k_sim3.hip.  The engine
// arithmetic, the schedule and the io block are ransac_host.h's, shared with orbfe_pnp.hip.
#include "orbfe_ctx.h"
#include "ransac_host.h"

void launch_sim3(hipStream_t st, const Sim3Hyp* hyps, int n_hyp, const Sim3Prob* probs, const float* pq, const float* px, const float* thr,
                 const float cam[4], Sim3Out* out, uint64_t* masks, uint64_t* ref_masks);

namespace {

// Ransac<Sim3Ret>'s function-local static std::default_random_engine (S7): its own, apart from Ransac<PnPRet>'s, behind one lock that
// also serialises every Sim3 set's iterate.
std::mutex g_sim3_mu;
uint32_t g_engine = 1;

constexpr int kMinSet = 3;

struct Prob {
  int32_t off = 0, n = 0, words = 0, min_inlier = 0, max_it = 0;
  int32_t cur = 0, best = 0;
  bool called = false;
  bool skipped = false;  // the caller left it out where the schedule had it: speculations leave it out until it is called again
  float best_model[12] = {};
  std::vector<int32_t> best_list;
};

// what one speculated call found: its hypotheses [h0, h0 + nh) of the download, the engine before it and after each hypothesis
struct CallRec {
  int32_t prob, n, h0, nh;
  uint32_t engine_start;
  std::vector<uint32_t> after;
};

}  // namespace

struct orbfe_sim3 {
  int device = 0;
  hipStream_t stream = nullptr;
  float cam[4] = {};
  std::vector<Prob> probs;
  // device: per correspondence (P3d, Q3d), (P2d, Q2d), (mvfErrorsP, mvfErrorsQ); the problems' records
  float *d_pq = nullptr, *d_px = nullptr, *d_thr = nullptr;
  Sim3Prob* d_probs = nullptr;
  ransac::Io io;  // a speculation's upload and results, and its page-locked staging
  // the speculation being replayed
  std::vector<CallRec> recs;
  size_t next = 0;
  std::vector<Sim3Hyp> hyps;
  std::vector<Sim3Out> out;
  std::vector<uint64_t> masks, ref_masks;
  int64_t launches = 0, hypotheses = 0;
  int64_t bytes_uploaded = 0;               // create's arrays and every speculation's upload
  bool profile = false;                     // orbfe_sim3_profile: events around every launch from then on
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double device_us = 0;
};

namespace {

bool alive(const Prob& p, int32_t cur, bool called) { return ransac::alive(p.n, kMinSet, cur, p.max_it, called); }

constexpr size_t kMaxHyps = 1 << 17;  // one speculation covers at most this many hypotheses (the rest: a later one)

void drop_records(orbfe_sim3* s) {
  s->recs.clear();
  s->next = 0;
}

// Speculate from the call (p, n): the schedule LoopClosing::computeSim3 will most likely run -- round-robin over the live problems,
// ascending, n each, no refine success -- its samples drawn from a copy of the engine, then one upload, one launch, one download.
orbfe_status speculate(orbfe_sim3* s, int32_t p, int32_t n) {
  drop_records(s);
  s->hyps.clear();
  const int P = (int)s->probs.size();
  std::vector<int32_t> cur(P);
  std::vector<char> called(P);
  for (int q = 0; q < P; ++q) {
    cur[q] = s->probs[q].cur;
    called[q] = s->probs[q].called;
  }
  uint32_t eng = g_engine;
  int64_t words = 0;
  auto add_call = [&](int32_t q, bool) {
    const Prob& pr = s->probs[q];
    CallRec r{q, n, (int32_t)s->hyps.size(), 0, eng, {}};
    const int32_t k = pr.n >= kMinSet ? std::max(0, std::min(n, pr.max_it - cur[q])) : 0;
    for (int32_t i = 0; i < k; ++i) {
      Sim3Hyp h{};
      h.prob = q;
      h.mask_off = (int32_t)words;
      words += pr.words;
      ransac::random_sample(eng, (uint32_t)pr.n, kMinSet, h.idx);
      r.after.push_back(eng);
      s->hyps.push_back(h);
    }
    r.nh = k;
    cur[q] += k;
    called[q] = 1;
    s->recs.push_back(std::move(r));
  };
  ransac::round_robin(
      P, p, [&](int q) { return !s->probs[q].skipped && alive(s->probs[q], cur[q], called[q]); }, add_call,
      [&] { return s->hyps.size() >= kMaxHyps || words > 0x3FFFFFFF; });
  if (words > 0x7FFFFFFF) return fail(nullptr, ORBFE_ECAPACITY, "sim3_iterate: speculation too large");
  const size_t nh = s->hyps.size();
  // upload: hyps;  download: out | masks | refine masks
  ScratchLayout L;
  ScratchRegion up, down;
  const size_t o_h = L.open(up).take<Sim3Hyp>(nh), o_out = L.close(up).open(down).take<Sim3Out>(nh), o_m = L.take<uint64_t>((size_t)words),
               o_rm = L.take<uint64_t>((size_t)words);
  L.close(down);
  HIP_TRY(nullptr, hipSetDevice(s->device));  // before the block is (re)allocated: it belongs to the set's device
  TRY(ransac::io_reserve(&s->io, L.end(), down.end));
  StagedIo io(s->io.d_io, s->io.h_io, s->stream);
  io.put(o_h, s->hyps.data(), nh * sizeof(Sim3Hyp));
  HIP_TRY(nullptr, io.upload(up));
  s->bytes_uploaded += (int64_t)up.bytes();
  if (s->profile) HIP_TRY(nullptr, hipEventRecord(s->ev0, s->stream));
  launch_sim3(s->stream, io.dev<Sim3Hyp>(o_h), (int)nh, s->d_probs, s->d_pq, s->d_px, s->d_thr, s->cam, io.dev<Sim3Out>(o_out),
              io.dev<uint64_t>(o_m), io.dev<uint64_t>(o_rm));
  HIP_TRY(nullptr, hipGetLastError());
  if (s->profile) HIP_TRY(nullptr, hipEventRecord(s->ev1, s->stream));
  HIP_TRY(nullptr, io.fetch(down, down.begin));
  if (s->profile) {
    float ms = 0;
    HIP_TRY(nullptr, hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->device_us += (double)ms * 1e3;
  }
  s->out.resize(nh);
  s->masks.resize((size_t)words);
  s->ref_masks.resize((size_t)words);
  io.get(s->out.data(), o_out, nh * sizeof(Sim3Out));
  io.get(s->masks.data(), o_m, (size_t)words * 8);
  io.get(s->ref_masks.data(), o_rm, (size_t)words * 8);
  s->launches += 1;
  s->hypotheses += (int64_t)nh;
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
  if (!out || n_problems < 0 || !offsets || !cam || (n_levels > 0 && !level_sigma2) || n_levels < 0 ||
      (n_problems > 0 && (!pose_p || !pose_q)))
    return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_create: bad arguments");
  *out = nullptr;
  const orbfe_sim3_params prm = params ? *params : orbfe_sim3_params{kMinSet, 100, 0.4f, 0.99f};
  if (prm.min_set != kMinSet)
    return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_create: min_set %d (Sim3Solver::create samples 3 pairs)", prm.min_set);
  if (offsets[0] != 0) return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_create: offsets[0] must be 0");
  for (int32_t i = 0; i < n_problems; ++i)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > ORBFE_BOW_MAX_FEATURES)
      return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_create: problem %d has %lld correspondences (0 .. %d)", i,
                  (long long)(offsets[i + 1] - offsets[i]), ORBFE_BOW_MAX_FEATURES);
  const int64_t total = offsets[n_problems];
  if (total > 0x0FFFFFFF) return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_create: %lld correspondences in all", (long long)total);
  if (total > 0 && (!pos_p || !pos_q || !octave_p || !octave_q)) return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_create: NULL correspondences");
  for (int64_t i = 0; i < total; ++i)
    if (octave_p[i] < 0 || octave_p[i] >= n_levels || octave_q[i] < 0 || octave_q[i] >= n_levels)
      return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_create: correspondence %lld has octaves %d, %d of %d levels", (long long)i, octave_p[i],
                  octave_q[i], n_levels);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, ORBFE_EDEVICE, "orbfe_sim3_create: no HIP device (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_create: device %d of %d", device_id, ndev);
  std::unique_ptr<orbfe_sim3> s(new (std::nothrow) orbfe_sim3());
  if (!s) return fail(nullptr, ORBFE_ENOMEM, "orbfe_sim3_create: out of memory");
  s->device = device_id;
  s->cam[0] = cam->fx;
  s->cam[1] = cam->fy;
  s->cam[2] = cam->cx;
  s->cam[3] = cam->cy;
  s->probs.resize((size_t)n_problems);
  std::vector<Sim3Prob> dp((size_t)n_problems);
  // Sim3Solver's constructor: p3d = Rpw * pos + tpw and q3d, Camera::project of both, mvfErrorsP / Q = (float)(9.210 * sigma2[octave])
  std::vector<float> pq((size_t)total * 6), px((size_t)total * 4), thr((size_t)total * 2);
  for (int32_t i = 0; i < n_problems; ++i) {
    Prob& p = s->probs[(size_t)i];
    p.off = (int32_t)offsets[i];
    p.n = (int32_t)(offsets[i + 1] - offsets[i]);
    p.words = (p.n + 63) / 64;
    ransac::ransac_params(p.n, kMinSet, prm.max_iterations, prm.ratio, prm.prob, &p.min_inlier, &p.max_it);
    dp[(size_t)i] = Sim3Prob{p.off, p.n, p.words, p.min_inlier};
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
  int cur = -1;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  orbfe_status st = ORBFE_OK;
  const size_t nb = (size_t)std::max<int64_t>(total, 1);
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess)
    st = fail(nullptr, ORBFE_EDEVICE, "orbfe_sim3_create: cannot create a stream on device %d", device_id);
  else if (hipMalloc((void**)&s->d_pq, nb * 24) != hipSuccess || hipMalloc((void**)&s->d_px, nb * 16) != hipSuccess ||
           hipMalloc((void**)&s->d_thr, nb * 8) != hipSuccess ||
           hipMalloc((void**)&s->d_probs, std::max<size_t>(dp.size(), 1) * sizeof(Sim3Prob)) != hipSuccess)
    st = fail(nullptr, ORBFE_ENOMEM, "orbfe_sim3_create: cannot allocate %lld correspondences on device %d", (long long)total, device_id);
  else if ((total && (hipMemcpy(s->d_pq, pq.data(), (size_t)total * 24, hipMemcpyHostToDevice) != hipSuccess ||
                      hipMemcpy(s->d_px, px.data(), (size_t)total * 16, hipMemcpyHostToDevice) != hipSuccess ||
                      hipMemcpy(s->d_thr, thr.data(), (size_t)total * 8, hipMemcpyHostToDevice) != hipSuccess)) ||
           (!dp.empty() && hipMemcpy(s->d_probs, dp.data(), dp.size() * sizeof(Sim3Prob), hipMemcpyHostToDevice) != hipSuccess))
    st = fail(nullptr, ORBFE_EDEVICE, "orbfe_sim3_create: upload failed");
  if (have_cur) (void)hipSetDevice(cur);
  if (st != ORBFE_OK) {
    orbfe_sim3_destroy(s.release());
    return st;
  }
  s->bytes_uploaded = total * 48 + (int64_t)(dp.size() * sizeof(Sim3Prob));
  *out = s.release();
  return ORBFE_OK;
}

void orbfe_sim3_destroy(orbfe_sim3* s) {
  if (!s) return;
  int cur = -1;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  (void)hipSetDevice(s->device);
  for (void* p : {(void*)s->d_pq, (void*)s->d_px, (void*)s->d_thr, (void*)s->d_probs})
    if (p) (void)hipFree(p);
  ransac::io_release(&s->io);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  if (have_cur) (void)hipSetDevice(cur);
  delete s;
}

orbfe_status orbfe_sim3_iterate(orbfe_sim3* s, int32_t problem, int32_t n_iterations, float* model, int32_t* has_model, int32_t* inliers,
                                int64_t* n_inliers, int64_t cap, int32_t* ret, int32_t* no_more) {
  if (!s || !model || !has_model || !n_inliers || !ret || !no_more || cap < 0 || *n_inliers < 0 || *n_inliers > cap || (cap > 0 && !inliers))
    return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_iterate: bad arguments");
  if (problem < 0 || problem >= (int32_t)s->probs.size())
    return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_iterate: problem %d of %zu", problem, s->probs.size());
  std::lock_guard<std::mutex> lk(g_sim3_mu);
  Prob& pr = s->probs[(size_t)problem];
  *ret = 0;
  const int32_t k = pr.n >= kMinSet ? std::max(0, std::min(n_iterations, pr.max_it - pr.cur)) : 0;
  // the next record serves this call if the call is the predicted one: same problem and n, engine untouched (the entry model and list
  // change nothing: modelFunc always writes and checkInliers clears, S2)
  bool hit = s->next > 0 && s->next < s->recs.size();
  if (hit) {
    const CallRec& r = s->recs[s->next];
    hit = r.prob == problem && r.n == n_iterations && r.engine_start == g_engine && r.nh == k;
  }
  if (!hit && s->next > 0 && s->next < s->recs.size()) {
    // The caller left out problems the schedule had before this one (computeSim3 discards a candidate after its solver is made, when too
    // few matches pass vbChoose, and never iterates it): they would break every round's prediction, so later schedules omit them.
    const size_t end = std::min(s->recs.size(), s->next + s->probs.size());
    size_t j = s->next;
    while (j < end && s->recs[j].prob != problem) ++j;
    if (j < end)
      for (size_t i = s->next; i < j; ++i) s->probs[(size_t)s->recs[i].prob].skipped = true;
  }
  pr.skipped = false;
  if (pr.n < kMinSet) {  // S5
    if (hit) s->next += 1;
    else drop_records(s);
    pr.called = true;
    *no_more = 1;
    return ORBFE_OK;
  }
  CallRec r;
  if (hit) {
    r = s->recs[s->next];
    s->next += 1;
  } else if (k == 0) {  // the budget is spent: nothing for the device
    drop_records(s);
    r = CallRec{problem, n_iterations, 0, 0, g_engine, {}};
  } else {
    int cur = -1;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    const orbfe_status st = speculate(s, problem, n_iterations);
    if (have_cur) (void)hipSetDevice(cur);
    if (st != ORBFE_OK) {
      drop_records(s);
      return st;
    }
    r = s->recs[0];
    s->next = 1;
  }
  if (r.nh != k || r.prob != problem) {
    drop_records(s);
    return fail(nullptr, ORBFE_EDEVICE, "orbfe_sim3_iterate: inconsistent speculation");
  }
  // replay Ransac::iterate from the records on copies, committed when the result fits
  std::vector<int32_t> list(inliers, inliers + *n_inliers);
  float cur_model[12];
  std::memcpy(cur_model, model, sizeof cur_model);
  bool has = *has_model != 0;
  int32_t cur = pr.cur, best = pr.best;
  bool best_changed = false;
  float best_model[12];
  std::vector<int32_t> best_list;
  bool success = false;
  uint32_t eng = g_engine;
  for (int32_t i = 0; i < r.nh; ++i) {
    const size_t h = (size_t)(r.h0 + i);
    const Sim3Out& o = s->out[h];
    std::memcpy(cur_model, o.model, sizeof cur_model);
    has = true;
    eng = r.after[(size_t)i];
    list.clear();  // S2
    ransac::append_bits(s->masks.data() + s->hyps[h].mask_off, pr.words, list);
    if (o.count > pr.min_inlier) {
      if (o.count > best) {
        best = o.count;
        best_changed = true;
        std::memcpy(best_model, cur_model, sizeof best_model);
        best_list = list;
      }
      if (!o.refined) {
        drop_records(s);
        return fail(nullptr, ORBFE_EDEVICE, "orbfe_sim3_iterate: refine record missing");
      }
      std::memcpy(cur_model, o.ref_model, sizeof cur_model);
      list.clear();
      ransac::append_bits(s->ref_masks.data() + s->hyps[h].mask_off, pr.words, list);
      if (o.ref_count > pr.min_inlier) {
        success = true;  // S3: the budget is not spent
        break;
      }
    }
    ++cur;
  }
  bool set_no_more = false;
  const std::vector<int32_t>* res = &list;
  const float* res_model = cur_model;
  bool res_has = has;
  if (success) {
    *ret = 1;
  } else {
    set_no_more = cur >= pr.max_it;
    const int32_t b = best_changed ? best : pr.best;
    if (b > 0) {  // S4
      *ret = 1;
      res = best_changed ? &best_list : &pr.best_list;
      res_model = best_changed ? best_model : pr.best_model;
      res_has = true;
    }
  }
  if ((int64_t)res->size() > cap) {
    *n_inliers = (int64_t)res->size();
    *ret = 0;
    drop_records(s);
    return fail(nullptr, ORBFE_ECAPACITY, "orbfe_sim3_iterate: %zu inliers, room for %lld", res->size(), (long long)cap);
  }
  // commit
  std::copy(res->begin(), res->end(), inliers);
  *n_inliers = (int64_t)res->size();
  std::memcpy(model, res_model, 12 * sizeof(float));
  *has_model = res_has ? 1 : 0;
  if (set_no_more) *no_more = 1;
  pr.cur = cur;
  pr.called = true;
  if (best_changed) {
    pr.best = best;
    std::memcpy(pr.best_model, best_model, sizeof best_model);
    pr.best_list = std::move(best_list);
  }
  g_engine = eng;
  if (success) drop_records(s);
  return ORBFE_OK;
}

orbfe_status orbfe_sim3_engine(uint32_t* get, const uint32_t* set) {
  return ransac::engine_access(g_sim3_mu, g_engine, get, set, "orbfe_sim3_engine");
}

orbfe_status orbfe_sim3_stats(orbfe_sim3* s, int64_t* launches, int64_t* hypotheses) {
  if (!s) return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_stats: NULL set");
  std::lock_guard<std::mutex> lk(g_sim3_mu);
  if (launches) *launches = s->launches;
  if (hypotheses) *hypotheses = s->hypotheses;
  return ORBFE_OK;
}

orbfe_status orbfe_sim3_profile(orbfe_sim3* s, int32_t enable, double* device_us, int64_t* bytes_uploaded) {
  if (!s) return fail(nullptr, ORBFE_EBADARG, "orbfe_sim3_profile: NULL set");
  std::lock_guard<std::mutex> lk(g_sim3_mu);
  if (enable > 0 && !s->ev0) {
    int cur = -1;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    const bool ok = hipSetDevice(s->device) == hipSuccess && hipEventCreate(&s->ev0) == hipSuccess && hipEventCreate(&s->ev1) == hipSuccess;
    if (have_cur) (void)hipSetDevice(cur);
    if (!ok) return fail(nullptr, ORBFE_EDEVICE, "orbfe_sim3_profile: cannot create events on device %d", s->device);
  }
  if (enable >= 0) s->profile = enable > 0;
  if (device_us) *device_us = s->device_us;
  if (bytes_uploaded) *bytes_uploaded = s->bytes_uploaded;
  return ORBFE_OK;
}

}  // extern "C"
