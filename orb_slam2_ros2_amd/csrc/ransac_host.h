// ransac_host.h -- the HIP side of a speculated Ransac<T>::iterate set, ransac::Set<Traits> (orbfe_pnp.hip, orbfe_sim3.hip): the sampling
// engine, setRansacParams, the round-robin schedule a speculation covers, its one upload / launch / download, and the calls replayed from
// its records by ransac_replay.h.  Host only; include after orbfe_ctx.h.  Traits supply
//   Policy (ransac_replay.h), Hyp, Out (orbfe_internal.h), view(out, mask, refine mask) -> HypView,
//   Plan: how a call's hypotheses are appended (open_call), the layout's extra takes (take, put) and the launch,
//   before_launch / after_launch (NoHooks: none).
#pragma once
#include <emmintrin.h>

#include "ransac_replay.h"

namespace ransac {

// minstd_rand0 and libstdc++'s uniform_int_distribution<size_t>(0, n - 1) (the scaling path: minstd's range is not 2^32 - 1)
inline uint32_t minstd(uint32_t& x) {
  x = (uint32_t)((uint64_t)x * 16807u % 2147483647u);
  return x;
}
inline uint32_t uniform_int(uint32_t& x, uint32_t n) {
  const uint64_t urngrange = 2147483645u, uerange = n;
  const uint64_t scaling = urngrange / uerange, past = uerange * scaling;
  uint64_t r;
  do r = (uint64_t)minstd(x) - 1u;
  while (r >= past);
  return (uint32_t)(r / scaling);
}
// randomSample(): k distinct indices below n, a repeated one drawn again
inline void random_sample(uint32_t& x, uint32_t n, int k_want, int32_t* out) {
  int k = 0;
  while (k != k_want) {
    const int32_t r = (int32_t)uniform_int(x, n);
    bool seen = false;
    for (int i = 0; i < k; ++i) seen |= out[i] == r;
    if (!seen) out[k++] = r;
  }
}

// setRansacParams(): its float / double mix, cvRound as cvtsd2si
inline void ransac_params(int32_t N, int32_t min_set, int32_t max_iterations, float ratio, float prob, int32_t* min_inlier, int32_t* max_it) {
  *min_inlier = (int32_t)std::max((float)min_set, (float)N * ratio);
  const float r = (float)*min_inlier / (float)N;
  if (r >= 1) {
    *max_it = 0;
    return;
  }
  const double q = std::log(1 - prob) / std::log(1 - std::pow(r, min_set));
  *max_it = std::min(max_iterations, _mm_cvtsd_si32(_mm_set_sd(q)));
}

// a problem the caller's loop will call again: budget left, or never called (the first call is what sets bNoMore)
inline bool alive(int32_t n, int32_t min_set, int32_t cur, int32_t max_it, bool called) {
  return n >= min_set ? (cur < max_it || !called) : !called;
}

// The schedule the reference's loops run from a call on problem p of P: that call, the rest of its round, then whole rounds, ascending,
// while a problem is live and the speculation has room.  add(q, first) appends one call and advances the caller's copies of the state.
template <class Alive, class Add, class Full>
inline void round_robin(int P, int p, Alive live, Add add, Full full) {
  add(p, true);
  for (int q = p + 1; q < P && !full(); ++q)
    if (live(q)) add(q, false);
  for (bool any = true; any && !full();) {
    any = false;
    for (int q = 0; q < P && !full(); ++q)
      if (live(q)) {
        add(q, false);
        any = true;
      }
  }
}

// a speculation's device block (upload, results, scratch) and its page-locked staging, grown by half when too small
struct Io {
  uint8_t* d_io = nullptr;
  size_t io_bytes = 0;
  uint8_t* h_io = nullptr;
  size_t h_bytes = 0;
};
inline orbfe_status io_reserve(Io* s, size_t dev_bytes, size_t host_bytes) {
  if (s->io_bytes < dev_bytes) {
    if (s->d_io) (void)hipFree(s->d_io);
    s->d_io = nullptr;
    s->io_bytes = 0;
    const size_t b = std::max<size_t>(dev_bytes + dev_bytes / 2, 1 << 20);
    HIP_TRY(nullptr, hipMalloc((void**)&s->d_io, b));
    s->io_bytes = b;
  }
  if (s->h_bytes < host_bytes) {
    if (s->h_io) (void)hipHostFree(s->h_io);
    s->h_io = nullptr;
    s->h_bytes = 0;
    const size_t b = std::max<size_t>(host_bytes + host_bytes / 2, 1 << 20);
    HIP_TRY(nullptr, hipHostMalloc((void**)&s->h_io, b, hipHostMallocDefault));
    s->h_bytes = b;
  }
  return ORBFE_OK;
}
inline void io_release(Io* s) {
  if (s->d_io) (void)hipFree(s->d_io);
  if (s->h_io) (void)hipHostFree(s->h_io);
  *s = Io{};
}

constexpr size_t kMaxHyps = 1 << 17;  // one speculation covers at most this many hypotheses (the rest: a later one)

struct NoHooks {
  template <class S>
  static orbfe_status before_launch(S&, size_t) { return ORBFE_OK; }
  template <class S>
  static orbfe_status after_launch(S&) { return ORBFE_OK; }
};

template <class T>
struct Set {
  // Ransac<T>'s function-local static std::default_random_engine (P6, S7): one per instantiation, so one per process for every PnP set
  // and another for every Sim3 set, each behind a lock that also serialises its sets' iterate.
  static inline std::mutex mu;
  static inline uint32_t engine = 1;

  int device = 0;
  hipStream_t stream = nullptr;
  float cam[4] = {};
  std::vector<Prob> probs;
  float* d_pts[3] = {};  // device: the problems' three per-point arrays ..
  RansacProb* d_probs = nullptr;  // .. and records
  Io io;                 // a speculation's upload, results and scratch, and its page-locked staging
  // the speculation being replayed
  Records R;
  std::vector<typename T::Hyp> hyps;
  std::vector<typename T::Out> out;
  std::vector<uint64_t> masks, ref_masks;
  int64_t launches = 0, hypotheses = 0;

  // create's refusals after the solver's own, in this order: offsets, sizes, arrays, octaves -- all before any device call -- then the device
  static orbfe_status check_create(const char* who, const char* nouns, int64_t max_n, int64_t max_total, int32_t device_id, int32_t n_problems,
                                   const int64_t* offsets, bool arrays_given, std::initializer_list<const int32_t*> octaves, int32_t n_levels) {
    if (offsets[0] != 0) return fail(nullptr, ORBFE_EBADARG, "%s: offsets[0] must be 0", who);
    for (int32_t i = 0; i < n_problems; ++i)
      if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > max_n)
        return fail(nullptr, ORBFE_EBADARG, "%s: problem %d has %lld %s (0 .. %lld)", who, i, (long long)(offsets[i + 1] - offsets[i]), nouns,
                    (long long)max_n);
    const int64_t total = offsets[n_problems];
    if (total > max_total) return fail(nullptr, ORBFE_EBADARG, "%s: %lld %s in all", who, (long long)total, nouns);
    if (total > 0 && !arrays_given) return fail(nullptr, ORBFE_EBADARG, "%s: NULL %s", who, nouns);
    for (int64_t i = 0; i < total; ++i)
      for (const int32_t* oc : octaves)
        if (oc[i] < 0 || oc[i] >= n_levels)
          return fail(nullptr, ORBFE_EBADARG, "%s: octave %d of %d levels (%s, index %lld)", who, oc[i], n_levels, nouns, (long long)i);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      return fail(nullptr, ORBFE_EDEVICE, "%s: no HIP device (this library has no CPU fallback)", who);
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, ORBFE_EBADARG, "%s: device %d of %d", who, device_id, ndev);
    return ORBFE_OK;
  }

  // setRansacParams of every problem; a stream, the three per-point arrays (width[i] floats a point) and the problem records on the device
  orbfe_status open(const char* who, const char* nouns, int32_t device_id, const orbfe_camera& c, int32_t n_problems, const int64_t* offsets,
                    int32_t max_iterations, float ratio, float prob, const float* const pts[3], const int width[3]) {
    device = device_id;
    cam[0] = c.fx, cam[1] = c.fy, cam[2] = c.cx, cam[3] = c.cy;
    probs.resize((size_t)n_problems);
    std::vector<RansacProb> dp((size_t)n_problems);
    for (int32_t i = 0; i < n_problems; ++i) {
      Prob& p = probs[(size_t)i];
      p.off = (int32_t)offsets[i];
      p.n = (int32_t)(offsets[i + 1] - offsets[i]);
      p.words = (p.n + 63) / 64;
      ransac_params(p.n, T::Policy::kMinSet, max_iterations, ratio, prob, &p.min_inlier, &p.max_it);
      dp[(size_t)i] = RansacProb{p.off, p.n, p.words, p.min_inlier};
    }
    const int64_t total = offsets[n_problems];
    const size_t nb = (size_t)std::max<int64_t>(total, 1), pb = std::max<size_t>(dp.size(), 1) * sizeof(RansacProb);
    DeviceScope dev(device_id);
    if (dev.err != hipSuccess || hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess)
      return fail(nullptr, ORBFE_EDEVICE, "%s: cannot create a stream on device %d", who, device_id);
    for (int a = 0; a < 3; ++a)
      if (hipMalloc((void**)&d_pts[a], nb * 4 * (size_t)width[a]) != hipSuccess)
        return fail(nullptr, ORBFE_ENOMEM, "%s: cannot allocate %lld %s on device %d", who, (long long)total, nouns, device_id);
    if (hipMalloc((void**)&d_probs, pb) != hipSuccess)
      return fail(nullptr, ORBFE_ENOMEM, "%s: cannot allocate %lld %s on device %d", who, (long long)total, nouns, device_id);
    for (int a = 0; a < 3 && total; ++a)
      if (hipMemcpy(d_pts[a], pts[a], (size_t)total * 4 * (size_t)width[a], hipMemcpyHostToDevice) != hipSuccess)
        return fail(nullptr, ORBFE_EDEVICE, "%s: upload failed", who);
    if (!dp.empty() && hipMemcpy(d_probs, dp.data(), dp.size() * sizeof(RansacProb), hipMemcpyHostToDevice) != hipSuccess)
      return fail(nullptr, ORBFE_EDEVICE, "%s: upload failed", who);
    return ORBFE_OK;
  }

  ~Set() {
    DeviceScope dev(device);
    for (void* p : {(void*)d_pts[0], (void*)d_pts[1], (void*)d_pts[2], (void*)d_probs})
      if (p) (void)hipFree(p);
    io_release(&io);
    if (stream) (void)hipStreamDestroy(stream);
  }

  static orbfe_status stats(const char* who, Set* s, int64_t* n_launches, int64_t* n_hypotheses) {
    if (!s) return fail(nullptr, ORBFE_EBADARG, "%s: NULL set", who);
    std::lock_guard<std::mutex> lk(mu);
    if (n_launches) *n_launches = s->launches;
    if (n_hypotheses) *n_hypotheses = s->hypotheses;
    return ORBFE_OK;
  }

  // get and / or set the engine's state under its lock
  static orbfe_status engine_access(const char* who, uint32_t* get, const uint32_t* set) {
    std::lock_guard<std::mutex> lk(mu);
    if (get) *get = engine;
    if (set) {
      if (*set == 0 || *set >= 2147483647u) return fail(nullptr, ORBFE_EBADARG, "%s: state %u outside 1 .. 2^31 - 2", who, *set);
      engine = *set;
    }
    return ORBFE_OK;
  }

  // Speculate from the call (p, n, entry state): the schedule the reference's loop will most likely run -- round-robin over the live
  // problems, ascending, n each, no refine success -- its samples drawn from a copy of the engine, then one upload, the launch, one download.
  orbfe_status speculate(const char* who, int32_t p, int32_t n, const float* model, bool has_model, const int32_t* entry, int64_t entry_len) {
    drop_records(R);
    hyps.clear();
    const int P = (int)probs.size();
    std::vector<int32_t> cur(P);
    std::vector<char> called(P);
    for (int q = 0; q < P; ++q) {
      cur[q] = probs[q].cur;
      called[q] = probs[q].called;
    }
    uint32_t eng = engine;
    int64_t words = 0;
    typename T::Plan plan(model, has_model, entry, entry_len);
    auto add_call = [&](int32_t q, bool first) {
      const Prob& pr = probs[q];
      const int32_t k = budget(pr, T::Policy::kMinSet, n, cur[q]);
      CallRec r{q, n, 0, k, -1, eng, {}};
      const size_t first_hyp = hyps.size();
      r.entry_hyp = plan.open_call(hyps, pr, q, first, k);
      r.h0 = (int32_t)hyps.size();
      for (int32_t i = 0; i < k; ++i) {
        typename T::Hyp h{};
        h.prob = q;
        random_sample(eng, (uint32_t)pr.n, T::Policy::kMinSet, h.idx);
        r.after.push_back(eng);
        hyps.push_back(h);
      }
      for (size_t h = first_hyp; h < hyps.size(); ++h) {
        hyps[h].mask_off = (int32_t)words;
        words += pr.words;
      }
      cur[q] += k;
      called[q] = 1;
      R.recs.push_back(std::move(r));
    };
    round_robin(
        P, p, [&](int q) { return !probs[q].skipped && alive(probs[q].n, T::Policy::kMinSet, cur[q], probs[q].max_it, called[q]); }, add_call,
        [&] { return hyps.size() >= kMaxHyps || words > 0x3FFFFFFF; });
    if (words > 0x7FFFFFFF) return fail(nullptr, ORBFE_ECAPACITY, "%s: speculation too large", who);
    const size_t nh = hyps.size();
    // upload: hyps | the plan's;  download: out | masks | refine masks;  device only: the plan's scratch
    ScratchLayout L;
    ScratchRegion up, down;
    const size_t o_h = L.open(up).take<typename T::Hyp>(nh), scratch_bytes = plan.take(L),
                 o_out = L.close(up).open(down).take<typename T::Out>(nh), o_m = L.take<uint64_t>((size_t)words),
                 o_rm = L.take<uint64_t>((size_t)words), o_scratch = L.close(down).take(scratch_bytes);
    TRY(io_reserve(&io, L.end(), down.end));
    StagedIo sio(io.d_io, io.h_io, stream);
    sio.put(o_h, hyps.data(), nh * sizeof(typename T::Hyp));
    plan.put(sio);
    HIP_TRY(nullptr, sio.upload(up));
    TRY(T::before_launch(*this, up.bytes()));
    plan.launch(*this, sio, o_h, (int)nh, o_out, o_m, o_rm, o_scratch);
    HIP_TRY(nullptr, hipGetLastError());
    TRY(T::after_launch(*this));
    HIP_TRY(nullptr, sio.fetch(down, down.begin));
    out.resize(nh);
    masks.resize((size_t)words);
    ref_masks.resize((size_t)words);
    sio.get(out.data(), o_out, nh * sizeof(typename T::Out));
    sio.get(masks.data(), o_m, (size_t)words * 8);
    sio.get(ref_masks.data(), o_rm, (size_t)words * 8);
    launches += 1;
    hypotheses += (int64_t)nh;
    return ORBFE_OK;
  }

  // Ransac<T>::iterate of one problem; the caller has checked the arguments and holds the lock
  orbfe_status iterate(const char* who, int32_t problem, int32_t n_iterations, float* model, int32_t* has_model, int32_t* inliers,
                       int64_t* n_inliers, int64_t cap, int32_t* ret, int32_t* no_more) {
    orbfe_status spec = ORBFE_OK;
    const Verdict v = ransac::iterate<typename T::Policy>(
        probs, R, engine, problem, n_iterations, model, has_model, inliers, n_inliers, cap, ret, no_more,
        [&](size_t h) { return T::view(out[h], masks.data() + hyps[h].mask_off, ref_masks.data() + hyps[h].mask_off); },
        [&](int32_t p, int32_t n, const float* m, bool has_m, const int32_t* entry, int64_t entry_len) {
          DeviceScope dev(device);  // (the io block belongs to the set's device)
          spec = dev.err != hipSuccess ? fail(nullptr, ORBFE_EDEVICE, "%s: hipSetDevice(%d) -> %s", who, device, hipGetErrorString(dev.err))
                                       : speculate(who, p, n, m, has_m, entry, entry_len);
          return spec == ORBFE_OK;
        });
    switch (v) {
      case kDone: return ORBFE_OK;
      case kSpeculationFailed: return spec;
      case kNoRoom: return fail(nullptr, ORBFE_ECAPACITY, "%s: %lld inliers, room for %lld", who, (long long)*n_inliers, (long long)cap);
      case kNoRefineRecord: return fail(nullptr, ORBFE_EDEVICE, "%s: refine record missing", who);
      case kNoEntryRecord: return fail(nullptr, ORBFE_EDEVICE, "%s: no record of the entry pose", who);
      default: return fail(nullptr, ORBFE_EDEVICE, "%s: inconsistent speculation", who);
    }
  }
};

}  // namespace ransac
