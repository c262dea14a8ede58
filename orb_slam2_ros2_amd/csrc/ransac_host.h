// ransac_host.h -- the host machinery the speculated Ransac<T>::iterate sets share (orbfe_pnp.hip, orbfe_sim3.hip): the sampling
// engine's arithmetic, randomSample, setRansacParams, the liveness rule, the round-robin schedule a speculation covers and the io block
// of one speculation.  Host only; include after orbfe_ctx.h.  Each user keeps its own engine state and lock (the reference has one
// function-local static engine per Ransac<T> instantiation).
#pragma once
#include <emmintrin.h>

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

// get and / or set an engine's state under its lock
inline orbfe_status engine_access(std::mutex& mu, uint32_t& engine, uint32_t* get, const uint32_t* set, const char* who) {
  std::lock_guard<std::mutex> lk(mu);
  if (get) *get = engine;
  if (set) {
    if (*set == 0 || *set >= 2147483647u) return fail(nullptr, ORBFE_EBADARG, "%s: state %u outside 1 .. 2^31 - 2", who, *set);
    engine = *set;
  }
  return ORBFE_OK;
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

// the set bits of m[0 .. words), ascending, appended to list
inline void append_bits(const uint64_t* m, int32_t words, std::vector<int32_t>& list) {
  for (int32_t w = 0; w < words; ++w)
    for (uint64_t b = m[w]; b; b &= b - 1) list.push_back(w * 64 + __builtin_ctzll(b));
}

}  // namespace ransac
