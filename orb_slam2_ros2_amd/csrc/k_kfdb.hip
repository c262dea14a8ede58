// k_kfdb.hip -- KeyFrameDB's query (src/KeyFrameDB.cc) on gfx950: the shared-word count of every keyframe against one query BowVector,
// minWordFilter, the L1 score of the survivors and (loop mode) minScoreFilter.  Host side: orbfe_kfdb.hip; the rules: include/orbfe.h and
// DESIGN 4.15; the checker: tests/kfdb_restatement.py.
//
// Storage: every keyframe is a slot (KfSlot) whose sorted words / values lie in two pools.  No inverted index: one pass over the stored
// words finds the common words that both the count and the score need, and add / erase / set_bad touch nothing but the slot table.
//   k_kfdb_count   one wave per slot (grid-stride, the workgroup count is an argument: no dispatch packet); lane l looks up the slot's words
//                  l, l + 64, .. in the query's sorted words (LDS, or global memory above KFDB_QLDS words) by binary search, the ballot's
//                  popcount is the count.  Ignored, bad and free slots count 0.  The grid-wide maximum goes to an agent-scope atomicMax on
//                  the query header, which only the NEXT launch reads.
//   k_kfdb_score   th1 = (float)((double)(float)max * 0.8); a slot with count > 0 and !((float)count < th1) is scored: the lanes form the
//                  terms |v - w| - |v| - |w| (v: the query's value, w: the keyframe's) of the common words, and the wave adds them up in
//                  ascending word order (readlane by readlane, every lane the same sequence of adds: DBoW's l1Score bit for bit), -s / 2.
//                  Loop mode drops score < min_score; a survivor claims a record by atomicAdd on the header.
//   k_kfdb_score_list   the same score for a list of slots (orbfe_kfdb_score).
//   k_kfdb_gather  copies the live slots' words / values into a new pool (the pool's growth and compaction).
//   k_kfdb_scatter writes changed slot records (add / erase / set_bad) from one uploaded list.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbfe_internal.h"

#define KFDB_WG 256                  // four waves: four slots in flight per workgroup
#define KFDB_WAVES (KFDB_WG / 64)
#define KFDB_QLDS 8192               // query words held in LDS (32 KB); larger queries search global memory

// first index in Q[lo, nq) whose word is >= w
template <typename P>
__device__ __forceinline__ int kfdb_lower(P Q, int lo, int nq, uint32_t w) {
  int hi = nq;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (Q[mid] < w)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool kfdb_ignored(const uint32_t* __restrict__ ign, int n_ign, uint32_t s) {
  int lo = 0, hi = n_ign;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ign[mid] < s)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n_ign && ign[lo] == s;
}

__device__ __forceinline__ double kfdb_readlane(double v, int k) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}

// the shared-word count of one slot (every lane gets it)
template <typename P>
__device__ __forceinline__ int kfdb_slot_count(P Q, int nq, const uint32_t* __restrict__ W, uint32_t len, int lane) {
  int c = 0, lo = 0;
  for (uint32_t b = 0; b < len; b += 64) {
    const uint32_t i = b + (uint32_t)lane;
    bool f = false;
    if (i < len) {
      const uint32_t w = W[i];
      lo = kfdb_lower(Q, lo, nq, w);  // the lane's words ascend: its next lower bound is not below this one
      f = lo < nq && Q[lo] == w;
    }
    c += __popcll(__ballot(f));
  }
  return c;
}

// DBoW's L1 score of the query against one slot: -s / 2, s the sequential sum over the common words in ascending order
template <typename P>
__device__ __forceinline__ double kfdb_slot_score(P Q, const double* __restrict__ QV, int nq, const uint32_t* __restrict__ W,
                                                  const double* __restrict__ V, uint32_t len, int lane) {
  double s = 0.0;
  int lo = 0;
  for (uint32_t b = 0; b < len; b += 64) {
    const uint32_t i = b + (uint32_t)lane;
    bool f = false;
    double t = 0.0;
    if (i < len) {
      const uint32_t w = W[i];
      lo = kfdb_lower(Q, lo, nq, w);
      f = lo < nq && Q[lo] == w;
      if (f) {
        const double v = QV[lo], x = V[i];
        t = fabs(v - x) - fabs(v) - fabs(x);
      }
    }
    uint64_t m = __ballot(f);
    while (m) {  // uniform: every lane adds the same terms in the same (ascending word) order
      const int k = __builtin_ctzll(m);
      m &= m - 1;
      s += kfdb_readlane(t, k);
    }
  }
  return -s / 2.0;
}

template <bool IN_LDS>
__device__ __forceinline__ void kfdb_count_body(const uint32_t* Q, int nq, const KfSlot* __restrict__ slots, int n_slots, const uint32_t* __restrict__ wpool,
                                                const uint32_t* __restrict__ ign, int n_ign, int32_t* __restrict__ counts, KfdbHdr* hdr, int n_wg) {
  const int lane = threadIdx.x & 63;
  for (int s = blockIdx.x * KFDB_WAVES + (threadIdx.x >> 6); s < n_slots; s += n_wg * KFDB_WAVES) {
    const KfSlot sl = slots[s];
    int c = 0;
    if ((sl.flags & (KFDB_LIVE | KFDB_BAD)) == KFDB_LIVE && !kfdb_ignored(ign, n_ign, (uint32_t)s)) c = kfdb_slot_count(Q, nq, wpool + sl.off, sl.len, lane);
    if (lane == 0) {
      counts[s] = c;
      if (c) atomicMax(&hdr->max_count, (uint32_t)c);
    }
  }
}

__global__ __launch_bounds__(KFDB_WG) void k_kfdb_count(const uint32_t* __restrict__ qwords, int nq, const KfSlot* __restrict__ slots, int n_slots,
                                                        const uint32_t* __restrict__ wpool, const uint32_t* __restrict__ ign, int n_ign,
                                                        int32_t* __restrict__ counts, KfdbHdr* hdr, int n_wg) {
  __shared__ uint32_t s_q[KFDB_QLDS];
  if (nq <= KFDB_QLDS) {
    for (int i = threadIdx.x; i < nq; i += KFDB_WG) s_q[i] = qwords[i];
    __syncthreads();
    kfdb_count_body<true>(s_q, nq, slots, n_slots, wpool, ign, n_ign, counts, hdr, n_wg);
  } else {
    kfdb_count_body<false>(qwords, nq, slots, n_slots, wpool, ign, n_ign, counts, hdr, n_wg);
  }
}

template <bool IN_LDS>
__device__ __forceinline__ void kfdb_score_body(const uint32_t* Q, const double* __restrict__ QV, int nq, const KfSlot* __restrict__ slots,
                                                int n_slots, const uint32_t* __restrict__ wpool, const double* __restrict__ vpool,
                                                const int32_t* __restrict__ counts, KfdbHdr* hdr, int has_min, double min_score,
                                                KfdbRec* __restrict__ recs, uint32_t rec_cap, int n_wg) {
  const int lane = threadIdx.x & 63;
  const float th1 = (float)((double)(float)hdr->max_count * 0.8);  // minWordFilter: float th1 = (float)maxWordNum * 0.8
  for (int s = blockIdx.x * KFDB_WAVES + (threadIdx.x >> 6); s < n_slots; s += n_wg * KFDB_WAVES) {
    const int c = counts[s];
    if (c == 0 || (float)c < th1) continue;
    const KfSlot sl = slots[s];
    const double score = kfdb_slot_score(Q, QV, nq, wpool + sl.off, vpool + sl.off, sl.len, lane);
    if (has_min && score < min_score) continue;  // minScoreFilter
    if (lane == 0) {
      const uint32_t k = atomicAdd(&hdr->n_out, 1u);
      if (k < rec_cap) {
        KfdbRec r;
        r.slot = (uint32_t)s;
        r.count = c;
        r.score = score;
        recs[k] = r;
      }
    }
  }
}

__global__ __launch_bounds__(KFDB_WG) void k_kfdb_score(const uint32_t* __restrict__ qwords, const double* __restrict__ qvalues, int nq,
                                                        const KfSlot* __restrict__ slots, int n_slots, const uint32_t* __restrict__ wpool,
                                                        const double* __restrict__ vpool, const int32_t* __restrict__ counts, KfdbHdr* hdr,
                                                        int has_min, double min_score, KfdbRec* __restrict__ recs, uint32_t rec_cap, int n_wg) {
  __shared__ uint32_t s_q[KFDB_QLDS];
  if (nq <= KFDB_QLDS) {
    for (int i = threadIdx.x; i < nq; i += KFDB_WG) s_q[i] = qwords[i];
    __syncthreads();
    kfdb_score_body<true>(s_q, qvalues, nq, slots, n_slots, wpool, vpool, counts, hdr, has_min, min_score, recs, rec_cap, n_wg);
  } else {
    kfdb_score_body<false>(qwords, qvalues, nq, slots, n_slots, wpool, vpool, counts, hdr, has_min, min_score, recs, rec_cap, n_wg);
  }
}

// scores of the slots list[0 .. n) into out[i]; the query's words are read from global memory (a handful of slots per call)
__global__ __launch_bounds__(KFDB_WG) void k_kfdb_score_list(const uint32_t* __restrict__ qwords, const double* __restrict__ qvalues, int nq,
                                                             const KfSlot* __restrict__ slots, const uint32_t* __restrict__ wpool,
                                                             const double* __restrict__ vpool, const uint32_t* __restrict__ list, int n,
                                                             double* __restrict__ out, int n_wg) {
  const int lane = threadIdx.x & 63;
  for (int i = blockIdx.x * KFDB_WAVES + (threadIdx.x >> 6); i < n; i += n_wg * KFDB_WAVES) {
    const KfSlot sl = slots[list[i]];
    const double score = kfdb_slot_score(qwords, qvalues, nq, wpool + sl.off, vpool + sl.off, sl.len, lane);
    if (lane == 0) out[i] = score;
  }
}

// the live slots' words / values from the old pools to new_off[s] in the new ones (one wave per slot)
__global__ __launch_bounds__(KFDB_WG) void k_kfdb_gather(const KfSlot* __restrict__ slots, const uint64_t* __restrict__ new_off, int n_slots,
                                                         const uint32_t* __restrict__ w_old, const double* __restrict__ v_old,
                                                         uint32_t* __restrict__ w_new, double* __restrict__ v_new, int n_wg) {
  const int lane = threadIdx.x & 63;
  for (int s = blockIdx.x * KFDB_WAVES + (threadIdx.x >> 6); s < n_slots; s += n_wg * KFDB_WAVES) {
    const KfSlot sl = slots[s];
    if (!(sl.flags & KFDB_LIVE)) continue;
    const uint64_t o = new_off[s];
    for (uint32_t i = (uint32_t)lane; i < sl.len; i += 64) {
      w_new[o + i] = w_old[sl.off + i];
      v_new[o + i] = v_old[sl.off + i];
    }
  }
}

__global__ __launch_bounds__(KFDB_WG) void k_kfdb_scatter(const uint32_t* __restrict__ idx, const KfSlot* __restrict__ src, int n,
                                                          KfSlot* __restrict__ slots) {
  const int i = blockIdx.x * KFDB_WG + threadIdx.x;
  if (i < n) slots[idx[i]] = src[i];
}

namespace {
int kfdb_grid(int n_items) {
  const int wg = (n_items + KFDB_WAVES - 1) / KFDB_WAVES;
  return wg < 1 ? 1 : (wg > 4096 ? 4096 : wg);
}
}  // namespace

void launch_kfdb_query(hipStream_t st, const uint32_t* qwords, const double* qvalues, int nq, const KfSlot* slots, int n_slots,
                       const uint32_t* wpool, const double* vpool, const uint32_t* ign, int n_ign, int32_t* counts, KfdbHdr* hdr,
                       int has_min, double min_score, KfdbRec* recs, uint32_t rec_cap) {
  if (n_slots <= 0) return;
  const int g = kfdb_grid(n_slots);
  hipLaunchKernelGGL(k_kfdb_count, dim3((unsigned)g), dim3(KFDB_WG), 0, st, qwords, nq, slots, n_slots, wpool, ign, n_ign, counts, hdr, g);
  hipLaunchKernelGGL(k_kfdb_score, dim3((unsigned)g), dim3(KFDB_WG), 0, st, qwords, qvalues, nq, slots, n_slots, wpool, vpool, counts, hdr, has_min,
                     min_score, recs, rec_cap, g);
}

void launch_kfdb_score_list(hipStream_t st, const uint32_t* qwords, const double* qvalues, int nq, const KfSlot* slots, const uint32_t* wpool,
                            const double* vpool, const uint32_t* list, int n, double* out) {
  if (n <= 0) return;
  const int g = kfdb_grid(n);
  hipLaunchKernelGGL(k_kfdb_score_list, dim3((unsigned)g), dim3(KFDB_WG), 0, st, qwords, qvalues, nq, slots, wpool, vpool, list, n, out, g);
}

void launch_kfdb_gather(hipStream_t st, const KfSlot* slots, const uint64_t* new_off, int n_slots, const uint32_t* w_old, const double* v_old,
                        uint32_t* w_new, double* v_new) {
  if (n_slots <= 0) return;
  const int g = kfdb_grid(n_slots);
  hipLaunchKernelGGL(k_kfdb_gather, dim3((unsigned)g), dim3(KFDB_WG), 0, st, slots, new_off, n_slots, w_old, v_old, w_new, v_new, g);
}

void launch_kfdb_scatter(hipStream_t st, const uint32_t* idx, const KfSlot* src, int n, KfSlot* slots) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_kfdb_scatter, dim3((unsigned)((n + KFDB_WG - 1) / KFDB_WG)), dim3(KFDB_WG), 0, st, idx, src, n, slots);
}
