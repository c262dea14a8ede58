// k_bowsearch.hip -- ORBMatcher::searchByBow (src/ORBMatcher.cc:170-253) of ONE query frame against up to ORBFE_BOW_SEARCH_MAX_KF stored
// keyframes, with verifyAngle (:1013-1051).  Three launches, none waits for the host:
//
// k_bow_match    one wave per (candidate keyframe, FeatureVector entry j of it): the keyframe feature's filter by mode, the entry's node
//                in the query's FeatureVector, getBestMatch over the node's query features that pass the mode's filter (bow_walk.h), the
//                threshold / ratio test (:237), the pair's angle bin (bow_angle.h).  Out: one BowSlot per entry.  Slot order IS the
//                reference's match order: nodes ascending, inside a node the keyframe's features in FeatureVector order.
// k_bow_select   one workgroup per candidate: the 30 bin counts in LDS, the three bins, then the survivors in (bin, slot) order -- a
//                match's place is the sizes of the chosen bins before its own plus the matches of its bin in earlier slots, counted
//                chunk by chunk in slot order with ballots.  Without the orientation check every slot carries bin 0, which is then the
//                one chosen bin: the same text is the plain stable compaction.  Out: the candidate's list in its own region, its length.
// k_bow_gather   one workgroup per candidate: the <= 64 lengths summed by one wave (every workgroup for itself: the lengths come from the
//                previous launch, nobody waits), workgroup 0 writes match_offsets, and each list moves to its place -- unless the total
//                exceeds the room, in which case only the offsets are written.
// For one candidate and a frame in its extraction slot (orbfe_track_reference_stored) the first two run alone: launch_bow_search_one.
//
// Every loop is bounded by a feature count, a node count or BOW_ANGLE_BINS.
#include <hip/hip_runtime.h>

#include "bow_angle.h"
#include "bow_walk.h"
#include "orbfe_internal.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace {

using namespace orbfe;

// Where the query's arrays are: behind the call's upload (BowQuery), where the keyframe store keeps them (BowQueryStored), or in an
// extraction slot with a FeatureVector in device memory whose node count the host does not know (BowQuerySlot).
__device__ __forceinline__ const uint8_t* q_desc(const uint8_t* up, const BowQuery& Q) { return up + Q.o_desc; }
__device__ __forceinline__ const uint8_t* q_desc(const uint8_t*, const BowQueryStored& Q) { return Q.desc; }
__device__ __forceinline__ const uint32_t* q_nodes(const uint8_t* up, const BowQuery& Q) { return (const uint32_t*)(up + Q.o_nodes); }
__device__ __forceinline__ const uint32_t* q_nodes(const uint8_t*, const BowQueryStored& Q) { return Q.nodes; }
__device__ __forceinline__ const int32_t* q_offs(const uint8_t* up, const BowQuery& Q) { return (const int32_t*)(up + Q.o_offs); }
__device__ __forceinline__ const int32_t* q_offs(const uint8_t*, const BowQueryStored& Q) { return Q.offs; }
__device__ __forceinline__ const uint32_t* q_feat(const uint8_t* up, const BowQuery& Q) { return (const uint32_t*)(up + Q.o_feat); }
__device__ __forceinline__ const uint32_t* q_feat(const uint8_t*, const BowQueryStored& Q) { return Q.feat; }
__device__ __forceinline__ float q_angle(const uint8_t* up, const BowQuery& Q, int i) { return ((const float*)(up + Q.o_angle))[i]; }
__device__ __forceinline__ float q_angle(const uint8_t*, const BowQueryStored& Q, int i) { return Q.kps[i].angle; }
__device__ __forceinline__ const uint8_t* q_desc(const uint8_t*, const BowQuerySlot& Q) { return Q.desc; }
__device__ __forceinline__ const uint32_t* q_nodes(const uint8_t*, const BowQuerySlot& Q) { return Q.nodes; }
__device__ __forceinline__ const int32_t* q_offs(const uint8_t*, const BowQuerySlot& Q) { return Q.offs; }
__device__ __forceinline__ const uint32_t* q_feat(const uint8_t*, const BowQuerySlot& Q) { return Q.feat; }
__device__ __forceinline__ float q_angle(const uint8_t*, const BowQuerySlot& Q, int i) { return Q.kps[i].angle; }
__device__ __forceinline__ int q_n_nodes(const BowQuery& Q) { return Q.n_nodes; }
__device__ __forceinline__ int q_n_nodes(const BowQueryStored& Q) { return Q.n_nodes; }
__device__ __forceinline__ int q_n_nodes(const BowQuerySlot& Q) { return *Q.n_nodes; }  // (written by the launch before)

// ORBMatcher.cc:212-231: which query features are no candidates
struct SkipQueryByMode {
  int mode;
  __device__ __forceinline__ bool operator()(uint8_t fl) const {
    return mode == ORBFE_BOW_TRACK ? (fl & ORBFE_TRI_GOOD) != 0 : mode == ORBFE_BOW_ADD ? (fl & 3) == 3 : false;
  }
};

template <class Q>
__global__ __launch_bounds__(256) void k_bow_match(const uint8_t* __restrict__ up, const BowKf* __restrict__ kfs, Q qr, BowParams P,
                                                   BowSlot* __restrict__ slots) {
  const int lane = threadIdx.x & 63;
  const BowKf& B = kfs[blockIdx.y];
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= B.n_feat) return;  // (the whole wave)
  BowSlot out = {-1, 0, 0, 0};
  const uint32_t pk = B.feat[j];
  const uint8_t fb = (up + B.o_flags)[pk];
  // ORBMatcher.cc:193-209: which keyframe features do not search
  const bool skip = P.mode == ORBFE_BOW_TRACK ? !(fb & ORBFE_TRI_GOOD) : P.mode == ORBFE_BOW_ADD ? (fb & 3) == 3 : false;
  int k = -1;
  const int qn_nodes = q_n_nodes(qr);
  if (!skip && qn_nodes > 0) {
    const uint32_t node = B.nodes[bow_entry_node(B.offs, B.n_nodes, j)];
    k = bow_find_node(q_nodes(up, qr), qn_nodes, node);
  }
  if (k >= 0) {
    const int32_t* oq = q_offs(up, qr);
    const uint8_t* kd = B.desc + (size_t)pk * 32;
    const uint4 a0 = *(const uint4*)kd, a1 = *(const uint4*)(kd + 16);
    Best2 b = {ORB_INT_MAX, ORB_INT_MAX, 0};
    const int ncand = bow_fold_node(b, a0, a1, q_feat(up, qr), oq[k], oq[k + 1], q_desc(up, qr), up + qr.o_flags, SkipQueryByMode{P.mode}, lane);
    const float ratio = (float)b.min_d / (float)b.second;
    if (ncand > 0 && !(b.min_d > P.dist_threshold || ratio > P.ratio)) {  // (0 / 0 is accepted, as in k_tri_match)
      out.q = b.min_idx;
      out.t = (int32_t)pk;
      out.d = b.min_d;
      if (P.check_orientation) out.bin = bow_angle_bin(q_angle(up, qr, b.min_idx), B.kps[pk].angle);
    }
  }
  if (lane == 0) slots[B.slot0 + j] = out;
}

#define BOW_SEL_WG 256

__global__ __launch_bounds__(BOW_SEL_WG) void k_bow_select(const BowKf* __restrict__ kfs, const BowSlot* __restrict__ slots,
                                                           BowMatch* __restrict__ lists, int32_t* __restrict__ counts) {
  __shared__ int32_t s_hist[BOW_ANGLE_BINS], s_base[BOW_ANGLE_BINS];
  __shared__ int32_t s_bin[BOW_ANGLE_CHOOSE];                  // the chosen bins, ascending (-1: fewer were chosen)
  __shared__ int32_t s_w[BOW_SEL_WG / 64][BOW_ANGLE_CHOOSE];   // per wave of a chunk: its matches in each chosen bin
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const BowKf& B = kfs[blockIdx.x];
  const BowSlot* S = slots + B.slot0;
  BowMatch* out = lists + B.slot0;
  const int n = B.n_feat;
  if (tid < BOW_ANGLE_BINS) s_hist[tid] = 0;
  __syncthreads();
  for (int s = tid; s < n; s += BOW_SEL_WG) {
    const BowSlot x = S[s];
    if (x.q >= 0) atomicAdd(&s_hist[x.bin], 1);  // (bow_angle_bin gives 0 .. 29)
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t chosen = bow_angle_choose(s_hist);
    int acc = 0, r = 0;
    for (int i = 0; i < BOW_ANGLE_BINS; ++i) {
      s_base[i] = acc;
      if ((chosen >> i) & 1u) {
        acc += s_hist[i];
        s_bin[r++] = i;
      }
    }
    for (; r < BOW_ANGLE_CHOOSE; ++r) s_bin[r] = -1;
    counts[blockIdx.x] = acc;
  }
  __syncthreads();
  const int c0 = s_bin[0], c1 = s_bin[1], c2 = s_bin[2];
  int run0 = 0, run1 = 0, run2 = 0;  // matches of each chosen bin in the chunks before this one
  for (int s0 = 0; s0 < n; s0 += BOW_SEL_WG) {
    const int s = s0 + tid;
    BowSlot x = {-1, 0, 0, -1};
    if (s < n) x = S[s];
    const bool ok = x.q >= 0;
    const unsigned long long m0 = __ballot(ok && x.bin == c0), m1 = __ballot(ok && x.bin == c1), m2 = __ballot(ok && x.bin == c2);
    if (lane == 0) s_w[w][0] = __popcll(m0), s_w[w][1] = __popcll(m1), s_w[w][2] = __popcll(m2);
    __syncthreads();
    int b0 = 0, b1 = 0, b2 = 0, t0 = 0, t1 = 0, t2 = 0;  // before this wave inside the chunk | the chunk's totals
#pragma unroll
    for (int u = 0; u < BOW_SEL_WG / 64; ++u) {
      const int v0 = s_w[u][0], v1 = s_w[u][1], v2 = s_w[u][2];
      if (u < w) b0 += v0, b1 += v1, b2 += v2;
      t0 += v0, t1 += v1, t2 += v2;
    }
    if (ok) {
      const unsigned long long below = (1ull << lane) - 1ull;
      int pos = -1;
      if (x.bin == c0) pos = s_base[c0] + run0 + b0 + __popcll(m0 & below);
      else if (x.bin == c1) pos = s_base[c1] + run1 + b1 + __popcll(m1 & below);
      else if (x.bin == c2) pos = s_base[c2] + run2 + b2 + __popcll(m2 & below);
      if (pos >= 0) out[pos] = {x.q, x.t, x.d};  // pos < the candidate's count <= n
    }
    run0 += t0, run1 += t1, run2 += t2;
    __syncthreads();  // s_w is rewritten by the next chunk
  }
}

__global__ __launch_bounds__(256) void k_bow_gather(const BowKf* __restrict__ kfs, BowParams P, const BowMatch* __restrict__ lists,
                                                    const int32_t* __restrict__ counts, int32_t* __restrict__ offsets,
                                                    BowMatch* __restrict__ matches) {
  __shared__ int32_t s_off[2];  // this candidate's first match | the total
  const int tid = threadIdx.x, k = blockIdx.x;
  if (tid < 64) {  // wave 0, all lanes: n_kf <= ORBFE_BOW_SEARCH_MAX_KF = 64 lengths
    const int v = tid < P.n_kf ? counts[tid] : 0;
    const int incl = wave_incl_scan_dpp<OpAddI>(v);
    if (k == 0) {
      if (tid == 0) offsets[0] = 0;
      if (tid < P.n_kf) offsets[tid + 1] = incl;
    }
    if (tid == k) s_off[0] = incl - v;
    if (tid == 63) s_off[1] = incl;
  }
  __syncthreads();
  if (s_off[1] > P.cap) return;  // ORBFE_ECAPACITY: the offsets only
  const BowMatch* src = lists + kfs[k].slot0;
  BowMatch* dst = matches + s_off[0];
  const int n = counts[k];
  for (int i = tid; i < n; i += 256) dst[i] = src[i];
}

template <class Q>
void launch_bow_search_t(hipStream_t st, const uint8_t* up, const BowKf* kfs, const Q& q, const BowParams& P, int max_feat, BowSlot* slots,
                         BowMatch* lists, int32_t* counts, int32_t* offsets, BowMatch* matches) {
  static_assert(ORBFE_BOW_SEARCH_MAX_KF <= 64, "k_bow_gather sums the lengths with one wave");
  if (max_feat > 0) k_bow_match<Q><<<dim3((max_feat + 3) / 4, P.n_kf), 256, 0, st>>>(up, kfs, q, P, slots);
  k_bow_select<<<P.n_kf, BOW_SEL_WG, 0, st>>>(kfs, slots, lists, counts);
  k_bow_gather<<<P.n_kf, 256, 0, st>>>(kfs, P, lists, counts, offsets, matches);
}

}  // namespace

void launch_bow_search(hipStream_t st, const uint8_t* up, const BowKf* kfs, const BowQuery& q, const BowParams& P, int max_feat, BowSlot* slots,
                       BowMatch* lists, int32_t* counts, int32_t* offsets, BowMatch* matches) {
  launch_bow_search_t(st, up, kfs, q, P, max_feat, slots, lists, counts, offsets, matches);
}
// one candidate, a frame in its slot: its list stays in `lists`, its length in counts[0] (no gather)
void launch_bow_search_one(hipStream_t st, const uint8_t* up, const BowKf* kf, const BowQuerySlot& q, const BowParams& P, int n_feat,
                           BowSlot* slots, BowMatch* lists, int32_t* counts) {
  if (n_feat > 0) k_bow_match<BowQuerySlot><<<dim3((n_feat + 3) / 4, 1), 256, 0, st>>>(up, kf, q, P, slots);
  k_bow_select<<<1, BOW_SEL_WG, 0, st>>>(kf, slots, lists, counts);
}
void launch_bow_search(hipStream_t st, const uint8_t* up, const BowKf* kfs, const BowQueryStored& q, const BowParams& P, int max_feat,
                       BowSlot* slots, BowMatch* lists, int32_t* counts, int32_t* offsets, BowMatch* matches) {
  launch_bow_search_t(st, up, kfs, q, P, max_feat, slots, lists, counts, offsets, matches);
}
