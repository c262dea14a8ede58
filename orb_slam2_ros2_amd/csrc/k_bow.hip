// k_bow.hip -- DBoW2 / DBoW3 TemplatedVocabulary::transform(features, v, fv, levelsup) for binary (ORB) features under L1 scoring and
// TF-IDF weighting, on gfx950.  Host side: orbfe_bow.hip.  The rules, bit-exact (tests/bow_restatement.py restates them in numpy):
//   1. descent    from the root, its children being level 1; at each node the Hamming-256 distance to every child in FILE order, the first
//                 minimum (strict <: a tie goes to the earliest child); stop at a leaf
//   2. node       the node the path passes at level nid_level = L - levelsup, the root if nid_level <= 0.  DBoW leaves the node unset when the
//                 leaf comes before nid_level (undefined behaviour); the decision here: the feature's node is that leaf
//   3. skip       a feature whose leaf weight is not > 0 adds nothing (DBoW's `if (w > 0)`): no BowVector entry, no FeatureVector entry
//   4. BowVector  words ascending; a word hit c times holds w + w + .. + w (c terms in sequence: BowVector::addWeight, not c * w); then L1:
//                 norm = the sequential double sum of |value| in ascending word order, value = value / norm (a division) when norm > 0
//   5. FeatureVector  nodes ascending, each node's feature indices ascending (fv.addFeature in feature order)
//
// Two launches.  k_bow_descend: a group of 16 lanes per descriptor; lane j takes children j and j + 16 of the current node (the children of a
// node are ONE contiguous block of 32-byte descriptors, orbfe_bow.hip), the group's minimum of (distance << 8 | child) is the first-minimum
// argmin.  It writes per feature the sort keys word << 16 | feature and node << 16 | feature (all ones: skipped) and the leaf weight.
// k_bow_group: one workgroup per image sorts both key lists (bitonic; in LDS up to 2048 keys, in the image's global key buffer above),
// marks run heads, compacts them with a workgroup scan and writes both CSRs; the L1 norm is one lane's sequential sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbfe_internal.h"
#include "wave_ops.h"

using namespace orbfe;

#define BOW_DESC_WG 256                        // k_bow_descend: 16 groups of 16 lanes = 16 descriptors per workgroup
#define BOW_GROUP_WG 1024                      // k_bow_group: threads per image
#define BOW_LDS_KEYS 2048                      // images of up to this many features sort in LDS
#define BOW_NONE 0xFFFFFFFFFFFFFFFFull         // a skipped feature / padding: sorts behind every real key

__global__ __launch_bounds__(BOW_DESC_WG) void k_bow_descend(const uint8_t* __restrict__ desc, size_t desc_img_stride, const int32_t* __restrict__ counts, int count_step,
                                                             int n_fixed, const BowChild* __restrict__ rec, const uint4* __restrict__ cdesc,
                                                             const double* __restrict__ cw, int root_first, int root_nc, int L, int nid_level,
                                                             uint64_t* __restrict__ wkey, uint64_t* __restrict__ nkey, double* __restrict__ wts,
                                                             size_t key_stride) {
  const int img = blockIdx.y;
  const int j = threadIdx.x & 15;
  const int f = blockIdx.x * (BOW_DESC_WG / 16) + (threadIdx.x >> 4);
  const int n = counts ? counts[(size_t)img * count_step] : n_fixed;
  const bool active = f < n;
  uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
  if (active) {
    const uint4* fd = (const uint4*)(desc + ((size_t)img * desc_img_stride + (size_t)f) * 32);
    a0 = fd[0];
    a1 = fd[1];
  }
  bool done = !active;
  int first = root_first, nc = root_nc, level = 0, leaf = -1;
  uint32_t nid = nid_level <= 0 ? 0u : 0xFFFFFFFFu;
  // L trips for every lane (the shuffles need the whole wave); a group that has reached its leaf idles
  for (int it = 0; it < L; ++it) {
    uint32_t key = 0xFFFFFFFFu;
    if (!done) {
      for (int ch = j; ch < nc; ch += 16) {
        const uint4 b0 = cdesc[2 * (size_t)(first + ch)], b1 = cdesc[2 * (size_t)(first + ch) + 1];
        const uint32_t d = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
                           __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
        key = min(key, (d << 8) | (uint32_t)ch);
      }
    }
    key = min(key, (uint32_t)__shfl_xor((int)key, 8));
    key = min(key, (uint32_t)__shfl_xor((int)key, 4));
    key = min(key, (uint32_t)__shfl_xor((int)key, 2));
    key = min(key, (uint32_t)__shfl_xor((int)key, 1));
    if (!done) {
      const int p = first + (int)(key & 0xFFu);
      const BowChild r = rec[p];
      ++level;
      if (level == nid_level) nid = r.node;
      if (r.nc == 0) {
        done = true;
        leaf = p;
      } else {
        first = r.first;
        nc = r.nc;
      }
    }
  }
  if (active && j == 0) {
    const BowChild r = rec[leaf];
    const double w = cw[leaf];
    if (nid == 0xFFFFFFFFu) nid = r.node;  // rule 2: the leaf came before nid_level
    const size_t o = (size_t)img * key_stride + (size_t)f;
    const bool keep = w > 0.0;
    wkey[o] = keep ? (((uint64_t)r.word << 16) | (uint64_t)f) : BOW_NONE;
    nkey[o] = keep ? (((uint64_t)nid << 16) | (uint64_t)f) : BOW_NONE;
    wts[o] = w;
  }
}

// exclusive scan of one int per thread over the workgroup; `tot` receives the total.  All threads must call it.
__device__ __forceinline__ int wg_excl_scan(int v, int* s_wave, int& tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_incl_scan_dpp<OpAddI>(v);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int base = 0, sum = 0;
  for (int w = 0; w < BOW_GROUP_WG / 64; ++w) {
    const int t = s_wave[w];
    base += w < wave ? t : 0;
    sum += t;
  }
  tot = sum;
  __syncthreads();  // s_wave is reused by the next call
  return base + incl - v;
}

// The body of k_bow_group over one image, instantiated twice: on LDS arrays (up to BOW_LDS_KEYS keys) and in place on the image's global key
// buffers.  Never on a pointer that may be either: a flat pointer into LDS plus the loop's index - 1 made the compiler address K[-1] as a base
// with an immediate offset of +8, and the flat aperture check (on the base, before the offset) faulted.
template <bool IN_LDS>
__device__ __forceinline__ void bow_group_body(uint64_t* W, uint64_t* K, double* V, const uint64_t* gw,
                                               const uint64_t* gn, const double* __restrict__ wts, int n, int N, uint32_t* __restrict__ words,
                                               double* values, uint32_t* __restrict__ nodes, int32_t* __restrict__ offsets,
                                               uint32_t* __restrict__ features, int32_t* __restrict__ o_counts, int* s_wave, double* s_norm) {
  const int t = threadIdx.x;
  for (int i = t; i < N; i += BOW_GROUP_WG) {
    const uint64_t a = i < n ? gw[i] : BOW_NONE, b = i < n ? gn[i] : BOW_NONE;
    W[i] = a;
    K[i] = b;
  }
  __syncthreads();
  // bitonic sort of both lists, ascending
  for (int k = 2; k <= N; k <<= 1) {
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int i = t; i < N; i += BOW_GROUP_WG) {
        const int ix = i ^ s;
        if (ix > i) {
          const bool up = (i & k) == 0;
          const uint64_t a = W[i], b = W[ix];
          if ((a > b) == up) {
            W[i] = b;
            W[ix] = a;
          }
          const uint64_t c = K[i], d = K[ix];
          if ((c > d) == up) {
            K[i] = d;
            K[ix] = c;
          }
        }
      }
      __syncthreads();
    }
  }
  // run heads: thread t owns the consecutive keys [t C, t C + C)
  const int C = (N + BOW_GROUP_WG - 1) / BOW_GROUP_WG;
  const int i0 = min(t * C, N), i1 = min(i0 + C, N);
  int cw = 0, cn = 0, cv = 0;
  for (int i = i0; i < i1; ++i) {
    const uint64_t a = W[i], b = K[i];
    cw += a != BOW_NONE && (i == 0 || (W[i - 1] >> 16) != (a >> 16));
    cn += b != BOW_NONE && (i == 0 || (K[i - 1] >> 16) != (b >> 16));
    cv += b != BOW_NONE;
  }
  int n_words, n_nodes, n_kept;
  int uw = wg_excl_scan(cw, s_wave, n_words);
  int un = wg_excl_scan(cn, s_wave, n_nodes);
  (void)wg_excl_scan(cv, s_wave, n_kept);
  for (int i = i0; i < i1; ++i) {
    const uint64_t a = W[i], b = K[i];
    if (a != BOW_NONE && (i == 0 || (W[i - 1] >> 16) != (a >> 16))) {
      // rule 4: w + w + .. + w over the run, in sequence (the run's keys differ only in the feature index)
      double v = 0.0;
      for (int q = i; q < N && (W[q] >> 16) == (a >> 16); ++q) v += wts[(uint32_t)(W[q] & 0xFFFFu)];
      words[uw] = (uint32_t)(a >> 16);
      V[uw] = v;
      ++uw;
    }
    if (b != BOW_NONE) {
      if (i == 0 || (K[i - 1] >> 16) != (b >> 16)) {
        nodes[un] = (uint32_t)(b >> 16);
        offsets[un] = i;
        ++un;
      }
      features[i] = (uint32_t)(b & 0xFFFFu);
    }
  }
  __syncthreads();
  if (t == 0) {
    // the L1 norm: ONE lane, ascending word order, eight loads in flight ahead of eight dependent adds
    double s = 0.0;
    int u = 0;
    for (; u + 8 <= n_words; u += 8) {
      const double v0 = V[u], v1 = V[u + 1], v2 = V[u + 2], v3 = V[u + 3], v4 = V[u + 4], v5 = V[u + 5], v6 = V[u + 6], v7 = V[u + 7];
      s += fabs(v0);
      s += fabs(v1);
      s += fabs(v2);
      s += fabs(v3);
      s += fabs(v4);
      s += fabs(v5);
      s += fabs(v6);
      s += fabs(v7);
    }
    for (; u < n_words; ++u) s += fabs(V[u]);
    *s_norm = s;
    offsets[n_nodes] = n_kept;
    o_counts[0] = n_words;
    o_counts[1] = n_nodes;
  }
  __syncthreads();
  const double norm = *s_norm;
  for (int u = t; u < n_words; u += BOW_GROUP_WG) {
    const double v = V[u];
    values[u] = norm > 0.0 ? v / norm : v;
  }
}

__global__ __launch_bounds__(BOW_GROUP_WG) void k_bow_group(uint64_t* __restrict__ wkey_g, uint64_t* __restrict__ nkey_g, const double* __restrict__ wts_g,
                                                            size_t key_stride, const int32_t* __restrict__ counts, int count_step, int n_fixed, size_t cap,
                                                            uint32_t* __restrict__ o_words, double* __restrict__ o_values, uint32_t* __restrict__ o_nodes,
                                                            int32_t* __restrict__ o_offsets, uint32_t* __restrict__ o_features, int32_t* __restrict__ o_counts) {
  __shared__ uint64_t s_w[BOW_LDS_KEYS], s_n[BOW_LDS_KEYS];
  __shared__ double s_v[BOW_LDS_KEYS];
  __shared__ int s_wave[BOW_GROUP_WG / 64];
  __shared__ double s_norm;
  const int img = blockIdx.x;
  const int n = counts ? counts[(size_t)img * count_step] : n_fixed;
  int N = 1;
  while (N < n) N <<= 1;
  uint64_t* gw = wkey_g + (size_t)img * key_stride;
  uint64_t* gn = nkey_g + (size_t)img * key_stride;
  const double* wts = wts_g + (size_t)img * key_stride;
  uint32_t* words = o_words + (size_t)img * cap;
  double* values = o_values + (size_t)img * cap;
  uint32_t* nodes = o_nodes + (size_t)img * cap;
  int32_t* offsets = o_offsets + (size_t)img * (cap + 1);
  uint32_t* features = o_features + (size_t)img * cap;
  // small images sort in LDS; larger ones in place in their global key buffers (key_stride >= N), the slower exact path
  if (N <= BOW_LDS_KEYS)
    bow_group_body<true>(s_w, s_n, s_v, gw, gn, wts, n, N, words, values, nodes, offsets, features, o_counts + 2 * img, s_wave, &s_norm);
  else
    bow_group_body<false>(gw, gn, values, gw, gn, wts, n, N, words, values, nodes, offsets, features, o_counts + 2 * img, s_wave, &s_norm);
}

void launch_bow(hipStream_t s, const uint8_t* d_desc, size_t desc_img_stride, const int32_t* d_counts, int count_step, int n_fixed, int n_img, int cap,
                const BowVocabDev& vd, int levelsup, uint64_t* d_wkey, uint64_t* d_nkey, double* d_wts, size_t key_stride, uint32_t* o_words,
                double* o_values, uint32_t* o_nodes, int32_t* o_offsets, uint32_t* o_features, int32_t* o_counts) {
  const int per_wg = BOW_DESC_WG / 16;
  // levelsup is any int >= 0: L - levelsup stays far from overflow for the levels a vocabulary has (<= 10)
  const int nid_level = levelsup > vd.L ? 0 : vd.L - levelsup;
  if (cap > 0) {
    dim3 g((unsigned)((cap + per_wg - 1) / per_wg), (unsigned)n_img);
    hipLaunchKernelGGL(k_bow_descend, g, dim3(BOW_DESC_WG), 0, s, d_desc, desc_img_stride, d_counts, count_step, n_fixed, vd.rec, vd.desc, vd.weight,
                       vd.root_first, vd.root_nc, vd.L, nid_level, d_wkey, d_nkey, d_wts, key_stride);
  }
  hipLaunchKernelGGL(k_bow_group, dim3((unsigned)n_img), dim3(BOW_GROUP_WG), 0, s, d_wkey, d_nkey, d_wts, key_stride, d_counts, count_step, n_fixed,
                     (size_t)cap, o_words, o_values, o_nodes, o_offsets, o_features, o_counts);
}
