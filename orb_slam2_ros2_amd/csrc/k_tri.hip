// k_tri.hip -- LocalMapping::createNewMapPoints (src/LocalMapping.cc:165-285) for one current keyframe and its neighbours.
//
// k_tri_match    one wave per (neighbour, FeatureVector entry j): the entry's node in the current keyframe's FeatureVector, the
//                bAddMPs filters, getBestMatch over the node's current features (bow_walk.h, match_fold.h), the threshold / ratio test
//                (searchByBow, ORBMatcher.cc:170-253), the mutual epipolar test (searchForTriangulation, :736-793), then the parallax
//                cosines, the three-way branch, triangulate / unProject and checkMapPoint.  Out: one TriSlot per entry; a slot that
//                can change the map state counts itself for its current feature.
// k_tri_scan     one workgroup: the per-feature counts -> offsets.
// k_tri_fill     the slots into per-feature lists (any order).
// k_tri_resolve  one thread per current feature: its list sorted by slot (= neighbour, then match order), walked with the reference's
//                state (T4: first accepted wins; T5: the own-stereo branch consumes the unprocessed point), then the tail flag (T6).
// k_tri_compact  one workgroup: the accepted slots in slot order -> records, the tail flags in feature order -> the tail list.
//
// Numerics (restated in tests/triangulation_restatement.py, which this file must equal bit for bit): no contraction; float
// products summed left to right; dots and norms in double; the SVD decision: Jacobi eigen-decomposition of A^T A in double (jacobi_dev.h).
#include <hip/hip_runtime.h>

#include "bow_walk.h"
#include "orbfe_internal.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace {

using namespace orbfe;

#include "jacobi_dev.h"

#define TRI_MIN_TH 50    // ORBMatcher::mnMinThreshold
#define TRI_RATIO 0.6f   // ORBMatcher(0.6f, false)
#define TRI_SCAN_WG 1024

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ V3 matvec(const float* R, int ld, V3 v) {  // rows of R (stride ld), left to right in float
  return {R[0] * v.x + R[1] * v.y + R[2] * v.z, R[ld] * v.x + R[ld + 1] * v.y + R[ld + 2] * v.z,
          R[2 * ld] * v.x + R[2 * ld + 1] * v.y + R[2 * ld + 2] * v.z};
}
__device__ __forceinline__ V3 matTvec(const float* R, int ld, V3 v) {  // R^T v
  return {R[0] * v.x + R[ld] * v.y + R[2 * ld] * v.z, R[1] * v.x + R[ld + 1] * v.y + R[2 * ld + 1] * v.z,
          R[2] * v.x + R[ld + 2] * v.y + R[2 * ld + 2] * v.z};
}
// R p + t of a row-major 4x4 pose: the product in float, the shift as (float)((double)sum + (double)t)
__device__ __forceinline__ V3 affine(const float* T, V3 p) {
  const V3 s = matvec(T, 4, p);
  return {(float)((double)s.x + (double)T[3]), (float)((double)s.y + (double)T[7]), (float)((double)s.z + (double)T[11])};
}
__device__ __forceinline__ double dot3(V3 a, V3 b) { return (double)a.x * (double)b.x + (double)a.y * (double)b.y + (double)a.z * (double)b.z; }
__device__ __forceinline__ double norm3(V3 a) { return sqrt(dot3(a, a)); }

// computeCosTheta (LocalMapping.cc:290-299); R == nullptr: the identity (I^T v == v up to the sign of a zero, which no result sees)
__device__ __forceinline__ float cos_theta(const float* R1, const float* R2, float p1x, float p1y, float p2x, float p2y, const TriParams& P) {
  const V3 v1 = {(p1x - P.cx) / P.fx, (p1y - P.cy) / P.fy, 1.f}, v2 = {(p2x - P.cx) / P.fx, (p2y - P.cy) / P.fy, 1.f};
  const V3 w1 = R1 ? matTvec(R1, 4, v1) : v1, w2 = R2 ? matTvec(R2, 4, v2) : v2;
  return (float)(dot3(w1, w2) / (norm3(w1) * norm3(w2)));
}

// MapPoint::checkMapPoint (MapPoint.cc:384-420), quirk T1: the second error uses kp1.y
__device__ __forceinline__ bool check_map_point(V3 p, const float* T1, const float* T2, const orbfe_keypoint& k1, const orbfe_keypoint& k2, const float* sf,
                                const TriParams& P) {
  const float s1 = sf[k1.octave], s2 = sf[k2.octave];
  const float l21 = s1 * s1, l22 = s2 * s2;
  const V3 c1 = affine(T1, p), c2 = affine(T2, p);
  if (c1.z <= 0 || c2.z <= 0) return false;
  const float u1 = c1.x / c1.z * P.fx + P.cx, v1 = c1.y / c1.z * P.fy + P.cy;
  const float u2 = c2.x / c2.z * P.fx + P.cx, v2 = c2.y / c2.z * P.fy + P.cy;
  const double a1 = (double)(k1.x - u1), b1 = (double)(k1.y - v1), a2 = (double)(k2.x - u2), b2 = (double)(k1.y - v2);
  const float e1 = (float)(a1 * a1 + b1 * b1), e2 = (float)(a2 * a2 + b2 * b2);
  if ((double)e1 > 5.991 * (double)l21 || (double)e2 > 5.991 * (double)l22) return false;
  const float dis = (float)(norm3(c1) / norm3(c2));
  const float py = s1 / s2;
  if ((double)dis > (double)py * 1.5 || (double)dis < (double)py / 1.5) return false;
  return true;
}

// triangulate (LocalMapping.cc:311-339) under the SVD decision: false when w3 / w2 > 1e-3 or world z < 0 (T9)
__device__ __forceinline__ bool triangulate(const float* T1, const float* T2, const orbfe_keypoint& k1, const orbfe_keypoint& k2, const TriParams& P, V3& out) {
  float A[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float* T = r < 2 ? T1 : T2;
    const orbfe_keypoint& kp = r < 2 ? k1 : k2;
    const int row = r & 1;
    const float f = row ? P.fy : P.fx;
    const float b = (row ? P.cy : P.cx) - (row ? kp.y : kp.x);
#pragma unroll
    for (int j = 0; j < 4; ++j) A[r][j] = f * T[4 * row + j] + b * T[8 + j];
  }
  double N[4][4], V[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double acc = (double)A[0][i] * (double)A[0][j];
#pragma unroll
      for (int k = 1; k < 4; ++k) acc = acc + (double)A[k][i] * (double)A[k][j];
      N[i][j] = acc;
    }
  jacobi_small<4>(N, V);
  // the smallest and the second smallest eigenvalue (first strict minima in index order), selects instead of variable indices
  double w0 = N[0][0], w1 = N[1][1], w2 = N[2][2], w3 = N[3][3];
  int m = 0;
  double wm = w0;
  if (w1 < wm) m = 1, wm = w1;
  if (w2 < wm) m = 2, wm = w2;
  if (w3 < wm) m = 3, wm = w3;
  int s = -1;
  double ws = 0;
  if (m != 0) s = 0, ws = w0;
  if (m != 1 && (s < 0 || w1 < ws)) s = 1, ws = w1;
  if (m != 2 && (s < 0 || w2 < ws)) s = 2, ws = w2;
  if (m != 3 && (s < 0 || w3 < ws)) s = 3, ws = w3;
  const float sv3 = (float)sqrt(wm > 0 ? wm : 0.0), sv2 = (float)sqrt(ws > 0 ? ws : 0.0);
  if ((double)(sv3 / sv2) > 1e-3) return false;
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (float)(m == 0 ? V[i][0] : m == 1 ? V[i][1] : m == 2 ? V[i][2] : V[i][3]);
  const double inv = 1.0 / (double)v[3];
  out = {(float)((double)v[0] * inv), (float)((double)v[1] * inv), (float)((double)v[2] * inv)};
  return !(out.z < 0);
}

__device__ __forceinline__ void mul33(const float* A, const float* B, float* C) {  // C = A B, 3x3 row-major, left to right
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void mul44(const float* A, const float* B, float* C) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) C[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j] + A[4 * i + 3] * B[12 + j];
}
// F = KInv^T [t]x R KInv of T (matcher_ext.epipolarFilter)
__device__ __forceinline__ void fundamental(const float* T, const TriParams& P, float* F) {
  const float x = T[3], y = T[7], z = T[11];
  const float ssm[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
  const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
  const float KT[9] = {P.kinv[0], P.kinv[3], P.kinv[6], P.kinv[1], P.kinv[4], P.kinv[7], P.kinv[2], P.kinv[5], P.kinv[8]};
  float a[9], b[9];
  mul33(KT, ssm, a);
  mul33(a, R, b);
  mul33(b, P.kinv, F);
}
// point2LineDistance(pl^T F, p) (ORBMatcher.cc:789-795)
__device__ __forceinline__ float line_dist(float lx, float ly, const float* F, float px, float py) {
  float prm[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) prm[j] = lx * F[j] + ly * F[3 + j] + 1.f * F[6 + j];
  const double dot = (double)prm[0] * (double)px + (double)prm[1] * (double)py + (double)prm[2] * 1.0;
  return (float)fabs(dot) / sqrtf(prm[0] * prm[0] + prm[1] * prm[1]);
}

// Where a keyframe's own arrays are: behind the call's upload (TriKf: orbfe_create_new_map_points) or where the keyframe store keeps
// them (TriKfStored: orbfe_create_new_map_points_stored).  The kernels are templates over the record and otherwise ONE text; the flags,
// the unprocessed points and the scale factors are in the upload in both forms.
#define TRI_KF_ARRAY(name, T, off, ptr)                                                                               \
  __device__ __forceinline__ const T* name(const uint8_t* up, const TriKf& K) { return (const T*)(up + K.off); }      \
  __device__ __forceinline__ const T* name(const uint8_t*, const TriKfStored& K) { return (const T*)K.ptr; }
TRI_KF_ARRAY(kf_kps, orbfe_keypoint, o_kps, kps)
TRI_KF_ARRAY(kf_desc, uint8_t, o_desc, desc)
TRI_KF_ARRAY(kf_nodes, uint32_t, o_nodes, nodes)
TRI_KF_ARRAY(kf_offs, int32_t, o_offs, offs)
TRI_KF_ARRAY(kf_feat, uint32_t, o_feat, feat)
TRI_KF_ARRAY(kf_depth, double, o_depth, depth)
TRI_KF_ARRAY(kf_ru, double, o_ru, ru)
#undef TRI_KF_ARRAY

template <class KF>
__global__ __launch_bounds__(256) void k_tri_match(const uint8_t* __restrict__ up, const KF* __restrict__ kfs, TriParams P,
                                                   TriSlot* __restrict__ slots, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int nbi = blockIdx.y;
  const KF& C = kfs[0];
  const KF& B = kfs[1 + nbi];
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= B.n_feat) return;
  TriSlot out = {-1, 0, nbi, 0, 0, {0.f, 0.f, 0.f}};
  const uint8_t* fl_c = up + C.o_flags;
  const uint8_t* fl_b = up + B.o_flags;
  const uint32_t pk = kf_feat(up, B)[j];
  int k = -1;
  if (!B.skip && (fl_b[pk] & 3) != 3) {
    const uint32_t node = kf_nodes(up, B)[bow_entry_node(kf_offs(up, B), B.n_nodes, j)];
    k = bow_find_node(kf_nodes(up, C), C.n_nodes, node);
  }
  if (k >= 0) {
    const int32_t* oc = kf_offs(up, C);
    const uint32_t* fc = kf_feat(up, C);
    const uint8_t* dc = kf_desc(up, C);
    const uint8_t* qd = kf_desc(up, B) + (size_t)pk * 32;
    const uint4 a0 = *(const uint4*)qd, a1 = *(const uint4*)(qd + 16);
    const int begin = oc[k], end = oc[k + 1];
    Best2 b = {ORB_INT_MAX, ORB_INT_MAX, 0};
    // bAddMPs: current features with a good in-map point are no candidates
    const int ncand = bow_fold_node(b, a0, a1, fc, begin, end, dc, fl_c, SkipGoodInMap(), lane);
    const float ratio = (float)b.min_d / (float)b.second;
    if (ncand > 0 && !(b.min_d > TRI_MIN_TH || ratio > TRI_RATIO)) {
      const int q = b.min_idx;
      const orbfe_keypoint k1 = kf_kps(up, C)[q];
      const orbfe_keypoint k2 = kf_kps(up, B)[pk];
      const float* sf = (const float*)(up + P.o_sf);
      // the mutual epipolar test
      float T21[16], T12[16], F21[9], F12[9];
      mul44(B.Tcw, C.Twc, T21);
      mul44(C.Tcw, B.Twc, T12);
      fundamental(T21, P, F21);
      fundamental(T12, P, F12);
      const float s1 = sf[k1.octave], s2 = sf[k2.octave];
      const float th1 = (float)(5.991 * (double)(s1 * s1)), th2 = (float)(5.991 * (double)(s2 * s2));
      if (!(line_dist(k2.x, k2.y, F21, k1.x, k1.y) > th1) && !(line_dist(k1.x, k1.y, F12, k2.x, k2.y) > th2)) {
        out.q = q;
        out.t = (int32_t)pk;
        const double dep1 = kf_depth(up, C)[q], dep2 = kf_depth(up, B)[pk];
        const float c0 = cos_theta(C.Tcw, B.Tcw, k1.x, k1.y, k2.x, k2.y, P);
        float c1 = 1.f, c2 = 1.f;
        const bool st1 = dep1 > 0, st2 = dep2 > 0;
        if (st1) c1 = cos_theta(nullptr, nullptr, k1.x, k1.y, (float)kf_ru(up, C)[q], k1.y, P);
        if (st2) c2 = cos_theta(nullptr, nullptr, k2.x, k2.y, (float)kf_ru(up, B)[pk], k2.y, P);
        const float cst = c2 < c1 ? c2 : c1;  // std::min(c1, c2)
        V3 p = {0.f, 0.f, 0.f};
        if (c0 < cst && c0 > 0 && (st1 || st2 || (double)c0 < 0.9998)) {
          if (triangulate(C.Tcw, B.Tcw, k1, k2, P, p)) {
            out.kind = ORBFE_TRI_TRIANGULATED;
            out.ok = check_map_point(p, C.Tcw, B.Tcw, k1, k2, sf, P);
          }
        } else if (st1 && c1 < c2) {
          const float* up3 = (const float*)(up + P.o_upos) + (size_t)q * 3;
          p = {up3[0], up3[1], up3[2]};
          out.kind = ORBFE_TRI_OWN_STEREO;
          out.ok = check_map_point(p, C.Tcw, B.Tcw, k1, k2, sf, P);
        } else if (st2 && c2 < c1) {
          const float x = (k2.x - P.cx) / P.fx, y = (k2.y - P.cy) / P.fy;
          const V3 pc = {(float)(dep2 * (double)x), (float)(dep2 * (double)y), (float)dep2};
          p = affine(B.Twc, pc);
          out.kind = ORBFE_TRI_NB_STEREO;
          out.ok = check_map_point(p, C.Tcw, B.Tcw, k1, k2, sf, P);
        }
        out.xyz[0] = p.x, out.xyz[1] = p.y, out.xyz[2] = p.z;
      }
    }
  }
  if (lane == 0) {
    slots[B.slot0 + j] = out;
    if (out.kind) atomicAdd(&cnt[out.q], 1);
  }
}

// exclusive scan of v[0 .. n) by one workgroup of TRI_SCAN_WG threads into off[0 .. n] (off[n] = total)
__device__ __forceinline__ void block_scan(const int32_t* v, int n, int32_t* off, int32_t* s_w) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int carry = 0;
  for (int b0 = 0; b0 < n; b0 += TRI_SCAN_WG) {
    const int i = b0 + tid;
    const int x = i < n ? v[i] : 0;
    const int incl = wave_incl_scan_dpp<OpAddI>(x);
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    int before = carry;
    for (int u = 0; u < w; ++u) before += s_w[u];
    if (i < n) off[i] = before + incl - x;
    int tot = 0;
    for (int u = 0; u < TRI_SCAN_WG / 64; ++u) tot += s_w[u];
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) off[n] = carry;
}

__global__ __launch_bounds__(TRI_SCAN_WG) void k_tri_scan(const int32_t* __restrict__ cnt, int n, int32_t* __restrict__ off) {
  __shared__ int32_t s_w[TRI_SCAN_WG / 64];
  block_scan(cnt, n, off, s_w);
}

__global__ __launch_bounds__(256) void k_tri_fill(const TriSlot* __restrict__ slots, int n_slots, const int32_t* __restrict__ off,
                                                  int32_t* __restrict__ fill, int32_t* __restrict__ list) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_slots) return;
  const TriSlot x = slots[s];
  if (!x.kind) return;
  const int pos = atomicAdd(&fill[x.q], 1);
  list[off[x.q] + pos] = s;
}

template <class KF>
__global__ __launch_bounds__(256) void k_tri_resolve(const uint8_t* __restrict__ up, const KF* __restrict__ kfs, TriParams P,
                                                     const TriSlot* __restrict__ slots, const int32_t* __restrict__ off,
                                                     int32_t* __restrict__ list, int32_t* __restrict__ acc, int32_t* __restrict__ tail_flag,
                                                     uint8_t* __restrict__ consumed) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= P.n_cur) return;
  const int b = off[q], e = off[q + 1];
  for (int i = b + 1; i < e; ++i) {  // insertion sort: the slot order is neighbour order, then match order
    const int x = list[i];
    int k = i - 1;
    while (k >= b && list[k] > x) {
      list[k + 1] = list[k];
      --k;
    }
    list[k + 1] = x;
  }
  bool unproc = up[P.o_unproc + q] != 0, assigned = false;
  for (int i = b; i < e && !assigned; ++i) {
    const int s = list[i];
    const TriSlot x = slots[s];
    if (x.kind == ORBFE_TRI_OWN_STEREO) {
      if (!unproc) continue;
      unproc = false;  // consumed, accepted or not (T5)
    }
    if (x.ok) {
      assigned = true;
      acc[s] = 1;
    }
  }
  const uint8_t good = (up + kfs[0].o_flags)[q] & ORBFE_TRI_GOOD;
  tail_flag[q] = (unproc && !assigned && !good) ? 1 : 0;  // T6
  consumed[q] = (up[P.o_unproc + q] != 0 && !unproc) ? 1 : 0;
}

__global__ __launch_bounds__(TRI_SCAN_WG) void k_tri_compact(TriParams P, const TriSlot* __restrict__ slots,
                                                             int32_t* __restrict__ acc, int32_t* __restrict__ tail_flag, int32_t* __restrict__ pos,
                                                             int32_t* __restrict__ hdr, TriRec* __restrict__ recs, int32_t* __restrict__ tail) {
  __shared__ int32_t s_w[TRI_SCAN_WG / 64];
  block_scan(acc, P.n_slots, pos, s_w);
  __syncthreads();
  for (int s = threadIdx.x; s < P.n_slots; s += TRI_SCAN_WG) {
    if (!acc[s] || pos[s] >= P.rec_cap) continue;
    const TriSlot x = slots[s];
    TriRec r;
    r.nb = x.nb;
    r.q = x.q;
    r.t = x.t;
    r.kind = x.kind;
    r.xyz[0] = x.xyz[0], r.xyz[1] = x.xyz[1], r.xyz[2] = x.xyz[2];
    recs[pos[s]] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) hdr[0] = pos[P.n_slots];
  __syncthreads();
  block_scan(tail_flag, P.n_cur, pos, s_w);
  __syncthreads();
  for (int q = threadIdx.x; q < P.n_cur; q += TRI_SCAN_WG)
    if (tail_flag[q] && pos[q] < P.tail_cap) tail[pos[q]] = q;
  if (threadIdx.x == 0) hdr[1] = pos[P.n_cur];
}

template <class KF>
void launch_tri_t(hipStream_t st, const uint8_t* up, const KF* kfs, const TriParams& P, int max_feat, TriSlot* slots, int32_t* cnt, int32_t* off,
                  int32_t* fill, int32_t* list, int32_t* acc, int32_t* tail_flag, int32_t* pos, int32_t* hdr, TriRec* recs, int32_t* tail,
                  uint8_t* consumed) {
  if (P.n_nb > 0 && max_feat > 0) k_tri_match<KF><<<dim3((max_feat + 3) / 4, P.n_nb), 256, 0, st>>>(up, kfs, P, slots, cnt);
  k_tri_scan<<<1, TRI_SCAN_WG, 0, st>>>(cnt, P.n_cur, off);
  if (P.n_slots > 0) k_tri_fill<<<(P.n_slots + 255) / 256, 256, 0, st>>>(slots, P.n_slots, off, fill, list);
  if (P.n_cur > 0) k_tri_resolve<KF><<<(P.n_cur + 255) / 256, 256, 0, st>>>(up, kfs, P, slots, off, list, acc, tail_flag, consumed);
  k_tri_compact<<<1, TRI_SCAN_WG, 0, st>>>(P, slots, acc, tail_flag, pos, hdr, recs, tail);
}

}  // namespace

void launch_tri(hipStream_t st, const uint8_t* up, const TriKf* kfs, const TriParams& P, int max_feat, TriSlot* slots, int32_t* cnt,
                int32_t* off, int32_t* fill, int32_t* list, int32_t* acc, int32_t* tail_flag, int32_t* pos, int32_t* hdr, TriRec* recs,
                int32_t* tail, uint8_t* consumed) {
  launch_tri_t(st, up, kfs, P, max_feat, slots, cnt, off, fill, list, acc, tail_flag, pos, hdr, recs, tail, consumed);
}
void launch_tri(hipStream_t st, const uint8_t* up, const TriKfStored* kfs, const TriParams& P, int max_feat, TriSlot* slots, int32_t* cnt,
                int32_t* off, int32_t* fill, int32_t* list, int32_t* acc, int32_t* tail_flag, int32_t* pos, int32_t* hdr, TriRec* recs,
                int32_t* tail, uint8_t* consumed) {
  launch_tri_t(st, up, kfs, P, max_feat, slots, cnt, off, fill, list, acc, tail_flag, pos, hdr, recs, tail, consumed);
}
