// k_mpstore.hip -- the two kernels of the map-point store (orbfe_mpstore.hip).
//
// k_mpstore_gather   rows of the listed ids -> the arrays orbfe_track_local_map's launches read (pos, view_dir, max_dist, min_dist, desc).
//                    The one launch orbfe_track_local_map_stored puts in front of the chain, and orbfe_mpstore_fetch's only one.
// k_mpstore_scatter  the fields of an upsert -> the rows of the listed ids, and their presence bytes (erase: presence bytes only).
//
// Both: four lanes per point, one 16-byte quarter of the 64-byte row each -- [pos.xyz vd.x] [vd.yz max min] [desc 0..15] [desc 16..31] --
// so the four loads (stores) of a point are one 64-byte run and a wave moves 16 whole rows per instruction.  A latency matter (200 to
// 350 KB for a KITTI local map), not a bandwidth one: no loop, no LDS, no workgroup waits on another.  Every address comes from an id
// checked against the capacity and a page pointer checked against nullptr; ids may repeat in a gather (it only reads), never in a
// scatter (the host refuses them), so no two threads write one byte -- except the gather's `absent` word, which every thread that finds
// an id without a row sets to the same value with an ordinary store.
#include <hip/hip_runtime.h>

#include "orbfe_mpstore.h"

namespace {

const int MP_NT = 256;

// (mp_row, the row of an id and its presence byte: orbfe_mpstore.h, shared with k_motion.hip)

__global__ __launch_bounds__(MP_NT) void k_mpstore_gather(MpTable t, int n, const uint64_t* __restrict__ ids, MpArrays out,
                                                          uint8_t* __restrict__ flags, uint32_t* __restrict__ absent) {
  const int g = blockIdx.x * MP_NT + threadIdx.x, i = g >> 2, q = g & 3;
  if (i >= n) return;
  uint8_t* pres = nullptr;
  const uint8_t* row = mp_row(t, ids[i], &pres);
  const bool have = row && *pres;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (have) v = ((const uint4*)row)[q];
  if (q == 0) {
    out.pos[3 * i + 0] = __uint_as_float(v.x), out.pos[3 * i + 1] = __uint_as_float(v.y), out.pos[3 * i + 2] = __uint_as_float(v.z);
    out.view_dir[3 * i + 0] = __uint_as_float(v.w);
    if (!have) {
      if (flags) flags[i] = 0;  // not searched, no edge: nothing behind this launch reads the zero row as a map point
      *absent = 1u;
    }
  } else if (q == 1) {
    out.view_dir[3 * i + 1] = __uint_as_float(v.x), out.view_dir[3 * i + 2] = __uint_as_float(v.y);
    out.max_dist[i] = __uint_as_float(v.z), out.min_dist[i] = __uint_as_float(v.w);
  } else {
    ((uint4*)out.desc)[2 * (size_t)i + (q - 2)] = v;
  }
}

__global__ __launch_bounds__(MP_NT) void k_mpstore_scatter(MpTable t, int n, const uint64_t* __restrict__ ids, uint32_t fields, MpArrays in,
                                                           uint8_t present) {
  const int g = blockIdx.x * MP_NT + threadIdx.x, i = g >> 2, q = g & 3;
  if (i >= n) return;
  uint8_t* pres = nullptr;
  uint8_t* row = mp_row(t, ids[i], &pres);
  if (!row) return;  // (never: the host has allocated the page of every id it lists)
  float* f = (float*)row;
  if (q == 0) {
    if (fields & MP_FIELD_POS) f[0] = in.pos[3 * i + 0], f[1] = in.pos[3 * i + 1], f[2] = in.pos[3 * i + 2];
    if (fields & MP_FIELD_NORMAL_DEPTH) f[3] = in.view_dir[3 * i + 0];
    *pres = present;
  } else if (q == 1) {
    if (fields & MP_FIELD_NORMAL_DEPTH)
      ((float4*)row)[1] = make_float4(in.view_dir[3 * i + 1], in.view_dir[3 * i + 2], in.max_dist[i], in.min_dist[i]);
  } else if (fields & MP_FIELD_DESC) {
    ((uint4*)row)[q] = ((const uint4*)in.desc)[2 * (size_t)i + (q - 2)];
  }
}

}  // namespace

void launch_mpstore_gather(hipStream_t st, MpTable t, int n, const uint64_t* ids, MpArrays out, uint8_t* flags, uint32_t* absent) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_mpstore_gather, dim3((4 * (unsigned)n + MP_NT - 1) / MP_NT), dim3(MP_NT), 0, st, t, n, ids, out, flags, absent);
}

void launch_mpstore_scatter(hipStream_t st, MpTable t, int n, const uint64_t* ids, uint32_t fields, MpArrays in, uint8_t present) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_mpstore_scatter, dim3((4 * (unsigned)n + MP_NT - 1) / MP_NT), dim3(MP_NT), 0, st, t, n, ids, fields, in, present);
}
