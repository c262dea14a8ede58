// ba_host.h -- what the host entry points of the bundle adjustments share (orbfe_ba.hip, orbfe_gba.hip): the problem's check, the
// vertex -> edges lists, the problem's arrays in the scratch and the system builder's launch record.
#pragma once
#include "orbfe_ctx.h"
namespace {

// every edge of the problem names an existing pose and point
orbfe_status ba_check_problem(orbfe_ctx* c, const char* who, const orbfe_ba_problem* p) {
  for (int e = 0; e < p->n_edges; ++e)
    if (p->edge_pose[e] < 0 || p->edge_pose[e] >= p->n_poses || p->edge_point[e] < 0 || p->edge_point[e] >= p->n_points)
      return fail(c, ORBFE_EBADARG, "%s: edge %d references vertex out of range", who, e);
  return ORBFE_OK;
}

// vertex -> edges lists, edges in ascending index (counting sort): the summation order of the segmented reductions
struct BaVertexLists {
  std::vector<int32_t> pt_off, pt_edges, ps_off, ps_edges;
};
void ba_vertex_lists(const orbfe_ba_problem* p, BaVertexLists* v) {
  const int E = p->n_edges, NK = p->n_poses, NP = p->n_points;
  v->pt_off.assign(NP + 1, 0), v->ps_off.assign(NK + 1, 0), v->pt_edges.resize(E), v->ps_edges.resize(E);
  for (int e = 0; e < E; ++e) {
    ++v->pt_off[p->edge_point[e] + 1];
    ++v->ps_off[p->edge_pose[e] + 1];
  }
  for (int i = 0; i < NP; ++i) v->pt_off[i + 1] += v->pt_off[i];
  for (int i = 0; i < NK; ++i) v->ps_off[i + 1] += v->ps_off[i];
  std::vector<int32_t> pc(v->pt_off.begin(), v->pt_off.end() - 1), kc(v->ps_off.begin(), v->ps_off.end() - 1);
  for (int e = 0; e < E; ++e) {
    v->pt_edges[pc[p->edge_point[e]]++] = e;
    v->ps_edges[kc[p->edge_pose[e]]++] = e;
  }
}

// The problem's arrays in the scratch (every entry point uploads them) and, behind them, the fixed flags and the vertex lists: one table
// of (source, bytes) that is laid out by ba_take and staged by ba_put.
enum { BA_POSE, BA_PT, BA_EP, BA_ET, BA_MEAS, BA_ST, BA_INFO, BA_DELTA, BA_FIX, BA_PTO, BA_PTE, BA_PSO, BA_PSE, BA_FIELDS };
struct BaInputs {
  struct Field {
    const void* src;
    size_t bytes, off;
  } f[BA_FIELDS];
  int n;
  size_t operator[](int k) const { return f[k].off; }
};
// v == nullptr: the problem alone (no fixed flags, no lists)
void ba_take(ScratchLayout& L, const orbfe_ba_problem* p, const uint8_t* pose_fixed, const BaVertexLists* v, BaInputs* in) {
  const size_t E = (size_t)p->n_edges, NK = (size_t)p->n_poses, NP = (size_t)p->n_points;
  const BaInputs::Field f[BA_FIELDS] = {
      {p->poses, NK * 56, 0}, {p->points, NP * 24, 0}, {p->edge_pose, E * 4, 0}, {p->edge_point, E * 4, 0}, {p->meas, E * 24, 0},
      {p->is_stereo, E, 0}, {p->info, E * 8, 0}, {p->huber_delta, E * 8, 0}, {pose_fixed, NK, 0},
      // (k_lm_linpoints / lm_pose_block and k_lba_solve read pt_off[point + 1] and ps_off[pose + 1] of the last vertex)
      {v ? v->pt_off.data() : nullptr, (NP + 1) * 4, 0}, {v ? v->pt_edges.data() : nullptr, E * 4, 0},
      {v ? v->ps_off.data() : nullptr, (NK + 1) * 4, 0}, {v ? v->ps_edges.data() : nullptr, E * 4, 0}};
  in->n = v ? BA_FIELDS : BA_FIX;
  for (int k = 0; k < in->n; ++k) in->f[k] = {f[k].src, f[k].bytes, L.take(f[k].bytes)};
}
void ba_put(StagedIo& io, const BaInputs& in) {
  for (int k = 0; k < in.n; ++k)
    if (in.f[k].src) io.put(in.f[k].off, in.f[k].src, in.f[k].bytes);
    else std::memset(io.host<uint8_t>(in.f[k].off), 0, in.f[k].bytes);  // (no pose_fixed array: every pose is free)
}
// what the system build and the device-side optimiser tell the k_lm kernels in the same way: sizes, inputs, lists, camera
void lm_fill_inputs(LmLaunch& L, const StagedIo& io, const BaInputs& in, const orbfe_ba_problem* p) {
  L.NK = p->n_poses, L.NP = p->n_points, L.E = p->n_edges;
  L.B.poses[0] = io.dev<double>(in[BA_POSE]), L.B.points[0] = io.dev<double>(in[BA_PT]);
  L.edge_pose = io.dev<int32_t>(in[BA_EP]), L.edge_point = io.dev<int32_t>(in[BA_ET]);
  L.pt_off = io.dev<int32_t>(in[BA_PTO]), L.pt_edges = io.dev<int32_t>(in[BA_PTE]);
  L.ps_off = io.dev<int32_t>(in[BA_PSO]), L.ps_edges = io.dev<int32_t>(in[BA_PSE]);
  L.meas = io.dev<double>(in[BA_MEAS]), L.info = io.dev<double>(in[BA_INFO]), L.is_stereo = io.dev<uint8_t>(in[BA_ST]);
  L.fixed = io.dev<uint8_t>(in[BA_FIX]), L.delta_eff = io.dev<double>(in[BA_DELTA]);
  L.prm = {p->fx, p->fy, p->cx, p->cy, p->bf};
}
// One system at one estimate, outside the device-side optimiser (orbfe_ba_build_system, the host-driven loop): both buffer sets are the
// one given, the control state is zeros (buffer 0 current), then launch_lm_build(s, L, 0, 0, 0, true).
struct LmSystemAt {
  size_t state, level, info_eff, hpp, bp, hll, bl, hpl, terms /* [E][32] */, chi /* [(NP + 31) / 32] */;
};
void lm_fill_one_system(LmLaunch& L, const StagedIo& io, const LmSystemAt& o) {
  LmBuffers& B = L.B;
  L.nf = 0;
  B.poses[1] = B.poses[0], B.points[1] = B.points[0];
  B.terms[0] = B.terms[1] = io.dev<double>(o.terms), B.Hpl[0] = B.Hpl[1] = io.dev<double>(o.hpl);
  B.Hpp[0] = B.Hpp[1] = io.dev<double>(o.hpp), B.bp[0] = B.bp[1] = io.dev<double>(o.bp);
  B.Hll[0] = B.Hll[1] = io.dev<double>(o.hll), B.bl[0] = B.bl[1] = io.dev<double>(o.bl);
  B.chi_part[0] = B.chi_part[1] = io.dev<double>(o.chi);
  L.state = io.dev<LmState>(o.state);
  L.info_eff = io.dev<double>(o.info_eff), L.chi2_last = nullptr, L.level = io.dev<uint8_t>(o.level);
}

}  // namespace
