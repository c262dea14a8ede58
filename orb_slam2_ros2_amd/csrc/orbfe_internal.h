// orbfe_internal.h -- structures shared by the host side of the C-ABI and the gfx950 kernels.
#pragma once
#include <stdint.h>

#include "../../include/orbfe.h"
#include "ba_edge_dev.h"

#define ORBFE_MAX_STRIPS 16  // Quadtree::initSplit root strips, round(w/h)  (ORBExtractor.cc:85)
#define ORBFE_BORDER 19      // ORBExtractor::mnBorderSize (ORBExtractor.cc:523)
#define ORBFE_EDGE 16        // mnBorderSize - 3: origin of the FAST region (ORBExtractor.cc:336-337)
#define ORBFE_CENTROID_R 15  // ORBExtractor::mnCentroidR (ORBExtractor.cc:518)
#define ORBFE_MAX_CELL 72    // largest FAST patch side (cell < 60, +6 overlap), LDS tile bound

// fixed-point bilinear tap: dst(dx) = S[ofs]*c0 + S[ofs+1]*c1   (cv::resize INTER_LINEAR, 11-bit)
struct ResizeTap {
  int32_t ofs;
  int16_t c0, c1;
};

// k_blur: output rows per wave (a block = 4 waves stacked vertically); the host sizes the tile grid with it.  A wave reads six rows more than
// it writes: 64 rows per wave (70 / 64 = 9 % of halo work, 19 % at 32) -- step 5.198 -> 5.163 ms, same box, alternating, three rounds; 48: no gain
#ifndef BLUR_ROWS
#define BLUR_ROWS 64
#endif

// k_resize work item: RS_TW x RS_TH output pixels of one level and the level-0 footprint they read
#define RS_TW 64
#define RS_LDS_BYTES 16384  // largest footprint a tile may stage
struct RsTile {
  int16_t level, x0, y0;  // output tile origin
  int16_t sx_lo, nw;      // footprint: first level-0 column (multiple of 16), 32-bit words per row (multiple of 4); nw == 0: does not fit the LDS
  int16_t sy_lo, nr;      // first level-0 row, rows
  int16_t pad;
};

// k_resize_regions work item: a block of level 0 staged ONCE and the output words of EVERY level whose first source pixel lies in it.
// rg_w x rg_h level-0 pixels per region (plus the halo the bilinear taps of its last words reach into), chosen per geometry: the block
// width (a multiple of 16 from 128 to 256) and height (47 or 63) that tile the image with the least waste -- a last column of a few
// pixels is a workgroup in eight that stages a tile and walks seven levels for almost nothing (1241 px: 176 -> 0.79 ms, 208 or 256 -> 0.66).
struct RsRegionLevel {
  int16_t wx0, nwx;        // output words (4 px) of the level: first, count
  int16_t oy0, noy;        // output rows: first, count
  uint16_t xt_lds, yt_lds; // first x tap (8-byte units) / y tap (16-byte units) of the level in the workgroup's LDS tables
  uint32_t inv_nwx;        // ceil(2^20 / nwx): word index -> row without a division
};
// taps as the inner loop wants them, laid out per region exactly as they sit in LDS (the workgroup copies them, 16 bytes at a time)
struct RgXTap {
  int32_t sxo;     // byte offset of the tap's first source pixel inside a staged row
  uint32_t taps2;  // (c0 << 4) | (c1 << 20): the two coefficients, pre-shifted, as the halves v_dot2_u32_u16 multiplies
};
struct RgYTap {
  int32_t o0, o1;   // byte offsets of the two source rows inside the staged tile
  uint32_t b0, b1;  // the two coefficients << 8
};
struct RsRegion {
  int16_t sx0, sy0;        // first staged level-0 column (multiple of 16) / row
  int16_t nq, nr;          // staged 16-byte quads per row, rows
  uint32_t inv_nq;         // ceil(2^20 / nq)
  uint16_t n_xt, n_yt;     // taps of all levels (n_xt is a multiple of 4)
  int16_t cy0, ch, cq;     // the block of level 0 the region OWNS: rows [cy0, cy0 + ch), cq 16-byte units from column sx0 (always staged: the
  int16_t pq;              // region kernel can write level 0 of the pyramid from its tile, which replaces the copy-in of device batches)
                           // pq: LDS row pitch of the tile in 16-byte units, ODD (a pitch of 128 / 192 / 256 bytes puts the rows a wave reads on the
                           // same banks: region widths 112 / 176 / 240 ran 15 % slower than 96 / 128 / 144 / 160 until the pitch was padded)
  uint32_t xt_off, yt_off; // first entry of the region in the context's RgXTap / RgYTap arrays
  RsRegionLevel lev[ORBFE_MAX_LEVELS - 1];
};

// k_quadtree: the levels whose trees one wave works through, as bit masks (one per blockIdx.x)
struct QtGroups {
  uint32_t mask[ORBFE_MAX_LEVELS];
  // n_order > 0: the waves of an image do not take fixed masks but PULL levels, in this order (most expensive first), from a per-image
  // counter: list scheduling with the trees' actual durations (a level's candidate count depends on the image)
  uint8_t order[ORBFE_MAX_LEVELS];
  int32_t n_order;
};

// Per pyramid level, resident in device memory (one table per context).
// A frame or two: k_fast appends a level's candidates to ORBFE_FAST_SHARDS lists (cell index mod shards) instead of one -- see k_fast.hip
#define ORBFE_FAST_SHARDS 16
struct LevelDev {
  int32_t w, h, stride;  // plane size, row pitch in bytes (multiple of 16)
  uint32_t plane_off;    // byte offset of the plane inside one image's pyramid buffer
  float sf;              // mvfScaledFactors[level]
  int32_t quota;         // mvnFeatures[level]
  int32_t quota_off;     // sum of quotas of the lower levels
  // FAST cell grid (ORBExtractor.cc:334-343)
  int32_t reg_w, reg_h;  // region [16, w-16) x [16, h-16)
  int32_t n_cols, n_rows, w_cell, h_cell;
  uint32_t inv_w_cell, inv_h_cell;  // ceil(2^20 / cell size): exact floor-division of a 12-bit coordinate by the cell size
  int32_t cell_base;     // first flattened cell id of this level
  int32_t n_cells;
  int32_t cell_cap;      // upper bound on 3x3-strict local maxima in one cell interior
  // candidate list / quadtree
  uint32_t cand_base;    // first record (uint32 units) of this level inside one image's candidate buffer
  uint32_t cand_cap;     // = n_cells * cell_cap
  uint32_t shard_cap;    // contexts of a frame or two (ORBFE_FAST_SHARDS): records of ONE shard of the level's region, ceil(n_cells / shards) * cell_cap; else 0
  int32_t n_ini;         // root strips
  // a level whose quota does not fit the node table one CU's LDS can hold keeps its table (and sort buffer) in global memory:
  // qt_big_cap > 0 nodes at byte offset qt_big_off of the image's block of the context's d_qt_big buffer, qt_big_sort keys to sort
  uint32_t qt_big_off;
  int32_t qt_big_cap, qt_big_sort;
  uint32_t qt_tab_off;   // this level's coordinate -> code tables in the context's d_qt_tabs (uint16 units, even)
  double strips[ORBFE_MAX_STRIPS + 1];
  // resize tap tables (levels >= 1): offsets into the context's tap array
  uint32_t xtab_off, ytab_off;
  // launch geometry
  int32_t rs_tiles_x, rs_tiles_y, rs_tile_base;  // resize: 64x4 output tiles
  int32_t bl_tiles_x, bl_tiles_y, bl_tile_base;  // blur:   64x16 output tiles
};

// k_blur_mfma.hip: launch geometry and band tables of the batches' blur on the integer matrix cores
struct MbLevel {
  int32_t wg_base, strips;  // first workgroup of the level (four 48-column strips each), strips per row
  int32_t tx_off, ty_off;   // first band (512-byte units) of the level's column blocks / row blocks
};
struct MbGeom {
  MbLevel lv[ORBFE_MAX_LEVELS];
  int32_t n_wg;
  uint32_t spare_off;  // byte offset, inside an image's block of the pyramid buffers, of 256 bytes no plane uses (lanes with nothing to store write there)
};

// One FAST cell (flattened over levels).  Patch = what the reference hands to cv::FAST (ORBExtractor.cc:363).
struct CellDev {
  int16_t level;
  int16_t x0, y0;      // patch origin in level coordinates (iniX, iniY)
  int16_t pw, ph;      // patch size (maxX-iniX, maxY-iniY)
  int16_t offx, offy;  // jdx*wCell, idx*hCell  (ORBExtractor.cc:370-371)
  int16_t pad;
};

// candidate / selected-keypoint record: x (12 bit) | y (12 bit) | response (8 bit); x,y in region coordinates
#define ORBFE_PACK_XYR(x, y, r) ((((uint32_t)(x)) << 20) | (((uint32_t)(y)) << 8) | ((uint32_t)(r)))
#define ORBFE_REC_X(p) (((p) >> 20) & 0xFFFu)
#define ORBFE_REC_Y(p) (((p) >> 8) & 0xFFFu)
#define ORBFE_REC_R(p) ((p)&0xFFu)

// auxiliary per-keypoint data the stereo matcher reads (createRowIndexDB row band, ORBMatcher.cc:924-927)
struct KpAux {
  int16_t row_min, row_max;  // [row_min, row_max)
};

// what the stereo matcher reads of a RIGHT keypoint per candidate (8 bytes next to each other): x in level-0 coordinates (the disparity range
// test, ORBMatcher.cc:44-48) and what pixelSADMatch needs of the winner -- octave and the patch centre getPitch computes,
// cvFloor(pt / scale[octave]) (ORBMatcher.cc:1004-1006) -- so that the best candidate's keypoint record is not a memory round trip of its own
struct KpX {
  float x;
  uint32_t q;  // octave (4 bits: ORBFE_MAX_LEVELS = 16) | cvFloor(pt.x / sf) << 4 (14 bits) | cvFloor(pt.y / sf) << 18 (14 bits; orbfe_create bounds the image at 4096 x 4096)
};
#define ORBFE_KPX_Q(oct, qx, qy) ((uint32_t)(oct) | ((uint32_t)(qx) << 4) | ((uint32_t)(qy) << 18))
#define ORBFE_KPX_OCT(q) ((int)((q)&15u))
#define ORBFE_KPX_QX(q) ((int)(((q) >> 4) & 0x3FFFu))
#define ORBFE_KPX_QY(q) ((int)((q) >> 18))

// device buffers of the batches' row-parallel stereo matcher (k_match.hip), per pair
struct StereoRowsBuf {
  uint32_t* lrow_off;
  uint16_t* lrow_list;
  uint4* work;
  int32_t* work_n;
};

// local BA: non-fixed keyframes the dense reduced solver takes (its panel, right-hand side and diagonal blocks live in 64 KB of LDS)
#define LBA_MAX_FREE 100

// (BaParamsDev, the camera of the edge model: ba_edge_dev.h)

// ---- device-side Levenberg-Marquardt control of the local BA (k_lm.hip) -------------------------------------------------------------
#define LM_CHOL_MAX_NB 42  // free keyframes the register-resident Cholesky takes: 42 * 41 / 2 = 861 off-diagonal blocks, two per thread of 448
// free keyframes the device-side path takes; past it the host-driven loop runs.  The value is kept from r4, when a one-workgroup back
// substitution held y in 48 KB of LDS; k_lmb_back_mw has no such limit and nothing structural enforces 1000 now -- what bounds the
// device path is memory (the dense (ld + 48) x ld system, the nf x NP pair table) and 32-bit products such as b * pair_cap in k_lm_schur.
#define LM_BIG_MAX_NB 1000

// The state record one control lane advances between the trials (device memory; the host reads it once per call).
struct LmState {
  double lambda, ni, current_chi, maxdiag;  // (lambda, ni, current_chi and qmax: the damping state of lm_ctrl.h)
  double chi_of[2];     // robust chi2 of the estimate in buffer 0 / 1
  int32_t iters[2];     // iteration budgets of the two optimize() calls (Optimizer.cc:336, :361)
  int32_t done[2];      // iterations started (what optimize() returns)
  int32_t round;        // 0 / 1: which optimize() call; 2: both over
  int32_t it;           // iteration index inside the round
  int32_t qmax;         // trials of the current iteration
  int32_t phase;        // 0: start an iteration | 1: a trial ran, decide it | 3: run another trial of this iteration | 2: round over
  int32_t cur;          // which of the two estimate / system buffers is current
  int32_t run_step, run_switch, run_final;  // gates the kernels of a step / the switch group / the final group read
  int32_t switched, finalized, stopped;
  int32_t ok;           // cleared by the solver kernels of a trial when a point block or a pivot is singular
  int32_t need_chi;     // the current system was (re)built outside a trial: take its chi2 from the partial sums
  int32_t pad;
};

// The estimates, the edge terms and the normal-equation blocks exist twice: [cur] = the current estimate and its system,
// [cur ^ 1] = the trial's.  The kernels of k_lm.hip take this record by value.
struct LmBuffers {
  double* poses[2];
  double* points[2];
  double* terms[2];     // [E][32]: the per-edge terms of one linearisation (k_lm.hip, LM_TERM)
  double* Hpl[2];       // [E][18]
  double* Hpp[2];       // [NK][36]
  double* bp[2];        // [NK][6]
  double* Hll[2];       // [NP][9]
  double* bl[2];        // [NP][3]
  double* chi_part[2];  // per linearize block: sum of rho(chi2) over its active edges
};

struct LmLaunch {
  int NK, NP, E, nf;
  LmBuffers B;
  LmState* state;
  LmState* state_out;  // copy of the state after the last control step of a pass, inside the result block (one download)
  const int32_t *edge_pose, *edge_point, *pt_off, *pt_edges, *ps_off, *ps_edges, *free_pose, *pose_slot;
  int2* pairs;          // [nf (nf + 1) / 2][pair_cap], built on the device (launch_lm_pairs)
  int32_t* pair_cnt;    // [nf (nf + 1) / 2]
  int32_t* pair_table;  // [nf][NP]: edge of free pose j observing the point, -1 if none
  int pair_cap;         // longest edge list of a free pose
  const double *meas, *info;
  const uint8_t *is_stereo, *fixed;
  double *info_eff, *delta_eff, *chi2_last;
  uint8_t* level;
  double *Dinv, *W, *Sblk, *rhs, *x, *scale_part;
  double* M;            // nf > LM_CHOL_MAX_NB: the dense reduced system of the blocked solver (k_lmbig.hip), (ld + 48) x ld, else nullptr
  int ld;
  int32_t* lmb_flags;   // [2 ld / 48 + 2]: [KT] bad pivot, [KT + 1 ...] the back substitution's column flags
  double* lmb_inv;      // [ld / 48][3][256]: inverses of the 16 x 16 diagonal blocks of the factorised diagonal tiles
  double *chi2_out, *poses_out, *points_out;
  uint8_t *bad, *level_out;
  const volatile uint8_t* abort_flag;  // device address of a host-mapped byte the caller's stop flag is mirrored into
  BaParamsDev prm;
};

// ---- block-CSR reduced system and its conjugate-gradient solver (k_bsr.hip, orbfe_gba.hip) ------------------------------------------
enum { PCG_RUNNING = 0, PCG_CONVERGED = 1, PCG_BREAKDOWN = 2 };
// The solver's scalars (device memory; the host reads iters and state between chunks of iterations).  Iteration k reads entry k & 1 of
// rz and state and writes the other one.
struct PcgState {
  double rz[2];       // r . M^-1 r
  double rz0, tol2;   // b . M^-1 b | tol^2: converged when rz <= tol2 * rz0
  int32_t state[2];   // PCG_*
  int32_t iters;      // iterations completed
  int32_t pq_bad;     // this iteration's p . S p was not positive and finite
  int32_t done;       // the verdict for the host (PCG_*): written with the state, read by no kernel
  int32_t pad;
};
struct BsrPcgLaunch {
  int nb;
  const int32_t *row_off, *col;
  const double *blocks, *rhs;
  double *Minv, *x, *r, *z, *p, *q;  // [nb][36] | five vectors of 6 nb
  double *part_pq, *part_rz;         // [nb] each: one partial per block row
  PcgState* state;
  int* ok;                           // cleared by a diagonal block that is not positive definite
};

// ---- bag of words (k_bow.hip, orbfe_bow.hip) --------------------------------------------------------------------------------------
// Device layout of a vocabulary: every node but the root has a POSITION; the children of a node occupy consecutive positions in file order,
// so one node's children are one contiguous block of 32-byte descriptors (desc[2 p], desc[2 p + 1]) and of records.
struct BowChild {
  int32_t first;  // position of the node's first child (-1: leaf)
  int32_t nc;     // its number of children (0: leaf)
  uint32_t word;  // word id (leaves; 0xFFFFFFFF for inner nodes)
  uint32_t node;  // node id (line order of the text file, root = 0)
};
struct BowVocabDev {
  const BowChild* rec;
  const uint4* desc;
  const double* weight;  // per position: the node's weight
  int32_t root_first, root_nc, L;
};

// ---- keyframe database (k_kfdb.hip, orbfe_kfdb.hip) ------------------------------------------------------------------------------
// One slot per keyframe; its sorted words and their values sit at [off, off + len) of the database's word / value pools.
struct KfSlot {
  uint64_t off;
  uint32_t len;
  uint32_t flags;  // KFDB_LIVE | KFDB_BAD; a free slot has neither
};
#define KFDB_LIVE 1u
#define KFDB_BAD 2u
// The query's device header: the grid-wide maximum of the shared-word counts (k_kfdb_count's atomicMax, read by the NEXT launch) and the
// number of survivors k_kfdb_score has claimed.  Zeroed by the query's upload.
struct KfdbHdr {
  uint32_t max_count;
  uint32_t n_out;
};
// one survivor: its slot (the host maps slots to ids), shared-word count and score
struct KfdbRec {
  uint32_t slot;
  int32_t count;
  double score;
};

// ---- RANSAC sets (k_pnp.hip, k_sim3.hip, ransac_host.h) ---------------------------------------------------------------------------
// One problem (a PnPSolver or a Sim3Solver) of a set: its points or correspondences at [off, off + n) of the set's per-point arrays, an
// inlier mask of `words` uint64 words, mnMinInlier.
struct RansacProb {
  int32_t off, n, words, min_inlier;
};

// ---- EPnP RANSAC (k_pnp.hip, orbfe_pnp.hip) ---------------------------------------------------------------------------------------
// One hypothesis of a speculated schedule: four problem-local sample indices or, with given = 1, a pose to count (the entry pose of the
// first call).  Its inlier mask sits at mask_off (in words) of the hypothesis masks, its refine mask at the same place of the refine masks.
struct PnpHyp {
  int32_t prob, given, mask_off, pad;
  int32_t idx[4];
  float pose[12];  // R row-major, then t
};
// One speculated iterate call: hypotheses [h0, h0 + nh), the entry pose's record (-1: none), the entry list at [entry_off, + entry_len)
// of the uploaded indices, the list scratch [list_off, + list_cap) of the call.
struct PnpCall {
  int32_t prob, h0, nh, entry_hyp;
  int32_t entry_off, entry_len;
  int64_t list_off, list_cap;
};
// What the device found for one hypothesis: Phase A's pose / count / degenerate flag, Phase B's refine (refined = 1 when it ran).
struct PnpOut {
  float pose[12];
  int32_t count, degen, refined, ref_degen;
  int32_t ref_count, err, pad0, pad1;
  float ref_pose[12];
};

// ---- Sim3 RANSAC (k_sim3.hip, orbfe_sim3.hip) -------------------------------------------------------------------------------------
// One hypothesis of a speculated schedule: three problem-local sample indices.  Its inlier mask sits at mask_off (in words) of the
// hypothesis masks, its refine mask at the same place of the refine masks.
struct Sim3Hyp {
  int32_t prob, mask_off;
  int32_t idx[3];
  int32_t pad[3];
};
// What the device found for one hypothesis: the model (Rqp row-major, then tqp) and its count; where the count exceeds mnMinInlier
// (refined = 1), refine's model and count.
struct Sim3Out {
  float model[12];
  float ref_model[12];
  int32_t count, refined, ref_count, pad;
};

// ---- new map points (k_tri.hip, orbfe_tri.hip) -----------------------------------------------------------------------------------
// One keyframe of the call inside the upload: byte offsets of its arrays, its sizes and poses.  kf[0] is the current keyframe,
// kf[1 + i] neighbour i; a neighbour's FeatureVector entry j is match slot slot0 + j.
struct TriKf {
  uint32_t o_kps, o_desc, o_nodes, o_offs, o_feat, o_flags, o_depth, o_ru;
  int32_t n, n_nodes, n_feat, slot0, skip, pad;
  float Tcw[16], Twc[16];
};
struct TriParams {
  float fx, fy, cx, cy;
  float kinv[9];
  int32_t n_nb, n_levels, n_cur, n_slots;
  uint32_t o_unproc, o_upos, o_sf;
  int32_t rec_cap, tail_cap;
};
// a match slot after k_tri_match: the current feature (-1: no match), the branch's kind (0: no point), checkMapPoint's verdict, the point
struct TriSlot {
  int32_t q, t, nb, kind, ok;
  float xyz[3];
};
struct TriRec {
  int32_t nb, q, t, kind;
  float xyz[3];
};

// ---- inverse fuses of a new keyframe (k_fuse.hip, orbfe_fuse.hip) -------------------------------------------------------------------
// One target keyframe of the call: byte offsets of its arrays in the scratch block (64 bit: 64 x 65535 features stay addressable), its
// grid geometry (search_area_layout.h: AreaGrid from its bounds), its octave-window case and its pose.
struct FuseKf {
  uint64_t o_kps, o_desc, o_coff, o_cfeat;
  int32_t n, rows, cols, clip_w, clip_h;
  int32_t mode;  // 0: [octave - 1, octave + 1], 1 (up): [octave, 7], 2 (down): [0, octave]
  int32_t in_lds, pad;  // the grid build keeps this keyframe's lists in LDS
  float R[9], t[3];
  float bounds[4];
};
struct FuseParams {
  float fx, fy, cx, cy;
  float th, ratio;
  int32_t dist_threshold, n_kf, n_cur;
};

// ---- keyframes resident on the device (k_kfstore.hip, orbfe_kfstore.hip) -----------------------------------------------------------
// One insertion: the source arrays (an extraction slot's, or the entry's own after a host upload), the entry's arrays, the grid's size.
struct KfPack {
  const orbfe_keypoint* s_kps;
  const uint8_t* s_desc;
  const double *s_depth, *s_right_u;  // nullptr: -1 everywhere
  orbfe_keypoint* kps;
  uint8_t* desc;
  double *depth, *right_u;
  int32_t *cell_off, *cell_feat;
  int32_t n, rows, cols, in_lds;
  int32_t n_copy;  // workgroups that copy (0: the features are in place, only the grid is built)
};
// TriKf of a STORED keyframe: the keyframe's own arrays where the store keeps them, its flags at o_flags of the call's upload.
struct TriKfStored {
  const orbfe_keypoint* kps;
  const uint8_t* desc;
  const uint32_t* nodes;
  const int32_t* offs;
  const uint32_t* feat;
  const double *depth, *ru;
  uint32_t o_flags;
  int32_t n, n_nodes, n_feat, slot0, skip, pad;
  float Tcw[16], Twc[16];
};

// ---- searchByBow over stored keyframes (k_bowsearch.hip, orbfe_bowsearch.hip) -------------------------------------------------------
// One candidate keyframe of the call: its arrays where the keyframe store keeps them, its flags at o_flags of the call's upload; its
// FeatureVector entry j is match slot slot0 + j.
struct BowKf {
  const orbfe_keypoint* kps;
  const uint8_t* desc;
  const uint32_t* nodes;
  const int32_t* offs;
  const uint32_t* feat;
  uint32_t o_flags;
  int32_t n_nodes, n_feat, slot0;
};
// The query in its two forms: host arrays behind the call's upload, or a stored keyframe.  The flags are in the upload in both.
struct BowQuery {
  uint32_t o_desc, o_angle, o_nodes, o_offs, o_feat, o_flags;
  int32_t n_nodes;
};
struct BowQueryStored {
  const orbfe_keypoint* kps;
  const uint8_t* desc;
  const uint32_t* nodes;
  const int32_t* offs;
  const uint32_t* feat;
  uint32_t o_flags;
  int32_t n_nodes;
};
// The third form (orbfe_track_reference_stored): a frame in its extraction slot.  Descriptors and angles are the slot's
// arrays; the FeatureVector is device memory too -- what k_bow_group has just written, or a host FeatureVector behind the call's upload
// -- and its node count is read from device memory, because the host never sees the one k_bow_group wrote.
struct BowQuerySlot {
  const orbfe_keypoint* kps;
  const uint8_t* desc;
  const uint32_t* nodes;
  const int32_t* offs;
  const uint32_t* feat;
  const int32_t* n_nodes;
  uint32_t o_flags;
};
struct BowParams {
  int32_t mode, dist_threshold, check_orientation, n_kf;
  float ratio;
  int32_t cap;  // matches the download has room for
};
// a match slot after k_bow_match: q = the query feature (-1: no match), the keyframe feature, the distance, verifyAngle's bin (0 without it)
struct BowSlot {
  int32_t q, t, d, bin;
};
struct BowMatch {
  int32_t q, t, d;
};

// ---- searchBySim3 over stored keyframes (k_sim3search.hip, orbfe_sim3search.hip) -----------------------------------------------------
// One keyframe of the pair as the device reads it: its arrays where the keyframe store keeps them, its map state at offsets of the
// call's upload, its pose, and the similarity that takes a point of ITS camera frame into the other keyframe's (direction A, source C:
// Scm.inv(); direction B, source M: Scm).  state[i] = the flag byte of feature i | SIM3S_NAMED if an input match names the feature.
#define SIM3S_NAMED 4
struct Sim3Kf {
  const orbfe_keypoint* kps;
  const uint8_t* desc;
  const int32_t *cell_off, *cell_feat;
  int32_t n, rows, cols, clip_w, clip_h;
  uint32_t o_state, o_pos, o_max, o_min;
  float bounds[4];
  float Rcw[9], tcw[3];
  float s, R[9], t[3];
};
struct Sim3SearchParams {
  float fx, fy, cx, cy;
  float th, ratio, log_sf;
  int32_t dist_threshold, max_level;
  uint32_t o_sf;
};
// the points overload: the loop group's map points at offsets of the upload, the similarity Scw
struct Sim3Points {
  uint32_t o_usable, o_pos, o_vdir, o_max, o_min, o_desc;
  int32_t m;
  float s, R[9], t[3];
};

// ---- the forward fuse over stored keyframes (k_fusepoints.hip, orbfe_fusepoints.hip) ------------------------------------
// One target keyframe as the device reads it: its arrays where the keyframe store keeps them, its stored bounds, the pose of the call.
struct FusePtsKf {
  const orbfe_keypoint* kps;
  const uint8_t* desc;
  const int32_t *cell_off, *cell_feat;
  int32_t n, rows, cols, clip_w, clip_h, pad;
  float bounds[4];
  float R[9], t[3];
};
// A pair (k, j) that passed isInVision, with what the projection found: the search does not project again.
struct FusePtsEntry {
  int32_t k, j, o;  // keyframe, point, predicted level
  float u, v, cos_theta;
};
// the map points and the scale factors in the call's upload; m points, n_kf keyframes
struct FusePtsParams {
  float fx, fy, cx, cy;
  float th, ratio, log_sf;
  int32_t dist_threshold, max_level, n_levels, n_kf, m;
  const uint8_t *usable, *desc;
  const float *pos, *vdir, *max_dist, *min_dist, *sf;
};
#define FUSEPTS_SEARCH_BLOCKS 2048  // k_fusepts_search's fixed grid: 8192 waves, 32 per compute unit of 256

// ---- the pose-only step of the six tracking calls (pose_check_dev.h on the device, pose_call.h on the host) ------------------------------
// The register kernels of k_pose.hip take this many edges (POSE_RT * POSE_EPT there); a frame holds one edge per feature at most, so the
// six calls refuse a context of more features, and k_trackref_seed keeps a claim per feature in LDS.
#define POSE_REG_EDGES 2048
// The frame of the step: its features where the slot keeps them, and for the fused calls the pose it has on entry and its camera.
struct PoseFrameDev {
  const orbfe_keypoint* kps;
  const int32_t* n_kp;  // the slot's count, at most nf
  int32_t nf, n_levels;
  const double* right_u;             // [nf], negative: a mono edge
  const float *sigma2, *inv_sigma2;  // [n_levels]
  float R0[9], t0[3];                // the pose the frame has until setPose (Optimizer.cc:201)
  float fx, fy, cx, cy, max_u, max_v;
};
// The edge list of Optimizer::OptimizePoseOnly in feature order (Optimizer.cc:58-117), as pose_edges_1024 writes it.
struct PoseEdgesDev {
  int32_t* edge_of;  // [nf] the edge of a feature, -1: none
  double *Xw, *meas, *info;
  float* sig;
  const uint8_t* e_inl;  // the optimiser's inlier flag per edge
};

// ---- the relocalisation refine over a stored keyframe (k_reloc.hip, orbfe_reloc.hip) -------------------------------------
// Everything the kernels of one call read and write: the frame where its slot keeps it, the keyframe where the store keeps it, the map
// state of the call's upload, the state that stays on the device and the block that goes down.  hdr: [0] verdict (0: still running),
// [1..2] n_edges, [3..4] n_inliers, [5..6] n_added, [7..8] tlc_z as float bits.
#define RELOC_H_VERDICT 0
#define RELOC_H_EDGES 1
#define RELOC_H_INLIERS 3
#define RELOC_H_ADDED 5
#define RELOC_H_TLCZ 7
struct RelocDev {
  PoseFrameDev F;  // R0, t0: the PnP pose
  PoseEdgesDev E;
  // the frame's packed records, descriptors and grid
  const uint4* f_kpl;
  const uint8_t* f_desc;
  const int32_t *cell_off, *cell_feat;
  int32_t rows, cols, clip_w, clip_h;
  // the stored keyframe and its map state
  const orbfe_keypoint* k_kps;
  const uint8_t* k_desc;
  const uint8_t* good;
  const float* pos;
  int32_t n;
  float kf_R[9], kf_t[3];
  // the call
  const int32_t* held;
  float baseline, th[2], ratio;
  int32_t min_threshold, min_inliers, enough;
  // device state: what the frame holds, the claims of a search, the optimisations' counts and estimates
  int32_t *cur, *claim /*[2][nf]*/, *cnt /*[2] edge counts, -1: no optimisation*/;
  double *p_init /*[2][7]*/, *p_opt /*[2][7]*/;
  // the downloaded block
  int32_t* hdr;
  double* pose_out /*[2][7]*/;
  float* tcw_out /*[2][12]*/;
  uint8_t* inlier /*[2][nf]*/;
  int32_t *assigned /*[2][nf]*/, *hits /*[2][nf]*/;
  uint8_t* qa /*[2][n]*/;
};

// ---- trackReference over a stored keyframe (k_trackref.hip, orbfe_trackref.hip) ------------------------------------------
// Everything the glue kernels of one call read and write.  hdr: [0] verdict (0: still running), [1] n_matches, [2] n_edges, [3] n_inliers.
#define TRACKREF_H_VERDICT 0
#define TRACKREF_H_MATCHES 1
#define TRACKREF_H_EDGES 2
#define TRACKREF_H_INLIERS 3
struct TrackRefDev {
  PoseFrameDev F;
  PoseEdgesDev E;
  // the map state of the call's upload: the keyframe's, then what the frame came with
  const float* pos;       // [n][3]
  const uint8_t* f_good;  // [nf]
  const float* f_pos;     // [nf][3]
  int32_t n, min_matches, min_inliers;
  // searchByBow's list (k_bow_select, one candidate) and its length
  const BowMatch* list;
  const int32_t* n_list;
  // device state: the optimisation's count and estimates
  int32_t* cnt /*[1] edge count, -1: no optimisation*/;
  double *p_init /*[7]*/, *p_opt /*[7]*/;
  // the downloaded block
  int32_t* hdr;
  BowMatch* matches /*[n]*/;
  int32_t *assigned /*[nf]*/, *cur /*[nf]: final_assigned*/;
  double* pose_out /*[7]*/;
  float* tcw_out /*[12]*/;
  uint8_t* inlier /*[nf]*/;
};

// ---- trackMotionModel over two frame slots (k_motion.hip, orbfe_motion.hip) ----------------------------------------------
// Everything the glue kernels of one call read and write.  Queries are indexed by LAST-FRAME FEATURE: a feature that is no query has
// radius -1 in both passes (k_search_area leaves such a query at once), so the searches keep a host-side count (the feature capacity),
// nothing is compacted and the query descriptors are the last slot's own array.  hdr: [0] verdict, [1] passes, [2] n_matches,
// [3] n_edges, [4] n_inliers, [5] n_in_map.
#define MOTION_H_VERDICT 0
#define MOTION_H_PASSES 1
#define MOTION_H_MATCHES 2
#define MOTION_H_EDGES 3
#define MOTION_H_INLIERS 4
#define MOTION_H_INMAP 5
struct MotionDev {
  PoseFrameDev F;  // the current frame; R0, t0: the predicted pose
  PoseEdgesDev E;  // (written by k_track_edges: the glue kernels only read it)
  // the last frame (slot arrays); l_depth nullptr: no depth
  const orbfe_keypoint* l_kps;
  const int32_t* l_n_kp;
  const double* l_depth;
  // the map state of the call's upload; table nullptr: positions from l_pos, else from the store's rows of l_ids (MpTable's fields)
  const uint8_t* l_flags;
  const uint64_t* l_ids;
  const float* l_pos;
  const uint8_t* const* table;
  uint32_t rows_per_page, max_pages;
  float lR[9], lt[3], lRwc[9], ltwc[3];
  float baseline, th, th_second;
  int32_t min_matches, min_inliers;
  // device state: the query arrays of both passes, the claims and the accepted-query counter, what the second pass excludes, the
  // optimisation's counts and estimates
  float *qxy, *rad1, *rad2, *q_pos;
  int8_t *lo, *hi;
  uint8_t *q_flags, *ex2;
  const int32_t *claim1, *n_accept;
  const uint8_t *qa1, *qa2;
  const int32_t* cnt /*[0] n_matches, [1] edge count, -1: no optimisation*/;
  double* p_init /*[7]*/;
  const double* p_opt /*[7]*/;
  // the downloaded block
  int32_t* hdr;
  uint32_t* bad;  // set by a flagged id without a row
  const int32_t* assigned /*[nf]*/;
  int32_t *cur /*[nf]: final_assigned*/, *qm /*[nf]: query_matches*/;
  uint8_t *inlier /*[nf]*/, *temp /*[nf]*/;
  float* temp_pos /*[nf][3]*/;
  double* pose_out /*[7]*/;
  float* tcw_out /*[12]*/;
};
