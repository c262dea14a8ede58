/* orbfe.h -- C-ABI of the MI355X (gfx950) ORB front end + local-BA edge kernels.
 *
 * Drop-in boundary for ONE hot path of sunshanlu/ORB_SLAM2_ROS2 (all citations relative to
 * src/ORB_SLAM2/ in that repository):
 *
 *   orbfe_extract*            replaces  ORBExtractor::ORBExtractor + ::extract
 *                                       (include/ORB_SLAM2/ORBExtractor.h:107-116, src/ORBExtractor.cc:205-214, 499-508),
 *                                       i.e. initPyramid (:278-320), extractFast (:331-387), Quadtree (:19-192),
 *                                       getGrayCentroid (:465-487) and computeBRIEF (:397-456)
 *   orbfe_get_pyramid         replaces  ORBExtractor::getPyramid()            (ORBExtractor.h:113)
 *   orbfe_get_scale_factors   replaces  ORBExtractor::getScaledFactors()      (ORBExtractor.h:116)
 *   orbfe_stereo_match        replaces  ORBMatcher::searchByStereo            (ORBMatcher.h:38, src/ORBMatcher.cc:18-81)
 *                                       incl. createRowIndexDB (:915-932), getBestMatch (:967-990),
 *                                       pixelSADMatch/SAD/getPitch (:841-905, :1002-1011)
 *   orbfe_match_bruteforce    replaces  ORBMatcher::getBestMatch / descDistance loops (src/ORBMatcher.cc:941-990)
 *   orbfe_stereo_batch_device           the same extract(L) + extract(R) + searchByStereo for a batch of stereo
 *                                       pairs whose images are already resident in device memory
 *                                       (Frame::Frame stereo ctor + Frame::createStereo, src/Frame.cc:85-111,
 *                                       include/ORB_SLAM2/Frame.h:313-322)
 *   orbfe_ba_eval_edges       replaces  the g2o edge evaluation that Optimizer::OptimizeLocalMap /
 *                                       OptimizePoseOnly drive (src/Optimizer.cc:225-442, :33-203):
 *                                       EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ computeError + linearizeOplus
 *                                       + RobustKernelHuber
 *
 * Conventions: plain C, caller owns every host buffer, the context owns every device buffer.  No call
 * throws or aborts; every call returns an orbfe_status and orbfe_last_error() gives the text of the calling
 * THREAD's last failed call.  Threading: calls on distinct contexts are thread-safe.  Calls on ONE context are
 * serialised by the library (a per-context lock every entry point takes -- the reference's matchers are called
 * from the Tracking, LocalMapping and LoopClosing threads), with one exception made for the reference's call
 * pattern -- Frame::Frame runs the left and the right ORBExtractor::extract on two std::threads
 * (src/Frame.cc:100-105): orbfe_extract_slot calls on DIFFERENT slots of one context run concurrently with each
 * other and with the other entry points (each slot has its own stream, pinned staging and launch graph); the
 * caller only has to keep a slot call away from calls that read or rewrite THAT slot (a stereo match on it, a
 * batch call over it).  A context used from several threads serves them one at a time: give every thread role
 * its own context where they should not wait for each other (host/orbfe_shim.hpp: matcherContext, solverContext).
 *
 * There is NO CPU fallback behind this interface: if no HIP device is usable, orbfe_create fails.
 */
#ifndef ORBFE_H_
#define ORBFE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBFE_ABI_VERSION 4
#define ORBFE_MAX_LEVELS 16
#define ORBFE_DESC_BYTES 32

typedef enum orbfe_status {
  ORBFE_OK = 0,
  ORBFE_EBADARG = 1,   /* NULL pointer, index out of range, unsupported parameter              */
  ORBFE_EBADSIZE = 2,  /* reference: ImageSizeError (src/ORBExtractor.cc:310-314) and friends   */
  ORBFE_EDEVICE = 3,   /* HIP runtime error / no gfx950 device                                  */
  ORBFE_ECAPACITY = 4, /* batch larger than max_images, output buffer too small                 */
  ORBFE_ENOMEM = 5
} orbfe_status;

/* Same memory layout as cv::KeyPoint {Point2f pt; float size, angle, response; int octave, class_id} (28 B). */
typedef struct orbfe_keypoint {
  float x, y;      /* level-0 coordinates: level coordinate * scale[octave] (src/ORBExtractor.cc:408-409) */
  float size;      /* 7.0 (cv::FAST)                                                                     */
  float angle;     /* signed degrees in (-180,180] (src/ORBExtractor.cc:407)                             */
  float response;  /* FAST score                                                                         */
  int32_t octave;
  int32_t class_id; /* -1 */
} orbfe_keypoint;

typedef struct orbfe_config {
  int32_t width, height;       /* level-0 image size (e.g. 1241x376 KITTI, 640x480 TUM); each <= 4096    */
  int32_t n_features;          /* ORBExtractor.nFeatures.  No limit besides 65535 (indices of the stereo row table are 16 bit):
                                  a level whose quota exceeds ~2700 keypoints (nFeatures > ~12000 at 8 levels x 1.2) keeps its
                                  quadtree node table in global memory instead of one CU's LDS -- exact, slower.
                                  (One more deviation, harmless: the quadtree's split loop is capped at 80 N + 1024 steps for N
                                  candidates; the reference's degenerate case -- fewer candidates than the quota, quirk Q3 -- ends
                                  by itself after ~50 halvings per point, far below the cap.)                              */
  int32_t n_levels;            /* ORBExtractor.nLevels (<= ORBFE_MAX_LEVELS)                            */
  float scale_factor;          /* ORBExtractor.scaleFactor                                              */
  int32_t fast_hi, fast_lo;    /* ORBExtractor.iniThFAST / minThFAST                                    */
  const int8_t* brief_pairs;   /* 256 x {x1,y1,x2,y2}; NULL = the embedded table (config/brief_template.txt) */
  int32_t blur_variant;        /* cv::GaussianBlur 7x7 sigma 2, 8.8 fixed-point taps (un-vendored OpenCV):
                                  0: {18,34,48,56,48,34,18} (OpenCV >= 4.3, default)  1: {18,34,49,55,49,34,18}          */
  int32_t gray_variant;        /* cv::cvtColor RGB/BGR -> gray fixed-point coefficients (orbfe_extract_color only):
                                  0: 14-bit R 4899 G 9617 B 1868, (sum + 2^13) >> 14 (default)
                                  1: 15-bit R 9798 G 19235 B 3735, (sum + 2^14) >> 15 (newer OpenCV 4.x builds)           */
  int32_t device_id;           /* HIP device ordinal                                                    */
  int32_t max_images;          /* image slots held on the device (a stereo pair uses two)               */
  void* stream;                /* optional hipStream_t to run on; NULL = context-owned stream           */
} orbfe_config;

typedef struct orbfe_ctx orbfe_ctx;

/* Per-level geometry as the reference derives it (src/ORBExtractor.cc:283-317, 334-343). */
typedef struct orbfe_level_info {
  int32_t width, height;
  float scale;                 /* mvfScaledFactors[level]                                               */
  int32_t quota;               /* mvnFeatures[level]                                                    */
  int32_t grid_cols, grid_rows, cell_w, cell_h; /* FAST cell grid of extractFast                        */
} orbfe_level_info;

int orbfe_abi_version(void);
orbfe_status orbfe_create(const orbfe_config* cfg, orbfe_ctx** out);
void orbfe_destroy(orbfe_ctx* ctx);
const char* orbfe_last_error(const orbfe_ctx* ctx); /* ctx may be NULL: error of the last failed orbfe_create / orbfe_vocab_* call */

orbfe_status orbfe_get_level_info(const orbfe_ctx* ctx, int32_t level, orbfe_level_info* out);
orbfe_status orbfe_get_scale_factors(const orbfe_ctx* ctx, float* out, int32_t n);
/* Keypoints one image can yield = the stride of every per-image array of this API ("[n_features]" below means this number).
 * It equals n_features for every configuration the reference ships; it is larger only where the reference itself returns more
 * than nFeatures keypoints: its per-level quotas are rounded level by level and only the last level absorbs the difference
 * (src/ORBExtractor.cc:292-300), so e.g. nFeatures = 7 at 8 levels x 1.2 asks for 2 keypoints on each of seven levels.          */
int32_t orbfe_get_capacity(const orbfe_ctx* ctx);

/* ---- extraction (host buffers) ---------------------------------------------------------------
 * One image -> slot 0.  kps has room for n_features entries, desc for n_features*32 bytes.          */
orbfe_status orbfe_extract(orbfe_ctx* ctx, const uint8_t* img, size_t stride_bytes, orbfe_keypoint* kps, uint8_t* desc,
                           int32_t* n_out);
/* n_img images -> slots 0..n_img-1; kps/desc are [n_img][n_features] arrays, n_out[n_img].           */
orbfe_status orbfe_extract_batch(orbfe_ctx* ctx, int32_t n_img, const uint8_t* const* imgs, size_t stride_bytes,
                                 orbfe_keypoint* kps, uint8_t* desc, int32_t* n_out);
/* One image -> slot `slot` (0 <= slot < max_images), otherwise like orbfe_extract.  The drop-in for ORBExtractor::extract as
 * Frame::Frame calls it (src/Frame.cc:100-105): two extractor objects, two threads -- give each object its own slot; the results
 * stay resident in the slot for orbfe_stereo_match(ctx, slot_left, slot_right, ..) / orbfe_get_pyramid / orbfe_search_in_area.   */
orbfe_status orbfe_extract_slot(orbfe_ctx* ctx, int32_t slot, const uint8_t* img, size_t stride_bytes, orbfe_keypoint* kps,
                                uint8_t* desc, int32_t* n_out);
/* orbfe_extract_slot in two halves (ABI 4).  _begin stages the image and enqueues the whole extraction on the slot's lane, then RETURNS;
 * _end waits for it and delivers what orbfe_extract_slot delivers (kps / desc may be NULL: only the count; all NULL: just drain).  For the
 * reference's own construction order: `ORBExtractor::ORBExtractor(image, ...)` runs on the constructing thread BEFORE Frame::Frame starts
 * its two extract() threads (src/ORB_SLAM2/src/Frame.cc:91-105) and already does the pyramid there (src/ORBExtractor.cc:205-214) -- a
 * constructor that calls _begin lets the device work while the std::threads are being created (30 - 50 us each, p99 80 - 130 us on the
 * GPU boxes of the pool), and extract() is then only _end.  The image must stay readable until _begin returns; between _begin and _end
 * the slot accepts no other call (ORBFE_EBADARG), and every _begin must be followed by an _end, from any thread.                       */
orbfe_status orbfe_extract_slot_begin(orbfe_ctx* ctx, int32_t slot, const uint8_t* img, size_t stride_bytes);
orbfe_status orbfe_extract_slot_end(orbfe_ctx* ctx, int32_t slot, orbfe_keypoint* kps, uint8_t* desc, int32_t* n_out);
/* The same for n_img images into the consecutive slots slot .. slot + n_img - 1 as ONE launch sequence on slot's lane (arrays as
 * orbfe_extract_batch): both eyes of a stereo frame when one caller holds both images, about half the time of two slot calls.  (The C++
 * mirror keeps one orbfe_extract_slot per extract() thread, src/Frame.cc:100-105: pairing the two threads into one such call was
 * measured and dropped)  The call holds the lanes of all the slots it writes; a slot call on any of them waits.
 * Slot calls run concurrently with each other; they order themselves behind work the locked entry points left on the context
 * stream, which takes the context's API lock for a moment -- a long call that holds it (orbfe_ba_local_optimize holds it for the whole
 * optimisation) delays them: give the back end its own context.
 * LIFETIME of a slot's device-resident results: until the next extraction INTO THAT SLOT.  The drop-in extractor rotates each eye over
 * four slots (host/orbfe_dropin.hpp, ContextPool::kSlots), so a Frame's device-side features stay valid for the four extractions that
 * follow it -- orbfe_stereo_match / orbfe_search_in_area / orbfe_get_pyramid on an older Frame read a newer frame's data.            */
orbfe_status orbfe_extract_slots(orbfe_ctx* ctx, int32_t slot, int32_t n_img, const uint8_t* const* imgs, size_t stride_bytes,
                                 orbfe_keypoint* kps, uint8_t* desc, int32_t* n_out);
/* Copy one pyramid level of a slot to the host (tight rows).  blurred=0: the planes getPyramid() returns;
 * blurred=1: the Gaussian-blurred planes BRIEF samples (mvBriefMat).  dst needs width*height bytes.   */
orbfe_status orbfe_get_pyramid(orbfe_ctx* ctx, int32_t slot, int32_t level, int32_t blurred, uint8_t* dst);

/* ---- stereo matching over the device-resident results of the last extract --------------------
 * right_u / depth: n_features doubles each, -1 where unmatched (mvFeatsRightU / mvDepths).
 * best_right / best_dist (nullable, n_features int32): getBestMatch result before the thresholds
 * (-1 where the candidate list was empty).                                                           */
orbfe_status orbfe_stereo_match(orbfe_ctx* ctx, int32_t slot_left, int32_t slot_right, float fx, float bf, double* right_u,
                                double* depth, int32_t* n_matches, int32_t* best_right, int32_t* best_dist);

/* ---- one stereo frame, host images in, everything out: ONE call -------------------------------
 * The device work of Frame::createStereo (include/ORB_SLAM2/Frame.h:313-323: the Frame constructor, src/ORB_SLAM2/src/Frame.cc:85-110,
 * with ORBExtractor::extract on the left and the right image, then ORBMatcher::searchByStereo, src/ORB_SLAM2/src/ORBMatcher.cc:18):
 * left -> slot 0, right -> slot 1, their stereo match behind them in the same launch
 * sequence, one synchronisation.  kps / desc / n_out as orbfe_extract_batch with two images ([2][n_features]), right_u / depth as
 * orbfe_stereo_match.  Results are those of orbfe_extract_batch([left, right]) + orbfe_stereo_match(0, 1): the same kernels in the
 * same order; what the call saves is the second call's launch, copy and wake-up (tests/test_gpu_frame_stereo.py compares them).   */
orbfe_status orbfe_frame_stereo(orbfe_ctx* ctx, const uint8_t* left, const uint8_t* right, size_t stride_bytes, float fx, float bf,
                                orbfe_keypoint* kps, uint8_t* desc, int32_t* n_out, double* right_u, double* depth,
                                int32_t* n_matches);
/* The same into the slot pair (slot_left, slot_left + 1), slot_left even, on slot_left's lane -- concurrent with slot calls on other
 * slots, lifetime of the device-resident results as for orbfe_extract_slot (the drop-in's createStereo adapter rotates over the pairs
 * of its context: host/orbfe_dropin.hpp).                                                                                          */
orbfe_status orbfe_frame_stereo_slots(orbfe_ctx* ctx, int32_t slot_left, const uint8_t* left, const uint8_t* right, size_t stride_bytes,
                                      float fx, float bf, orbfe_keypoint* kps, uint8_t* desc, int32_t* n_out, double* right_u,
                                      double* depth, int32_t* n_matches);

/* ---- whole stereo pairs, images already in device memory --------------------------------------
 * d_left/d_right: device pointers to n_pairs images each, image p at base + p*image_pitch_bytes,
 * rows stride_bytes apart.  Pair p uses slots 2p (left) and 2p+1 (right).  Asynchronous on the
 * context stream; results stay on the device until fetched.  The images must be complete when the call
 * is made and stay unchanged until the call's first kernels have run (the resize reads them directly and
 * writes level 0 of the pyramid from them): do not overwrite them before orbfe_sync or a fetch of this
 * batch's results has returned (the host-image stream entry points manage their own ring of buffers). */
orbfe_status orbfe_stereo_batch_device(orbfe_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, size_t stride_bytes,
                                       size_t image_pitch_bytes, int32_t n_pairs, float fx, float bf);
orbfe_status orbfe_sync(orbfe_ctx* ctx);

/* ---- whole stereo pairs from HOST memory, copies overlapped with compute ------------------------
 * The loop of example/Stereo/KittiStereo.cc:28-37 (imread x2 -> Frame::createStereo) as a three-stage pipeline over batches: while
 * batch k is computed, batch k+1 is uploaded and the packed results of batch k-1 are downloaded (three input and three result buffers
 * on the device, one copy stream per direction).  left / right: n_pairs images each, image p at base + p * image_pitch_bytes, rows
 * stride_bytes apart.  orbfe_stream_submit returns at once with a ticket; the images must stay untouched, and `out` is not
 * valid, until orbfe_stream_wait(ticket) has returned.  At most THREE tickets may be outstanding (a fourth submit waits for the oldest).  Host memory from
 * orbfe_host_alloc (page-locked) makes both copies asynchronous DMA; ordinary memory works but the runtime stages it and the
 * overlap is lost.  The slots of the context hold the results of the newest submitted batch (pair p in slots 2p / 2p+1).
 * `out` arrays: kps [2 n_pairs][n_features], desc [2 n_pairs][n_features][32], counts [2 n_pairs] (slot order); right_u / depth
 * [n_pairs][n_features], n_matches [n_pairs]; entries past a slot's count are stale; any pointer may be NULL.                      */
typedef struct orbfe_batch_results {
  orbfe_keypoint* kps;
  uint8_t* desc;
  int32_t* counts;
  double* right_u;
  double* depth;
  int32_t* n_matches;
} orbfe_batch_results;
void* orbfe_host_alloc(size_t bytes); /* page-locked host memory (NULL on failure); release with orbfe_host_free */
/* ... placed on the NUMA node of HIP device `device_id` (< 0: the calling thread's current device, = orbfe_host_alloc): what a
 * multi-rank job calls with its own device, so that ranks which never called hipSetDevice do not all pin to GPU 0's node          */
void* orbfe_host_alloc_on(int32_t device_id, size_t bytes);
void orbfe_host_free(void* p);
/* Hardware queues the streaming entry points want (GPU_MAX_HW_QUEUES, read by the HIP runtime at the process's FIRST HIP call: the
 * process exports it, a library cannot).  orbfe_stream_submit prints one line on stderr when the variable is unset or below 8; the
 * one-frame-at-a-time entry points are faster with the runtime's default and never ask for it.                                   */
int32_t orbfe_recommended_hw_queues(void);
orbfe_status orbfe_stream_submit(orbfe_ctx* ctx, const uint8_t* left, const uint8_t* right, size_t stride_bytes,
                                 size_t image_pitch_bytes, int32_t n_pairs, float fx, float bf, const orbfe_batch_results* out,
                                 int64_t* ticket);
orbfe_status orbfe_stream_wait(orbfe_ctx* ctx, int64_t ticket);
/* Device pointers of the packed results of `ticket` (same arrays and strides as orbfe_batch_results), for consumers that stay on
 * the device (a gather over RCCL): complete once orbfe_stream_wait(ticket) has returned, valid until ticket + 3 is submitted.      */
orbfe_status orbfe_stream_device_results(orbfe_ctx* ctx, int64_t ticket, int32_t n_pairs, const void** d_kps, const void** d_desc,
                                         const void** d_counts, const void** d_right_u, const void** d_depth, const void** d_nmatch);
/* Fetch the results of slot (keypoints/descriptors) and, for a left slot, of its pair. Any pointer may be NULL. */
orbfe_status orbfe_fetch_features(orbfe_ctx* ctx, int32_t slot, orbfe_keypoint* kps, uint8_t* desc, int32_t* n_out);
orbfe_status orbfe_fetch_stereo(orbfe_ctx* ctx, int32_t pair, double* right_u, double* depth, int32_t* n_matches,
                                int32_t* best_right, int32_t* best_dist);
/* The packed results of slots [slot0, slot0 + n_slots) / pairs [pair0, pair0 + n_pairs) in one copy per array, full strides:
 * kps [n_slots][n_features], desc [n_slots][n_features][32], counts [n_slots]; right_u / depth [n_pairs][n_features], n_matches
 * [n_pairs].  Entries past a slot's count are stale.  Any pointer may be NULL.                                                */
orbfe_status orbfe_fetch_batch(orbfe_ctx* ctx, int32_t slot0, int32_t n_slots, orbfe_keypoint* kps, uint8_t* desc, int32_t* counts);
orbfe_status orbfe_fetch_stereo_batch(orbfe_ctx* ctx, int32_t pair0, int32_t n_pairs, double* right_u, double* depth,
                                      int32_t* n_matches);
/* Frame records of a ticket for the sequence-level gather: one fixed-size record per pair, what Frame::createStereo leaves
 * for the tracker -- int32 n_keypoints | int32 n_matches | 8 bytes pad | LEFT keypoints [n_features x 28 B] | LEFT descriptors
 * [n_features x 32 B] | right_u [n_features] f64 | depth [n_features] f64, entries past the count zeroed -- written to caller-provided
 * DEVICE memory (n_pairs * orbfe_record_bytes(ctx) bytes; e.g. a torch tensor handed to an RCCL gather).  Returns when the records
 * are complete.  The ticket must be live (submitted, and ticket + 3 not yet submitted).                                            */
size_t orbfe_record_bytes(const orbfe_ctx* ctx);
orbfe_status orbfe_stream_pack_records(orbfe_ctx* ctx, int64_t ticket, int32_t n_pairs, void* d_records);
/* Device pointers of the packed per-slot results, for gathers that never touch the host
 * (keypoints [max_images][n_features] orbfe_keypoint, descriptors [max_images][n_features][32],
 * counts [max_images] int32, right_u/depth [max_images/2][n_features] double).                       */
orbfe_status orbfe_device_results(orbfe_ctx* ctx, const void** d_kps, const void** d_desc, const void** d_counts,
                                  const void** d_right_u, const void** d_depth, const void** d_nmatch);

/* ---- brute-force Hamming-256 best / second-best (host buffers) --------------------------------
 * q: nq*32 bytes, t: nt*32 bytes.  Candidate lists in CSR form: query i scans train indices
 * cand_idx[cand_offsets[i] .. cand_offsets[i+1]) IN THAT ORDER (order matters, quirk Q6);
 * cand_offsets == NULL means "all nt, ascending".  Outputs per query: best_idx (-1 if no candidate),
 * best_dist, second_dist (INT32_MAX if none) exactly as ORBMatcher::getBestMatch computes them.       */
orbfe_status orbfe_match_bruteforce(orbfe_ctx* ctx, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt,
                                    const uint32_t* cand_offsets, const uint32_t* cand_idx, int32_t* best_idx,
                                    int32_t* best_dist, int32_t* second_dist);

/* ---- local-BA edge evaluation (fp64) ----------------------------------------------------------- */
typedef struct orbfe_ba_problem {
  int32_t n_poses, n_points, n_edges;
  const double* poses;       /* [n_poses][7]  qx,qy,qz,qw, tx,ty,tz  (g2o::SE3Quat of VertexSE3Expmap)   */
  const double* points;      /* [n_points][3] (VertexPointXYZ)                                          */
  const int32_t* edge_pose;  /* [n_edges]                                                               */
  const int32_t* edge_point; /* [n_edges]                                                               */
  const double* meas;        /* [n_edges][3]  u, v, u_right (u_right ignored for mono edges)            */
  const uint8_t* is_stereo;  /* [n_edges]     1: EdgeStereoSE3ProjectXYZ, 0: EdgeSE3ProjectXYZ           */
  const double* info;        /* [n_edges]     information = info * I                                    */
  const double* huber_delta; /* [n_edges]     <= 0: no robust kernel                                    */
  double fx, fy, cx, cy, bf;
} orbfe_ba_problem;

typedef struct orbfe_ba_edge_out {
  double* error;    /* [n_edges][3]  (3rd component 0 for mono)                                         */
  double* chi2;     /* [n_edges]                                                                        */
  double* rho;      /* [n_edges][2]  robustified chi2 rho(chi2), weight rho'(chi2)                      */
  double* j_point;  /* [n_edges][3][3] d e / d point (rows 0-1 used for mono), nullable                 */
  double* j_pose;   /* [n_edges][3][6] d e / d (omega, upsilon), nullable                               */
  uint8_t* depth_positive; /* [n_edges] isDepthPositive(), nullable                                     */
} orbfe_ba_edge_out;

/* DIAGNOSTIC entry points (this one and orbfe_ba_build_system): they return the per-edge Jacobians / the normal-equation blocks of ONE
 * linearisation to the host -- 4.8 MB over PCIe for the 15 597 edges of BASELINE config 5, which is why the host-array call takes about
 * as long as one CPU core needs for the arithmetic (0.42 vs 0.46 ms; the kernel itself 10 us).  They exist so that the edge formulas and
 * the quadratic form can be checked against the oracle; the optimisers (orbfe_ba_local_optimize, orbfe_pose_only_optimize,
 * orbfe_track_local_map) evaluate, build and solve on the device and move only poses, points and flags.                              */
orbfe_status orbfe_ba_eval_edges(orbfe_ctx* ctx, const orbfe_ba_problem* prob, const orbfe_ba_edge_out* out);

/* Normal-equation blocks of one linearisation, laid out like g2o's BlockSolver_6_3 (src/Optimizer.h:49-54): replaces
 * BaseBinaryEdge::constructQuadraticForm over all edges (what optimizer.optimize() runs per LM iteration under
 * Optimizer::OptimizeLocalMap, src/Optimizer.cc:336,361).  W = rho'(chi2) * info * I per edge (Huber as configured);
 * pose_fixed[k] != 0 => vertex k gets no blocks (setFixed, Optimizer.cc:248,288); points are the marginalised set.  */
typedef struct orbfe_ba_system_out {
  double* Hpp;  /* [n_poses][6][6]  sum B^T W B            (zero for fixed poses)                         */
  double* bp;   /* [n_poses][6]     - sum B^T W e                                                          */
  double* Hll;  /* [n_points][3][3] sum A^T W A                                                            */
  double* bl;   /* [n_points][3]    - sum A^T W e                                                          */
  double* Hpl;  /* [n_edges][6][3]  B^T W A of the edge (zero if its pose is fixed), nullable              */
} orbfe_ba_system_out;
orbfe_status orbfe_ba_build_system(orbfe_ctx* ctx, const orbfe_ba_problem* prob, const uint8_t* pose_fixed /*[n_poses], nullable*/,
                                   const orbfe_ba_system_out* out);

/* The g2o part of Optimizer::OptimizeLocalMap (include/ORB_SLAM2/Optimizer.h:69, src/Optimizer.cc:336-391) on the graph the
 * caller built (:232-330): optimize(iters_first = 5) with the problem's Huber deltas, then every edge with chi2 > 5.991 (mono) /
 * 7.815 (stereo) or non-positive depth goes to level 1 and ALL robust kernels are dropped (:338-359), optimize(iters_second = 10)
 * on level 0, final computeError() + the same test on every edge (:364-391).  BlockSolver_6_3 + OptimizationAlgorithmLevenberg
 * semantics (lambda0 = 1e-5 max diag, gain ratio, <= 10 trials per iteration, points marginalised by Schur complement); the
 * reduced system is factorised densely, by one of four Cholesky solvers -- no bound on the number of non-fixed keyframes, as
 * Optimizer.cc:232 has none:
 *   Levenberg-Marquardt control on the device, 1..42 non-fixed keyframes      one workgroup, the matrix in registers
 *   Levenberg-Marquardt control on the device, 43..1000                       48x48 tiles on the fp64 matrix cores, many workgroups
 *   host-driven Levenberg-Marquardt loop, up to 100                           one workgroup out of LDS, 6x6 blocks
 *   host-driven Levenberg-Marquardt loop, beyond 100                          the same with its panel in global memory, many workgroups
 * (the host-driven loop runs when a pose observes a point twice, beyond 1000 non-fixed keyframes, or with ORBFE_LBA_HOST_LM=1 in the
 * environment at orbfe_create; orbfe_debug_reduced_solve reaches each solver directly).  stop_flag (nullable) is polled like g2o's
 * forceStopFlag (Optimizer.cc:230): it points at ONE BYTE, the reference's `bool mbAbortBA` (include/ORB_SLAM2/LocalMapping.h:185) passed as
 * `bool& isStop` (Optimizer.h:69) -- only that byte is read, non-zero = stop.  The map bookkeeping of :393-441 stays with the caller.                               */
typedef struct orbfe_ba_optimize_out {
  double* poses;         /* [n_poses][7]  optimised estimates (fixed poses unchanged)                          */
  double* points;        /* [n_points][3]                                                                     */
  uint8_t* level;        /* [n_edges] 1: excluded from the second round (setLevel(1)), nullable                 */
  double* chi2;          /* [n_edges] chi2 at the final estimates, nullable                                    */
  uint8_t* bad;          /* [n_edges] final chi2 / depth test failed (the vToProcess candidates), nullable       */
  int32_t* iterations;   /* [2] Levenberg iterations run by the two optimize() calls, nullable                  */
} orbfe_ba_optimize_out;
orbfe_status orbfe_ba_local_optimize(orbfe_ctx* ctx, const orbfe_ba_problem* prob, const uint8_t* pose_fixed /*[n_poses], nullable*/,
                                     int32_t iters_first, int32_t iters_second, const volatile uint8_t* stop_flag,
                                     const orbfe_ba_optimize_out* out);

/* ---- global bundle adjustment: Optimizer::globalOptimization from the point where the graph is built (src/Optimizer.cc:934-1043) ----
 * ONE SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg on the graph type of orbfe_ba_local_optimize: no
 * classification round, no second round, then one computeError() on every edge at the final estimates.  A global BA runs on every
 * keyframe of the map, so its reduced camera system is large and block-sparse (consecutive keyframes share points, a loop adds a few
 * far blocks): solver 2 builds it as 6x6 block-CSR and solves it by a block-Jacobi preconditioned conjugate gradient in fp64 (x0 = 0,
 * stop at r.M^-1 r <= pcg_tol^2 b.M^-1 b; no convergence within pcg_max_iter, or p.Sp not positive and finite, rejects the Levenberg trial
 * as a bad pivot of the dense solvers does).  solver 1 is orbfe_ba_local_optimize(iterations, 0), its poses, points and chi2.  solver 0
 * chooses by the number of non-fixed keyframes alone: 1 up to ORBFE_GBA_DENSE_MAX_FREE, 2 past it (the measured crossover: up to there
 * the local BA's device-side solvers are faster, past it they give way to the panel solver).  Every sum has a fixed order: a
 * repeated call is bit-identical.  stop_flag as in orbfe_ba_local_optimize.  n_edges == 0 returns the inputs.                         */
#define ORBFE_GBA_DENSE_MAX_FREE 1000
typedef struct orbfe_ba_global_options {
  int32_t solver;        /* 0 auto, 1 dense (the local BA's solvers), 2 block-sparse PCG                          */
  double pcg_tol;        /* <= 0: 1e-10                                                                         */
  int32_t pcg_max_iter;  /* <= 0: 4 * 6 * (non-fixed keyframes)                                                 */
} orbfe_ba_global_options;
typedef struct orbfe_ba_global_out {
  double* poses;         /* [n_poses][7]  optimised estimates (fixed poses unchanged)                            */
  double* points;        /* [n_points][3]                                                                       */
  double* chi2;          /* [n_edges] chi2 at the final estimates, nullable                                      */
  int32_t* iterations;   /* [1] Levenberg iterations run, nullable                                               */
  int64_t* cg_stats;     /* [3] trials, CG iterations in all, trials the solver rejected (zeros for solver 1); nullable */
} orbfe_ba_global_out;
orbfe_status orbfe_ba_global_optimize(orbfe_ctx* ctx, const orbfe_ba_problem* prob, const uint8_t* pose_fixed /*[n_poses], nullable*/,
                                      int32_t iterations, const volatile uint8_t* stop_flag, const orbfe_ba_global_options* opt /*nullable*/,
                                      const orbfe_ba_global_out* out);

/* ---- grid-guided matching against the features of one slot ---------------------------------------------------------
 * Replaces VirtualFrame::initGrid + findFeaturesInArea (src/Frame.cc:53-69, 286-311) + ORBMatcher::getBestMatch
 * (src/ORBMatcher.cc:967-990), the core of the guided searches (ORBMatcher::searchByProjection, src/ORBMatcher.cc:265-347 and
 * :561-612): query i searches the 64x48-px grid cells overlapping [x-r, x+r] x [y-r, y+r] around qxy[i] with r = radius[i] (the
 * caller multiplies by getScaledFactor2(octave), Frame.cc:289), cells rows-outer / columns-inner, a cell's features in index
 * order, keeps octaves in [min_level[i], max_level[i]] and features with exclude[idx] == 0 (nullable: e.g. "already has a
 * map point", ORBMatcher.cc:322-332), and applies the reference's order-dependent best / second-best scan.  Outputs as
 * orbfe_match_bruteforce plus the candidate count; best_idx = -1 when the list is empty.  Cell indices are clamped to the
 * grid (the reference indexes one column past the grid when the box touches x == width and width is a multiple of 64).      */
orbfe_status orbfe_search_in_area(orbfe_ctx* ctx, int32_t slot, int32_t nq, const float* qxy /*[nq][2]*/, const float* radius,
                                  const int8_t* min_level, const int8_t* max_level, const uint8_t* q_desc /*[nq][32]*/,
                                  const uint8_t* exclude /*[n_features], nullable*/, int32_t* best_idx, int32_t* best_dist,
                                  int32_t* second_dist, int32_t* n_cand);

/* The same search against a feature set the CALLER supplies -- a KeyFrame's mvFeatsLeft / descriptors: keyframes are not resident in a
 * slot.  This is the core of the remaining guided searches, ORBMatcher::searchBySim3 x2 (src/ORBMatcher.cc:370-559, via
 * KeyFrame::findFeaturesInArea), and of searchByProjection / fuse when the target is a KeyFrame (:561-734).  t_kps: x, y, octave are
 * read; exclude: [nt] flags, nullable; the grid is the context's width x height.                                                  */
orbfe_status orbfe_search_in_area_features(orbfe_ctx* ctx, int32_t nt, const orbfe_keypoint* t_kps, const uint8_t* t_desc /*[nt][32]*/,
                                           int32_t nq, const float* qxy /*[nq][2]*/, const float* radius, const int8_t* min_level,
                                           const int8_t* max_level, const uint8_t* q_desc /*[nq][32]*/, const uint8_t* exclude,
                                           int32_t* best_idx, int32_t* best_dist, int32_t* second_dist, int32_t* n_cand);
/* ... with the two things the frame-level searchByProjection (src/ORBMatcher.cc:265-347) needs besides: `bounds` = {min_u, max_u, min_v,
 * max_v}, the target frame's undistorted image bounds (VirtualFrame::mfMinU..mfMaxV, include/ORB_SLAM2/Frame.h:33-43): initGrid sizes the
 * grid from them and findFeaturesInArea clips the search box at (int)max_u / (int)max_v (src/Frame.cc:55-56, :289-293); NULL = the image,
 * i.e. a camera without distortion.  `excluded_hits` [nt], nullable: for every EXCLUDED feature how many queries had it inside their
 * window and octave range -- the reference calls MapPoint::addMatchInTrack once per such occurrence while it drops the feature from
 * the candidate list (ORBMatcher.cc:321-331); entries of features that are not excluded are 0.                                        */
orbfe_status orbfe_search_in_area_features_ex(orbfe_ctx* ctx, int32_t nt, const orbfe_keypoint* t_kps, const uint8_t* t_desc /*[nt][32]*/,
                                              const float* bounds /*[4], nullable*/, int32_t nq, const float* qxy /*[nq][2]*/,
                                              const float* radius, const int8_t* min_level, const int8_t* max_level,
                                              const uint8_t* q_desc /*[nq][32]*/, const uint8_t* exclude, int32_t* best_idx,
                                              int32_t* best_dist, int32_t* second_dist, int32_t* n_cand, int32_t* excluded_hits);

/* ---- pose-only optimisation of one frame (fp64), entirely on the device -------------------------------------------
 * Replaces the g2o part of Optimizer::OptimizePoseOnly (include/ORB_SLAM2/Optimizer.h:72, src/Optimizer.cc:33-178): one SE3 pose
 * vertex, one unary edge per observed map point -- EdgeSE3ProjectXYZOnlyPose when u_right < 0 (Optimizer.cc:77), else
 * EdgeStereoSE3ProjectXYZOnlyPose -- information info[i]*I (the caller passes getScaledFactorInv2(octave), :85,:106), Huber
 * sqrt(5.991)/sqrt(7.815); 4 rounds x optimize(10) from the initial pose with the re-classification chi2 > 5.991*sigma2[i] /
 * 7.815*sigma2[i] (sigma2 = getScaledFactor2(octave), :136,:157) and the kernels dropped in the third round (:149,:170).
 * Outputs the optimised pose (qx qy qz qw tx ty tz), the inlier flag of every edge and `edges - nBad` of the last round.
 * The projection post-check of Optimizer.cc:180-190 (Frame::project2UV with the frame's float pose) stays with the caller.  */
orbfe_status orbfe_pose_only_optimize(orbfe_ctx* ctx, int32_t n, const double* xw /*[n][3]*/, const double* meas /*[n][3] u v uR*/,
                                      const double* info /*[n]*/, const float* sigma2 /*[n]*/, const double* pose_in /*[7]*/,
                                      double fx, double fy, double cx, double cy, double bf, double* pose_out /*[7]*/,
                                      uint8_t* inlier_out /*[n], nullable*/, int32_t* n_good);

/* ---- frame-level glue either side of the ORB path -----------------------------------------------------
 * orbfe_extract_color: Tracking::grabFrame's cv::cvtColor(COLOR_RGB2GRAY / COLOR_BGR2GRAY) (src/Tracking.cc:55-68) fused in front of
 * orbfe_extract (slot 0): img is 8-bit 3-channel interleaved, color_order 1 = RGB, 2 = BGR (the reference's Camera.Color values);
 * the grey image becomes level 0 of the pyramid (orbfe_get_pyramid(ctx, 0, 0, 0, ..) returns it).
 * orbfe_frame_rgbd: for the keypoints of `slot`, Camera::undistortPoints (src/Camera.cc:29-39; no-op when k1 == 0) IN PLACE on the
 * device-resident keypoints -- so the feature grid of orbfe_search_in_area sees undistorted positions as VirtualFrame::initGrid does
 * (Frame.cc:108,148) -- and, when depth != NULL, the RGB-D tail of Frame::Frame (src/Frame.cc:136-158): depth read at the
 * DISTORTED keypoint with truncated indices, divided by depth_scale in float, depth_out = d and right_u_out = x_undist - bf / d
 * where d > 0, else -1.  depth_type 0: uint16 image, 1: float image; rows depth_stride_bytes apart (host memory).
 * Strides: a colour image's stride_bytes is at least 3 * width; depth_stride_bytes is at least width elements AND a multiple of the
 * element size (2 or 4 bytes) -- anything else is ORBFE_EBADARG.  Either image may be a column range of a larger one (a cv::Mat ROI,
 * stride = Mat::step): nothing behind the last element of the LAST row is read, i.e. stride * (height - 1) + width * element bytes.
 * Outputs [n_features] (entries past the keypoint count are -1), any may be NULL.  Stereo rigs are taken as rectified (k1 == 0,
 * the reference's only stereo configuration): orbfe_stereo_match does not undistort.                                          */
typedef struct orbfe_camera {
  float fx, fy, cx, cy;      /* Camera::mK as the reference stores it (float)                    */
  float k1, k2, p1, p2, k3;  /* Camera::mDistCoeff                                                */
  float bf;                  /* Camera::mfBf                                                      */
} orbfe_camera;
orbfe_status orbfe_extract_color(orbfe_ctx* ctx, const uint8_t* img, size_t stride_bytes, int32_t color_order, orbfe_keypoint* kps,
                                 uint8_t* desc, int32_t* n_out);
/* The device work of Frame::createRGBD (include/ORB_SLAM2/Frame.h:326-331) as ONE call: cv::cvtColor of Tracking::grabFrame when
 * color_order is 1 (RGB) or 2 (BGR) -- 0: the image is gray already -- (src/Tracking.cc:55-68), the extraction into `slot` (the RGB-D
 * Frame constructor, src/ORB_SLAM2/src/Frame.cc:125-135), then the constructor's tail: Camera::undistortPoints and the depth / rightU
 * lookup (:136-158).  One launch sequence on the slot's lane, one synchronisation; the depth image is not uploaded (the last kernel reads
 * one value per keypoint from the page-locked staging copy).  Results as orbfe_extract_color / orbfe_extract_slot followed by
 * orbfe_frame_rgbd (tests/test_frame_glue.py compares them): kps_undistorted / desc [n_features], depth_out / right_u_out [n_features]
 * (-1 where there is no depth), nullable.                                                                                          */
orbfe_status orbfe_frame_rgbd_image(orbfe_ctx* ctx, int32_t slot, const uint8_t* img, size_t stride_bytes, int32_t color_order,
                                    const orbfe_camera* cam, const void* depth, int32_t depth_type, size_t depth_stride_bytes,
                                    float depth_scale, orbfe_keypoint* kps_undistorted, uint8_t* desc, int32_t* n_out, double* depth_out,
                                    double* right_u_out);
orbfe_status orbfe_frame_rgbd(orbfe_ctx* ctx, int32_t slot, const orbfe_camera* cam, const void* depth, int32_t depth_type,
                              size_t depth_stride_bytes, float depth_scale, orbfe_keypoint* kps_undistorted, double* depth_out,
                              double* right_u_out);

/* MapPoint::isInVision + MapPoint::predictLevel (src/MapPoint.cc:141-201) for n map points against one frame -- the per-point
 * preamble of ORBMatcher::searchByProjection(frame, mapPoints, ...) (src/ORBMatcher.cc:575-580), whose outputs feed
 * orbfe_search_in_area.  pose: Rcw row-major + tcw as the reference's float cv::Mat; bounds: VirtualFrame::mfMinU, mfMaxU, mfMinV,
 * mfMaxV (Frame.h:259-264).  Outputs per point: projection uv, camera-centre distance, cosTheta, predicted level (clamped to
 * [0, 7] like the reference) and visible = isInVision's return value; a point that fails a test keeps visible = 0 and the
 * values computed up to that test.  Float arithmetic in the reference's order (documented in csrc/k_guided.hip).              */
typedef struct orbfe_frame_pose {
  float Rcw[9], tcw[3];
  float min_u, max_u, min_v, max_v;
} orbfe_frame_pose;
orbfe_status orbfe_project_map_points(orbfe_ctx* ctx, int32_t n, const float* pos /*[n][3]*/, const float* view_dir /*[n][3]*/,
                                      const float* max_dist /*[n]*/, const float* min_dist /*[n]*/, const orbfe_frame_pose* pose,
                                      const orbfe_camera* cam, float* uv /*[n][2]*/, float* distance /*[n]*/, float* cos_theta /*[n]*/,
                                      int8_t* level /*[n]*/, uint8_t* visible /*[n]*/);

/* ---- the tracking chain of one frame as ONE call -------------------------------------------------------------------------
 * Tracking::trackLocalMap (src/Tracking.cc:641-675) calls ORBMatcher::searchByProjection(frame, local map points, th)
 * (src/ORBMatcher.cc:561-612: MapPoint::isInVision + predictLevel per point, findFeaturesInArea + getBestMatch, then the assignment
 * in map-point order -- a feature that holds a good map point keeps it, a free one goes to the first point whose best match it is)
 * and then Optimizer::OptimizePoseOnly(frame) (src/Optimizer.cc:33-178) on what the frame holds.  Called one by one
 * (orbfe_project_map_points, orbfe_search_in_area, orbfe_pose_only_optimize) that is three host -> device -> host round trips with the
 * map points and the frame's features marshalled each time; here the frame's features are the device-resident results of `slot`, the
 * map points go up once, and the projections, windows, candidate lists, assignment and edge list stay on the device.
 * flags[i]: bit 0 = !isBad && isInMap, bit 1 = !isBad, bit 2 = member of the list searchByProjection walks (a point the frame holds
 * from an earlier stage but that is not in the local map carries bits 0-1 only: not searched, still an edge).
 * Outputs: assigned[f] = index of the map point feature f holds after the search (-1: none); n_matches = searchByProjection's return
 * value; when n_matches >= min_matches (else n_edges = -1, pose_out = pose_se3, no inliers -- trackLocalMap returns false there):
 * n_edges, n_good = edges - nBad after the four rounds, pose_out (qx qy qz qw tx ty tz), inlier[f] = 1 where feature f's edge ended
 * as an inlier.  The projection post-check (Optimizer.cc:180-190) and the map points' counters stay with the caller, as in
 * orbfe_pose_only_optimize.  At most 2048 features per frame.                                                                    */
typedef struct orbfe_track_input {
  int32_t n_mp;
  const float* pos;              /* [n_mp][3] MapPoint::getPos()                                                   */
  const float* view_dir;         /* [n_mp][3]                                                                      */
  const float* max_dist;         /* [n_mp]                                                                         */
  const float* min_dist;         /* [n_mp]                                                                         */
  const uint8_t* desc;           /* [n_mp][32] MapPoint::getDesc()                                                 */
  const uint8_t* flags;          /* [n_mp], see above                                                              */
  const int32_t* held;           /* [n_features], nullable: map point (index) a feature holds on entry, -1 none    */
  const double* right_u;         /* [n_features], nullable (every edge mono): Frame::getRightU                     */
  const float* level_sigma2;     /* [n_levels] VirtualFrame::getScaledFactor2(level)                               */
  const float* level_inv_sigma2; /* [n_levels] getScaledFactorInv2(level)                                          */
  const double* pose_se3;        /* [7] Converter::ConvertTcw2SE3(mRcw, mtcw): the optimisation's initial estimate */
  float th;                      /* searchByProjection's th (Tracking.cc:645-649: 3, or 5 after a relocalisation)  */
  float ratio;                   /* ORBMatcher::mfRatio (0.8 in trackLocalMap)                                     */
  int32_t min_threshold;         /* ORBMatcher::mnMinThreshold (50)                                                */
  int32_t min_matches;           /* Tracking.cc:656: below this many matches no optimisation (30)                  */
} orbfe_track_input;
typedef struct orbfe_track_output {
  int32_t* assigned;  /* [n_features]                                  */
  int32_t* edge_of;   /* [n_features], nullable: edge index of a feature in the optimisation (-1 none) */
  uint8_t* inlier;    /* [n_features]                                  */
  int32_t *n_matches, *n_edges, *n_good;
  double* pose_out;   /* [7]                                           */
} orbfe_track_output;
orbfe_status orbfe_track_local_map(orbfe_ctx* ctx, int32_t slot, const orbfe_frame_pose* pose, const orbfe_camera* cam,
                                   const orbfe_track_input* in, const orbfe_track_output* out);

/* The middle of Tracking::trackMotionModel (src/Tracking.cc:382-396) as ONE call: ORBMatcher::searchByProjection(frame, lastFrame, matches, th)
 * -- in this reference a search around the LAST frame's feature positions within th * getScaledFactor2(octave) pixels (VirtualFrame::
 * findFeaturesInArea, src/Frame.cc:286-311: by grid cell), octave window by the motion direction, among the
 * frame's features that hold no map point yet, accepted when ratio < mfRatio and distance < mnMinThreshold; every accepted query is a match
 * and setMapPoints assigns them in query order, so the last query that picked a feature keeps it (src/ORBMatcher.cc:265-347, :815-830) --
 * then, with fewer than min_matches matches, the same search with th_second among the features still free (Tracking.cc:388-391; the
 * matches of the first stay), then Optimizer::OptimizePoseOnly(frame).  The frame's features are the device-resident results of `slot`.
 * Queries = the last frame's features that hold a good map point, in feature order (the caller's filter, :286-289).
 * Outputs as orbfe_track_local_map (assigned[f] = query index); n_matches = the accepted queries of all passes; excluded_hits[f]
 * (nullable) = how many queries met feature f among their candidates while it held a map point (the addMatchInTrack calls of :322-331);
 * query_matches[i] (nullable, [n]) = in how many of the searches query i was accepted as a match (setMapPoints calls addMatchInTrack for
 * every match, whether a later query takes the feature over or not); passes (nullable) = 1 or 2.  The second search is decided on the
 * host.  At most 2048 features per frame.                                                                                            */
typedef struct orbfe_motion_input {
  int32_t n;
  const float* qxy;              /* [n][2] the last frame's (undistorted) feature positions: the search centres            */
  const int8_t* q_octave;        /* [n] their octaves: findFeaturesInArea searches within th * getScaledFactor2(octave)     */
  const int8_t* q_min_level;     /* [n] octave window (:300-315: [octave, 7] forward, [0, octave] backward, else +-1)       */
  const int8_t* q_max_level;     /* [n]                                                                                    */
  const uint8_t* desc;           /* [n][32] the last frame's descriptors                                                   */
  const float* pos;              /* [n][3] the map points' positions (the pose-only edges)                                 */
  const int32_t* held;           /* [n_features], nullable: query index a feature of the frame holds on entry, -1 none     */
  const double* right_u;         /* [n_features], nullable                                                                 */
  const float* level_sigma2;     /* [n_levels]                                                                             */
  const float* level_inv_sigma2; /* [n_levels]                                                                             */
  const double* pose_se3;        /* [7] the predicted pose: the optimisation's initial estimate                            */
  float th, th_second;           /* 15, 30 (Tracking.cc:387, 390); th_second <= 0: no second search                        */
  float ratio;                   /* ORBMatcher::mfRatio (0.9 in trackMotionModel)                                          */
  int32_t min_threshold;         /* ORBMatcher::mnMinThreshold                                                             */
  int32_t min_matches;           /* 20 (Tracking.cc:388, 392)                                                              */
} orbfe_motion_input;
orbfe_status orbfe_track_motion_model(orbfe_ctx* ctx, int32_t slot, const float* bounds4 /* mfMinU mfMaxU mfMinV mfMaxV */, const orbfe_camera* cam,
                                      const orbfe_motion_input* in, const orbfe_track_output* out, int32_t* excluded_hits, int32_t* query_matches,
                                      int32_t* passes);

/* ---- map.pb: the reference's on-disk map, and a local bundle adjustment on it -------------------------------
 * `orbslam2.MapData` as Map::saveToProtobuf writes it (src/Map.cc:200-250; proto/Map.proto, Keyframe.proto,
 * MapPoint.proto), read and written without libprotobuf (host/map_pb.hpp).  The first three calls are host-only
 * (no context, no device).  Output buffers follow the "size query" convention: *out_len receives the size needed;
 * with out == NULL or cap too small nothing is written and ORBFE_ECAPACITY is returned (ORBFE_OK for out == NULL). */
typedef struct orbfe_map_summary {
  uint64_t next_id;        /* KeyFrameList.next_id (KeyFrame::mnNextId)                                   */
  int32_t n_scale_factors; /* KeyFrameList.scale_factors (KeyFrame::mvfScaledFactors)                     */
  int32_t n_keyframes, n_mappoints;
  int64_t n_keypoints;     /* over all keyframes                                                          */
  int64_t n_observations;  /* keypoints that carry a map point id (map_points[i] != -1)                   */
} orbfe_map_summary;
/* Map::loadFromProtobuf's parse (src/Map.cc:263-267); ORBFE_EBADARG for a malformed file                  */
orbfe_status orbfe_map_pb_summary(const uint8_t* pb, size_t len, orbfe_map_summary* out);
/* parse + serialise: the canonical encoding libprotobuf's C++ serialiser produces for the same content    */
orbfe_status orbfe_map_pb_reencode(const uint8_t* pb, size_t len, uint8_t* out, size_t cap, size_t* out_len);

/* The reference's other on-disk format, the TEXT map of Map::saveToTxtFile / loadFromTxtFile (src/Map.cc:82-165): `KeyFrames.txt`
 * (one header line + 10 lines per keyframe, KeyFrame.cc:400-530) and `MapPoints.txt` (3 lines per map point, MapPoint.cc:538-596), as
 * conversions to and from map.pb (host/map_txt.hpp; numbers formatted by iostreams exactly like the reference: 6 significant digits,
 * so the text form is lossy).  Size-query convention as above, for both outputs.                                                  */
orbfe_status orbfe_map_pb_to_txt(const uint8_t* pb, size_t len, char* kf_out, size_t kf_cap, size_t* kf_len, char* mp_out, size_t mp_cap,
                                 size_t* mp_len);
orbfe_status orbfe_map_txt_to_pb(const char* kf_txt, size_t kf_len, const char* mp_txt, size_t mp_len, uint8_t* out, size_t cap,
                                 size_t* out_len);

/* The graph Optimizer::OptimizeLocalMap builds around keyframe kf_id (src/Optimizer.cc:232-330): vertices =
 * [covisible keyframes (weight > 15, descending) + kf_id | fixed observers], map points of the free group in
 * ascending id, one edge per observation (stereo iff right_u > 0; information getScaledFactorInv2 / Inv, quirk Q9).
 * sizes[4] = {n_poses, n_group, n_points, n_edges}; every array pointer may be NULL (size query), else it must
 * hold the counts a previous call returned.                                                                  */
typedef struct orbfe_map_graph {
  uint64_t* pose_kf_id;  /* [n_poses]                                                                       */
  uint8_t* pose_fixed;   /* [n_poses]  setFixed                                                             */
  double* poses;         /* [n_poses][7] Converter::ConvertTcw2SE3                                          */
  uint64_t* point_id;    /* [n_points]                                                                      */
  double* points;        /* [n_points][3]                                                                   */
  int32_t* edge_pose;    /* [n_edges] vertex index                                                          */
  int32_t* edge_point;   /* [n_edges] point index                                                           */
  int32_t* edge_feat;    /* [n_edges] keypoint index inside the observing keyframe                          */
  double* meas;          /* [n_edges][3]                                                                    */
  uint8_t* is_stereo;    /* [n_edges]                                                                       */
  double* info;          /* [n_edges]                                                                       */
  double* huber_delta;   /* [n_edges]                                                                       */
} orbfe_map_graph;
orbfe_status orbfe_map_local_graph(const uint8_t* pb, size_t len, uint64_t kf_id, int32_t sizes[4], const orbfe_map_graph* out);

/* Optimizer::OptimizeLocalMap(kf, isStop) (src/Optimizer.cc:225-441) on a map file: graph as above, the two
 * optimize() rounds on the device (orbfe_ba_local_optimize), then the reference's write-back policy (:363-441):
 * outlier observations erased and poses / points stored as float unless more than 20 % of the affected keyframes
 * would lose more than 30 % of their map points.  Camera::mfFx.. come from `cam` (fx fy cx cy bf).  Output: the
 * updated map.pb.  MapPoint::updateDescriptor / updateNormalAndDepth and KeyFrame::updateConnections (:436-440)
 * are map bookkeeping and are NOT applied.                                                                   */
typedef struct orbfe_map_ba_report {
  int32_t n_poses, n_group, n_points, n_edges;
  int32_t n_outlier_edges, n_keyframes_hit, n_bad_keyframes, written;
  int32_t iterations[2];
  double chi2_before, chi2_after; /* sum of robustified-free chi2 over all edges at the initial / final estimates */
} orbfe_map_ba_report;
orbfe_status orbfe_map_local_ba(orbfe_ctx* ctx, const uint8_t* pb, size_t len, uint64_t kf_id, const orbfe_camera* cam,
                                const volatile uint8_t* stop_flag, uint8_t* out, size_t cap, size_t* out_len,
                                orbfe_map_ba_report* report);

/* ---- bag of words: DBoW3's Vocabulary::transform on the device -----------------------------------
 * VirtualFrame::computeBow (include/ORB_SLAM2/Frame.h:224-231) runs mpVoc->transform(mvLeftDescriptor, mBowVec, mFeatVec, 4) for
 * searchByBow, every new keyframe and every relocalisation / loop query.  orbfe_vocab holds a vocabulary tree in the ORB-SLAM2 text
 * format (`Path.Vocabulary: ORBvoc.txt`); it is host data plus ONE device copy per HIP device, uploaded on the first transform on that
 * device and shared by every context there (a failed upload leaves nothing behind: the next call on that device tries again).
 * orbfe_vocab_destroy frees every device copy; no call that uses the vocabulary may still be running or queued.  It restores the
 * calling thread's current HIP device.
 *
 * Text format: line 1 `k L scoring weighting`; every further non-blank line is one node `parent_id is_leaf b0 .. b31 weight` (bytes in
 * decimal, weight a decimal number -- [+-]digits[.digits][e[+-]digits], read independently of the locale; no nan / inf / hex).
 * The root is the implicit node 0, node i is the i-th node line; a node's children keep file order; leaves get
 * word ids 0, 1, .. in file order.  ORBFE_EBADARG (text in orbfe_last_error(NULL)) for: a malformed header; k outside 2..20 or L outside
 * 1..10; scoring / weighting other than 0 0 (L1 norm, TF-IDF); is_leaf other than 0 / 1; parent_id >= own id or a leaf parent; more than
 * k children under a node; an inner node (the root included) without children; depth > L; a byte outside 0..255; a truncated line or
 * extra tokens.  Blank lines are skipped (DBoW2's `while (!f.eof())` loop makes a garbage node of a trailing empty line).             */
typedef struct orbfe_vocab orbfe_vocab;
typedef struct orbfe_vocab_info {
  int32_t k, L;
  int32_t n_nodes; /* root included */
  int32_t n_words;
} orbfe_vocab_info;
orbfe_status orbfe_vocab_load_txt(const char* path, orbfe_vocab** out);
orbfe_status orbfe_vocab_info_get(const orbfe_vocab* v, orbfe_vocab_info* out);
/* The parsed arrays in node-id order, n_nodes entries each (any pointer may be NULL): parent (-1 for the root), is_leaf, desc
 * [n_nodes][32] (zeros for the root), weight, word_id (-1 for inner nodes).                                                          */
orbfe_status orbfe_vocab_export(const orbfe_vocab* v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight, int32_t* word_id);
void orbfe_vocab_destroy(orbfe_vocab* v);

/* DBoW2 / DBoW3 TemplatedVocabulary::transform(features, v, fv, levelsup) for binary features under L1 / TF-IDF, bit-exact:
 *   descent   from the root; at each node the Hamming-256 distance to every child in file order, the FIRST minimum (strict <); stop at a leaf
 *   node      the node the path passes at level L - levelsup (the root if that is <= 0; the leaf itself if the leaf comes first -- DBoW
 *             leaves it unset there, a documented decision)
 *   skip      a feature whose leaf weight is not > 0 adds nothing (neither BowVector nor FeatureVector)
 *   BowVector words ascending; a word hit c times holds w + w + .. + w (c terms in sequence, BowVector::addWeight); then L1: norm = the
 *             sequential sum of |value| in ascending word order, value = value / norm when norm > 0
 *   FeatureVector  nodes ascending, each node's feature indices ascending
 * Outputs (host CSR, the capacity is the call's feature count / the context's n_features per slot): words / values [n_words]; nodes
 * [n_nodes], node_offsets [n_nodes + 1] into features [number of features kept].  Any array pointer may be NULL.                   */
typedef struct orbfe_bow_out {
  uint32_t* words;        /* [cap]     */
  double* values;         /* [cap]     */
  int32_t* n_words;       /* [1]       */
  uint32_t* nodes;        /* [cap]     */
  int32_t* node_offsets;  /* [cap + 1] */
  uint32_t* features;     /* [cap]     */
  int32_t* n_nodes;       /* [1]       */
} orbfe_bow_out;
#define ORBFE_BOW_MAX_FEATURES 65535
/* n host descriptors (n * 32 bytes), 0 <= n <= ORBFE_BOW_MAX_FEATURES (more: ORBFE_ECAPACITY), any levelsup >= 0; cap = n.           */
orbfe_status orbfe_bow_transform(orbfe_ctx* ctx, const orbfe_vocab* v, const uint8_t* desc, int32_t n, int32_t levelsup,
                                 const orbfe_bow_out* out);
/* The descriptors the last extraction left in slots slot0, slot0 + slot_step, .. (n_slots of them), read on the device (no upload).
 * slot_step 2 takes the left images of a batch of stereo pairs (pair p in slots 2p / 2p + 1) without the right ones.  Every out array is
 * [n_slots][cap] with cap = orbfe_get_capacity(ctx) (node_offsets [n_slots][cap + 1]); n_words / n_nodes are [n_slots].  Slot rules as
 * orbfe_fetch_batch.                                                                                                                 */
orbfe_status orbfe_bow_slots(orbfe_ctx* ctx, const orbfe_vocab* v, int32_t slot0, int32_t n_slots, int32_t slot_step, int32_t levelsup,
                             const orbfe_bow_out* out);

/* ---- keyframe database: KeyFrameDB's place-recognition query on the device ------------------------------------------------------
 * KeyFrameDB (src/KeyFrameDB.cc) answers Tracking::trackReLocalize (findRelocKfs, src/Tracking.cc:418) and LoopClosing::detectLoop
 * (findLoopCloseKfs, src/LoopClosing.cc:224).  orbfe_kfdb holds keyframes keyed by a uint64 id -- each one's BowVector (words strictly
 * ascending and < n_words, 0 .. ORBFE_BOW_MAX_FEATURES of them) -- on ONE device; any context on that device may query it (a context on
 * another device: ORBFE_EBADARG).  One lock per database serialises add, erase, set_bad and query (the reference's mMutex).
 *   add      keyframes as one CSR: keyframe i has words[offsets[i] .. offsets[i + 1]); an id already present is left as it is (OK: the
 *            reference's std::set); capacity grows as needed.  An invalid keyframe (unsorted / repeated / out-of-vocabulary words, a
 *            size beyond the limit, an id repeated inside the call) rejects the whole call with ORBFE_EBADARG and adds nothing.
 *   set_bad  KeyFrame::isBad() as the database sees it (flags[i] != 0: bad); bad keyframes stay listed and every query skips them.
 *            Unknown ids: ORBFE_EBADARG, nothing changed.
 *   erase    removes the ids (unknown ids are ignored, as std::set::erase does).
 *   query    the shared-word count of every listed keyframe that is not bad and not in `ignore`, then minWordFilter -- dropped when
 *            (float)count < (float)((double)(float)max_count * 0.8) -- and, when min_score is not NULL (loop mode), minScoreFilter --
 *            dropped when score < *min_score.  Survivors in ascending id order: id, count, score = DBoW's L1 score of (query, keyframe),
 *            bit-equal to DBoW3::Vocabulary::l1Score(query, keyframe) (sequential sum in ascending word order).  *n_out is the number
 *            of survivors even when it exceeds cap (ORBFE_ECAPACITY, and then nothing is written).  One upload and one download on
 *            the context's stream.  Ignored ids that are not in the database are skipped.
 *   score    the L1 score of the query against each chosen keyframe (bad or not); an id not in the database: ORBFE_EBADARG.
 * The group filter (groupFilter, src/KeyFrameDB.cc:125-174) is host code over the survivors and each one's ordered covisible list (the
 * caller's KeyFrame::getOrderedConnectedKfs(10) without null / bad entries): a group starts at survivor i with acc = 0 + score[i] and
 * best = i; each covisible id that is a survivor (others are skipped) adds its score, a strictly greater score makes it the best;
 * th2 = (max over groups of acc, floor 0) * 0.75; out = the best ids of the groups with acc > th2, ascending and unique
 * (out has room for n).  No device, no context.                                                                                      */
typedef struct orbfe_kfdb orbfe_kfdb;
typedef struct orbfe_kfdb_query_in {
  const uint32_t* words;      /* [n_words] strictly ascending                        */
  const double* values;       /* [n_words]                                           */
  int32_t n_words;            /* 0 .. ORBFE_BOW_MAX_FEATURES                         */
  const uint64_t* ignore;     /* [n_ignore] ids left out of the count (any order)    */
  int32_t n_ignore;
  const double* min_score;    /* NULL: relocalisation; else loop mode with this floor */
} orbfe_kfdb_query_in;
orbfe_status orbfe_kfdb_create(int32_t device_id, int32_t n_words, orbfe_kfdb** out);
void orbfe_kfdb_destroy(orbfe_kfdb* db);  /* no call on the database may still run */
orbfe_status orbfe_kfdb_add(orbfe_kfdb* db, int32_t n_kf, const uint64_t* ids, const int64_t* offsets, const uint32_t* words,
                            const double* values);
orbfe_status orbfe_kfdb_set_bad(orbfe_kfdb* db, int32_t n, const uint64_t* ids, const uint8_t* flags);
orbfe_status orbfe_kfdb_erase(orbfe_kfdb* db, int32_t n, const uint64_t* ids);
orbfe_status orbfe_kfdb_size(orbfe_kfdb* db, int64_t* out);
orbfe_status orbfe_kfdb_query(orbfe_ctx* ctx, orbfe_kfdb* db, const orbfe_kfdb_query_in* q, uint64_t* out_ids, int32_t* out_counts,
                              double* out_scores, int64_t cap, int64_t* n_out);
orbfe_status orbfe_kfdb_score(orbfe_ctx* ctx, orbfe_kfdb* db, const orbfe_kfdb_query_in* q, const uint64_t* ids, int32_t n, double* scores);
orbfe_status orbfe_kfdb_group_filter(int64_t n, const uint64_t* ids, const double* scores, const int64_t* conn_offsets, const uint64_t* conn_ids,
                                     uint64_t* out, int64_t* n_out);

/* ---- EPnP RANSAC (PnPSolver + Ransac<PnPRet>, src/PnPSolver.cc, include/ORB_SLAM2/Ransac.hpp) --------------------------------------
 * One orbfe_pnp set holds the PnP problems of a relocalisation -- one per candidate keyframe, in the order Tracking creates its
 * solvers -- on ONE device: problem i has the points [offsets[i], offsets[i + 1]) of xyz (map points, world frame), uv (keypoints)
 * and octave (0 .. n_levels - 1, the threshold (float)(5.991 * level_sigma2[octave])), 0 .. ORBFE_PNP_MAX_POINTS of them.  params
 * NULL: setRansacParams() (min set 4, at most 100 iterations, ratio 0.4, probability 0.99); min_set must be 4.  One upload.
 *   iterate  Ransac::iterate(n_iterations, modelRet, bNoMore, vnInlierIndices) of one problem, exactly: pose
 *            (Rcw row-major, then tcw) and has_pose (0: the empty cv::Mats) are in / out, as are inliers[0 .. *n_inliers) (problem-local
 *            indices, the list is appended to, duplicates included); *no_more is only ever set to 1; *ret the return value.  cap: room in
 *            inliers; a longer result is ORBFE_ECAPACITY with *n_inliers the size needed and nothing changed.  An iterate call that is
 *            not the predicted one (another problem or n, a non-empty entry pose or list, an engine moved since) starts a new
 *            speculation: the schedule Tracking runs -- round-robin over the live problems, ascending, n_iterations each, no refine
 *            success -- in one upload, two launches and one download, replayed call by call from then on.  Speculation only changes
 *            the speed, never a result.
 *   engine   the process-wide sampling engine (Ransac<PnPRet>'s static std::default_random_engine, default seed: state 1): get and / or
 *            set its state (1 .. 2^31 - 2).  One lock serialises the engine and every set's iterate.
 *   stats    launch sequences and hypotheses evaluated on the device so far.
 * Errors: ORBFE_EBADARG (NULL pointers, problem out of range, octave out of range, min_set != 4, inlier index out of range, engine
 * state out of range), ORBFE_EDEVICE (no device, HIP failure), ORBFE_ENOMEM, ORBFE_ECAPACITY (inliers too small).                     */
#define ORBFE_PNP_MAX_POINTS 65536
typedef struct orbfe_pnp orbfe_pnp;
typedef struct orbfe_pnp_params {
  int32_t min_set;        /* mnMinSet (4)          */
  int32_t max_iterations; /* nMaxIterations (100)  */
  float ratio;            /* fRatio (0.4)          */
  float prob;             /* fProb (0.99)          */
} orbfe_pnp_params;
orbfe_status orbfe_pnp_create(int32_t device_id, int32_t n_problems, const int64_t* offsets /*[n_problems + 1]*/, const float* xyz /*[N][3]*/,
                              const float* uv /*[N][2]*/, const int32_t* octave /*[N]*/, const float* level_sigma2, int32_t n_levels,
                              const orbfe_camera* cam /* fx fy cx cy */, const orbfe_pnp_params* params, orbfe_pnp** out);
void orbfe_pnp_destroy(orbfe_pnp* set);  /* no call on the set may still run */
orbfe_status orbfe_pnp_iterate(orbfe_pnp* set, int32_t problem, int32_t n_iterations, float* pose /*[12] in/out*/, int32_t* has_pose,
                               int32_t* inliers, int64_t* n_inliers, int64_t cap, int32_t* ret, int32_t* no_more);
orbfe_status orbfe_pnp_engine(uint32_t* get, const uint32_t* set);
orbfe_status orbfe_pnp_stats(orbfe_pnp* set, int64_t* launches, int64_t* hypotheses);

/* ---- Sim3 RANSAC (Sim3Solver + Ransac<Sim3Ret>, src/Sim3Solver.cc, include/ORB_SLAM2/Sim3Solver.h, Ransac.hpp) ---------------------
 * One orbfe_sim3 set holds the Sim3 problems of one LoopClosing::computeSim3 call (src/LoopClosing.cc:300-415) -- one per loop
 * candidate, in the order its first loop creates the solvers -- on ONE device: problem i has the correspondences
 * [offsets[i], offsets[i + 1]) (0 .. ORBFE_BOW_MAX_FEATURES of them) of pos_p / pos_q (the world positions of the two map points),
 * octave_p / octave_q (the two keypoints' octaves, 0 .. n_levels - 1, the thresholds (float)(9.210 * level_sigma2[octave])) and the
 * keyframe poses pose_p[i] / pose_q[i] (Rpw row-major, then tpw; likewise q).  create is Sim3Solver's constructor
 * (Sim3Solver.cc:162-206) after its vbChoose filter, which stays with the caller (:173-182): p3d = Rpw * pos + tpw, Camera::project,
 * setRansacParams.  params NULL: max 100 iterations, ratio 0.4, probability 0.99; min_set must be 3 and the scale is fixed, as
 * Sim3Solver::create forces both (Sim3Solver.h:71-76, S1).  One upload.
 *   iterate  Ransac::iterate(n_iterations, modelRet, bNoMore, vnInlierIndices) (Ransac.hpp:63-103) of one problem, exactly (DESIGN 4.21,
 *            S1-S7) over Sim3Solver::modelFunc (:24-148, Horn) and checkInliers / computeError (:215-259): model (Rqp row-major, then
 *            tqp; mfS is 1) and has_model (0: the empty cv::Mats) are in / out, as are inliers[0 .. *n_inliers) (problem-local
 *            indices); both end as the reference leaves them -- untouched when no hypothesis ran.  *no_more is only ever set to 1;
 *            *ret the return value.  cap: room in inliers; a longer result is ORBFE_ECAPACITY with *n_inliers the size needed and
 *            nothing changed.  A call that is not the predicted one (another problem or n, an engine moved since) starts a new
 *            speculation: the schedule computeSim3 runs -- round-robin over the live problems, ascending, n_iterations each, no
 *            refine success -- in one upload, ONE launch and one download, replayed call by call from then on.  A problem the caller
 *            leaves out where the schedule had it (a candidate computeSim3 discards after making its solver) is left out of later
 *            schedules until it is called.  Speculation only changes the speed, never a result.
 *   engine   Ransac<Sim3Ret>'s own static std::default_random_engine (default seed: state 1), apart from orbfe_pnp_engine's: get and
 *            / or set its state (1 .. 2^31 - 2).  One lock serialises this engine and every Sim3 set's iterate.
 *   stats    launch sequences and hypotheses evaluated on the device so far.
 *   profile  enable > 0 puts two events around every launch from then on, 0 stops that, < 0 leaves it; device_us (NULL: not wanted) is
 *            the time between those events so far, bytes_uploaded (NULL: not wanted) what create and every speculation sent up.
 * Errors: ORBFE_EBADARG (NULL pointers, problem out of range, octave out of range, min_set != 3, engine state out of range),
 * ORBFE_EDEVICE (no device, HIP failure), ORBFE_ENOMEM, ORBFE_ECAPACITY (inliers too small).                                          */
typedef struct orbfe_sim3 orbfe_sim3;
typedef struct orbfe_sim3_params {
  int32_t min_set;        /* mnMinSet (3)          */
  int32_t max_iterations; /* nMaxIterations (100)  */
  float ratio;            /* fRatio (0.4)          */
  float prob;             /* fProb (0.99)          */
} orbfe_sim3_params;
orbfe_status orbfe_sim3_create(int32_t device_id, int32_t n_problems, const int64_t* offsets /*[n_problems + 1]*/, const float* pos_p /*[N][3]*/,
                               const float* pos_q /*[N][3]*/, const int32_t* octave_p /*[N]*/, const int32_t* octave_q /*[N]*/,
                               const float* pose_p /*[n_problems][12]*/, const float* pose_q /*[n_problems][12]*/, const float* level_sigma2,
                               int32_t n_levels, const orbfe_camera* cam /* fx fy cx cy */, const orbfe_sim3_params* params, orbfe_sim3** out);
void orbfe_sim3_destroy(orbfe_sim3* set);  /* no call on the set may still run */
orbfe_status orbfe_sim3_iterate(orbfe_sim3* set, int32_t problem, int32_t n_iterations, float* model /*[12] in/out*/, int32_t* has_model,
                                int32_t* inliers, int64_t* n_inliers, int64_t cap, int32_t* ret, int32_t* no_more);
orbfe_status orbfe_sim3_engine(uint32_t* get, const uint32_t* set);
orbfe_status orbfe_sim3_stats(orbfe_sim3* set, int64_t* launches, int64_t* hypotheses);
orbfe_status orbfe_sim3_profile(orbfe_sim3* set, int32_t enable, double* device_us, int64_t* bytes_uploaded);

/* ---- Sim3 optimisation (Optimizer::OptimizeSim3, src/Optimizer.cc:464-619) -----------------------------------------------------------
 * The last step of LoopClosing::computeSim3 (src/LoopClosing.cc:300-415) for one candidate, from the point where the graph is built
 * (:509-553): pair i is one match that passed the vbIsInlier filter of :492-508, which stays with the caller as map state does
 * everywhere -- pc[i] = cPc = Rcw * cPw + tcw and pm[i] = mPc (float, :511-512), uv_c[i] / uv_m[i] the two key points (:535, :545),
 * info_c[i] = pCurr->getScaledFactorInv2(ckp.octave) and info_m[i] = pCurr->getScaledFactorInv2(mkp.octave) (:536, :546: pCurr for
 * both).  One VertexSim3Expmap with the scale FIXED (the reference's only caller passes bFixedScale = true; there is no free-scale
 * mode), an EdgeSim3ProjectXYZ and an EdgeInverseSim3ProjectXYZ per pair with Huber sqrt(9.210), both cameras (fx, fy, cx, cy);
 * optimize(5), pairs with a chi2 > 9.210 dropped, optimize(nBad ? 10 : 5), pairs with both chi2 <= 9.210 are the inliers (:565-607).
 * g2o differentiates these edges numerically and so does the device.
 *   model       in / out, orbfe_sim3_iterate's layout (Rqp row-major, then tqp; mfS is 1): ConvertSim3G2o on entry, ConvertG2o2Sim3 on
 *               return (:474, :617).
 *   inlier_out  [n]: 1 for the pairs that stay in the match list, in order (:608-616).
 *   n_inliers   the return value.  0 with fewer than 20 pairs left after the first round (:584): model is untouched and inlier_out all
 *               1, as the reference returns before it swaps the list.  n < 20 gets there without a launch.
 *   est_out     NULL or [8]: the final estimate in double (qx qy qz qw tx ty tz s), the start estimate on the early return.
 * One upload, ONE launch, one download; 0 <= n <= ORBFE_BOW_MAX_FEATURES.  Errors: ORBFE_EBADARG (NULL context or model, n out of
 * range, NULL arrays with n > 0, a model entry that is not finite: nothing is launched), ORBFE_EDEVICE.                              */
orbfe_status orbfe_sim3_optimize(orbfe_ctx* ctx, int32_t n, const float* pc /*[n][3] cPc*/, const float* pm /*[n][3] mPc*/,
                                 const float* uv_c /*[n][2]*/, const float* uv_m /*[n][2]*/, const double* info_c /*[n]*/,
                                 const double* info_m /*[n]*/, float fx, float fy, float cx, float cy,
                                 float* model /*[12] in/out: R row-major, t -- orbfe_sim3_iterate's layout*/,
                                 uint8_t* inlier_out /*[n]*/, int32_t* n_inliers, double* est_out /*[8] qx qy qz qw tx ty tz s, nullable*/);

/* ---- pose graph over the essential graph (Optimizer::optimizeEssentialGraph, src/Optimizer.cc:746-920) -----------------------------
 * The step LoopClosing::correctLoop (src/LoopClosing.cc:432-541) ends in, from the point where the graph is built (:767-877): vertex v
 * is one good keyframe with its VertexSim3Expmap estimate (the corrected Sim3 of the loop group, ConvertSim3G2o of the pose otherwise),
 * fixed where it is the loop keyframe; edge e is one EdgeSim3 (:804-877: loop connections, spanning tree, loop edges, covisibility)
 * from vertex edge_v0[e] to vertex edge_v1[e] with the measurement meas[e] = S_v1w * S_wv0 and the identity as information.  The scale
 * is FIXED: the reference's only caller passes bFixedScale = true and every Sim3 it passes has scale 1; there is no free-scale mode and
 * an s other than 1 is refused.  err = log(meas * S_v0 * S_v1^-1); g2o differentiates this edge numerically for both vertices and so
 * does the device; Levenberg-Marquardt as optimizer.optimize(iterations) runs it (the reference: 20), lambda_0 = 1e-5 max |diag|, at
 * most 10 trials per iteration.  Several edges may join one pair of vertices, in either orientation; a vertex
 * without an edge keeps its bytes.
 *   estimates_out  [n_vertices][8]: every estimate after the last accepted trial (fixed ones unchanged).
 *   chi2_out       NULL or [n_edges]: err . err of every edge at estimates_out.
 *   stats          NULL or [2]: iterations run, trials run.
 * One upload, a host-driven loop of a few scalars per trial, one download.  The system of the nf non-fixed vertices is dense, 6 nf
 * square in double: nf <= ORBFE_PG_MAX_FREE (288 nf^2 bytes: 302 MB at the bound, what the panel solver of the local bundle adjustment
 * factorises in place).  ORBFE_PG_MAX_FREE is this dense solver's bound; orbfe_pose_graph_optimize_ex below has a sparse solver without one.
 * ORBFE_OK with nothing launched and the estimates copied through (chi2_out is not written): n_edges == 0, iterations == 0, every
 * vertex fixed.  Errors, with nothing written: ORBFE_EBADARG (a NULL context, graph or estimates_out; a negative count or iterations
 * < 0; a NULL array with a non-zero count; an edge index out of range; edge_v0[e] == edge_v1[e]; an entry that is not finite; an s
 * other than 1 on a vertex or a measurement), ORBFE_EBADSIZE (more than ORBFE_PG_MAX_FREE non-fixed vertices), ORBFE_EDEVICE.        */
#define ORBFE_PG_MAX_FREE 1024
typedef struct orbfe_pose_graph {
  int32_t n_vertices, n_edges;
  const double* estimates;   /* [n_vertices][8] qx qy qz qw tx ty tz s (s must be 1) */
  const uint8_t* fixed;      /* [n_vertices] */
  const int32_t* edge_v0;    /* [n_edges] vertex 0 (pkf1) */
  const int32_t* edge_v1;    /* [n_edges] vertex 1 (pkf2) */
  const double* meas;        /* [n_edges][8] */
} orbfe_pose_graph;
orbfe_status orbfe_pose_graph_optimize(orbfe_ctx* ctx, const orbfe_pose_graph* graph, int32_t iterations,
                                       double* estimates_out /*[n_vertices][8]*/, double* chi2_out /*[n_edges], nullable*/,
                                       int32_t* stats /*[2] iterations run, trials run; nullable*/);
/* The same optimisation with a choice of linear solver; ORBFE_PG_MAX_FREE is the DENSE solver's bound only.
 *   solver 1  orbfe_pose_graph_optimize, byte for byte (and its ORBFE_EBADSIZE past ORBFE_PG_MAX_FREE non-fixed vertices).
 *   solver 2  a block-sparse Cholesky over the graph's own structure: the non-fixed vertices in vertex order, no
 *             reordering -- keyframe ids are nearly a time order, so spanning tree and covisibility links make a band and a loop
 *             connection one long row.  A host symbolic phase (elimination tree, the factor's columns) per call, then per trial one
 *             assembly into the factor's storage and ONE single-workgroup kernel that factorises and substitutes.  No bound on the
 *             vertices but memory (288 bytes per block of the factor; ORBFE_ENOMEM).  Same Levenberg-Marquardt loop and kernels otherwise;
 *             the estimates agree with solver 1 to the factorisations' rounding (3e-15 after one iteration at 257 vertices), not bit for
 *             bit.  Every sum has a fixed order: a repeated call is bit-identical.
 *   solver 0  (and opt == NULL) sparse past ORBFE_PG_MAX_FREE non-fixed vertices; below it from ORBFE_PG_SPARSE_MIN_FREE on, unless the
 *             factor is dense-ish: more than ORBFE_PG_SPARSE_MAX_COL_BLOCKS blocks per column on average (l_blocks > that x nf); dense
 *             otherwise.  Both numbers are measured crossovers: 24 non-fixed vertices is the smallest measured size at
 *             which the sparse solver wins; a factor of 20 blocks a column is the densest measured at which it wins at 100, 500 and
 *             1000 keyframes alike (an essential graph has 7 to 9).
 *   stats     NULL or [4]: iterations run, trials run, the solver used (1 or 2; the value asked for where nothing was launched), the
 *             blocks of the factor with the diagonal ones (0 for solver 1).
 * Everything else -- arguments, early returns, errors -- as orbfe_pose_graph_optimize; a solver outside 0 .. 2 is ORBFE_EBADARG.        */
#define ORBFE_PG_SPARSE_MIN_FREE 24
#define ORBFE_PG_SPARSE_MAX_COL_BLOCKS 20
typedef struct orbfe_pose_graph_options {
  int32_t solver;            /* 0 auto, 1 dense (orbfe_pose_graph_optimize), 2 block-sparse Cholesky */
} orbfe_pose_graph_options;
orbfe_status orbfe_pose_graph_optimize_ex(orbfe_ctx* ctx, const orbfe_pose_graph* graph, int32_t iterations,
                                          const orbfe_pose_graph_options* opt /*nullable*/, double* estimates_out /*[n_vertices][8]*/,
                                          double* chi2_out /*[n_edges], nullable*/, int32_t* stats /*[4], nullable*/);

/* ---- new map points of a keyframe (LocalMapping::createNewMapPoints, src/LocalMapping.cc:165-285) ---------------------------------
 * One call runs loop 1 and loop 2 of createNewMapPoints for the current keyframe `cur` against the neighbours nbs[0 .. n_nb) IN THE
 * GIVEN ORDER (the reference's std::map order, T2): searchForTriangulation (searchByBow with bAddMPs, ratio 0.6, threshold 50, no
 * verifyAngle; the mutual epipolar test), the parallax cosines, the three-way branch, triangulate, unProject and checkMapPoint, then
 * the first-wins resolution and the tail list (quirks T1-T9 and the SVD decision: DESIGN 4.17).  A neighbour closer than `bl` to the
 * current keyframe ((float)|Ow_cur - Ow_nb| < bl) is skipped (T7).  One upload, a fixed launch sequence, one download.
 * Outputs: records[0 .. *n_records) in processing order -- the one accepted candidate of each current feature that got a point --
 * and tail[0 .. *n_tail): the current features, ascending, whose unprocessed point was not consumed and whose slot (flag GOOD of cur)
 * is empty after loop 2.  Both counts are set even when they exceed their capacity (ORBFE_ECAPACITY, nothing written).
 * consumed (NULL: not wanted) [cur->n]: 1 where an own-stereo candidate took the feature's unprocessed point, accepted or not (T5) --
 * the entries loop 2 erases from mmUnprocessMps.
 * Errors: ORBFE_EBADARG (NULL pointers, n_nb outside 0 .. ORBFE_TRI_MAX_NB, n outside 0 .. ORBFE_BOW_MAX_FEATURES, FeatureVector nodes
 * not strictly ascending, offsets not starting at 0 / decreasing / past the feature count, feature indices out of range, an octave
 * outside 0 .. n_levels - 1), ORBFE_EDEVICE, ORBFE_ENOMEM, ORBFE_ECAPACITY.                                                            */
#define ORBFE_TRI_MAX_NB 64
#define ORBFE_TRI_GOOD 1  /* flags: the feature's map point is non-null and not bad */
#define ORBFE_TRI_INMAP 2 /*        ... and isInMap()                              */
#define ORBFE_TRI_TRIANGULATED 1 /* record kinds: triangulate (LocalMapping.cc:224-230)                                 */
#define ORBFE_TRI_OWN_STEREO 2   /* the current feature's unprocessed point (:232-239)                                   */
#define ORBFE_TRI_NB_STEREO 3    /* the neighbour's unprojection (:240-247)                                             */
typedef struct orbfe_tri_kf {
  int32_t n;                     /* features                                                                   */
  const orbfe_keypoint* kps;     /* [n] mvFeatsLeft                                                            */
  const uint8_t* desc;           /* [n][32]                                                                    */
  int32_t n_nodes;               /* FeatureVector in orbfe_bow_out's layout                                    */
  const uint32_t* nodes;         /* [n_nodes] strictly ascending                                               */
  const int32_t* node_offsets;   /* [n_nodes + 1]                                                              */
  const uint32_t* features;      /* [node_offsets[n_nodes]]                                                    */
  const uint8_t* flags;          /* [n] ORBFE_TRI_GOOD | ORBFE_TRI_INMAP                                       */
  const double* depth;           /* [n] mvDepths (> 0: stereo)                                                 */
  const double* right_u;         /* [n] mvRightU                                                               */
  float Tcw[16];                 /* the pose as the keyframe stores it, row-major                              */
  float Twc[16];                 /* its stored inverse (not recomputed)                                        */
  float Ow[3];                   /* getFrameCenter()                                                           */
  const uint8_t* unproc;         /* cur only: [n] the feature has an entry in mmUnprocessMps (else NULL)       */
  const float* unproc_pos;       /* cur only: [n][3] that point's world position                               */
} orbfe_tri_kf;
typedef struct orbfe_tri_record {
  int32_t nb;                    /* neighbour index                                                            */
  int32_t query, train;          /* feature of cur, feature of the neighbour                                   */
  int32_t kind;                  /* ORBFE_TRI_*                                                                */
  float xyz[3];                  /* world position of the point                                                */
} orbfe_tri_record;
orbfe_status orbfe_create_new_map_points(orbfe_ctx* ctx, const orbfe_tri_kf* cur, int32_t n_nb, const orbfe_tri_kf* nbs,
                                         const orbfe_camera* cam /* fx fy cx cy */, const float* k_inv /*[9] Camera::mKInv*/, float bl,
                                         const float* scale_factors, int32_t n_levels, orbfe_tri_record* records, int64_t cap,
                                         int64_t* n_records, int32_t* tail, int64_t tail_cap, int64_t* n_tail, uint8_t* consumed);

/* ---- the inverse fuses of a new keyframe (LocalMapping::fuseMapPoints, src/LocalMapping.cc:352-405) ------------------------------
 * After its forward fuse, fuseMapPoints runs ORBMatcher::fuse(pkf, cur, map) (src/ORBMatcher.cc:716-724) once per target keyframe:
 * searchByProjection(pkf, cur, matches, 3.0f, true) (:265-347) + processFuseMps (:623-663).  With bFuse that search projects nothing:
 * feature i of `cur` searches target k around ITS OWN position with ITS OWN descriptor, so the search result of (k, i) depends on
 * keyframe data alone and only MapPoint::isInVision(target k) depends on the map state.  One call computes, for every target k and
 * every feature i of `cur`:
 *   best_idx[k][i]   the feature of target k that findFeaturesInArea(cur.kps[i], th, lo, hi) (src/Frame.cc:286-311, radius
 *                    th * sf[octave]^2, cells clamped as orbfe_search_in_area) + getBestMatch(cur.desc[i], ..) select, if the list is
 *                    not empty, (float)best / (float)second < ratio and best < dist_threshold (:339); -1 otherwise.  The octave window
 *                    follows z[k] (tlc.z of :274-276, computed by the caller) against bl: z > bl: [octave, 7], z < -bl: [0, octave],
 *                    else [octave - 1, octave + 1] clipped to 0 .. 7 (the reference hard-codes 7).  Computed for EVERY (k, i), with or
 *                    without a point in the slot: a slot that is empty now can gain a point before its keyframe's turn.
 *   best_dist[k][i]  the distance of that match (0 where best_idx is -1)
 *   visible[k][i]    MapPoint::isInVision(target k) (src/MapPoint.cc:141-171) of the point in slot i, in the float / double mix of
 *                    orbfe_project_map_points; 0 where has_point[i] is 0
 * The caller replays the reference's sequential loop over the targets with these tables (which entries stay valid while
 * MapPoint::replace changes the map).  One upload, three launches, one download.  n_kf == 0 or cur->n == 0: ORBFE_OK, nothing written.
 * Errors: ORBFE_EBADARG (NULL pointers, n_kf outside 0 .. ORBFE_FUSE_MAX_KF, n outside 0 .. ORBFE_BOW_MAX_FEATURES, an octave outside
 * 0 .. n_levels - 1, bad bounds), ORBFE_EBADSIZE (a target's grid exceeds the LDS counters), ORBFE_EDEVICE, ORBFE_ENOMEM.              */
#define ORBFE_FUSE_MAX_KF 64
typedef struct orbfe_fuse_kf {
  int32_t n;                  /* features, 0 .. ORBFE_BOW_MAX_FEATURES                                       */
  const orbfe_keypoint* kps;  /* [n] mvFeatsLeft                                                             */
  const uint8_t* desc;        /* [n][32]                                                                     */
  float Rcw[9], tcw[3];       /* getPose(Rcw, tcw), row-major                                                */
  float bounds[4];            /* mfMinU mfMaxU mfMinV mfMaxV (grid + clipping, as orbfe_search_in_area_features_ex) */
} orbfe_fuse_kf;
typedef struct orbfe_fuse_points { /* one row per feature of `cur` */
  const uint8_t* has_point;   /* [n] the slot holds a non-null, not-bad map point                             */
  const float* pos;           /* [n][3] */
  const float* view_dir;      /* [n][3] */
  const float* max_dist;      /* [n]    */
  const float* min_dist;      /* [n]    */
} orbfe_fuse_points;
orbfe_status orbfe_fuse_into_keyframes(orbfe_ctx* ctx, const orbfe_fuse_kf* cur, const orbfe_fuse_points* pts, int32_t n_kf,
                                       const orbfe_fuse_kf* targets, const float* z /*[n_kf]*/, const orbfe_camera* cam /* fx fy cx cy */,
                                       float bl, const float* scale_factors, int32_t n_levels, float th, float ratio,
                                       int32_t dist_threshold, int32_t* best_idx /*[n_kf][cur->n]*/, int32_t* best_dist /*[n_kf][cur->n]*/,
                                       uint8_t* visible /*[n_kf][cur->n]*/);

/* ---- keyframes resident on the device -------------------------------------------------------------------------------
 * One orbfe_kfstore holds, on ONE device and keyed by a uint64 id (KeyFrame::getID()), what never changes after a keyframe's creation:
 * its n features (keypoints, descriptors, depth and right_u, -1 where there is none), its frame bounds, the area grid built from them
 * (cell_off[rows * cols + 1], cell_feat[n]: VirtualFrame::initGrid, what orbfe_fuse_into_keyframes builds per call) and, once set_bow
 * has run, its FeatureVector in orbfe_bow_out's layout.  Poses and map points are NOT stored: they change during mapping and stay
 * arguments of the calls below.  The store has its own lock and serves every context on its device; a context on another device:
 * ORBFE_EBADARG.  add, add_from_slot, set_bow and erase take the lock exclusively; fetch, info, size and the two *_stored calls take
 * it shared for their whole (synchronous) duration, so an erase never frees memory under a running kernel.  An entry never moves:
 * memory comes in slabs of slab_bytes (0: 32 MB), an entry larger than a slab gets an allocation of its own, erased space is reused.
 *   create         width, height: the image size a NULL `bounds` stands for (a context's config); n_levels: octaves are 0 .. n_levels - 1
 *   add            from host arrays (loaded maps, tests).  depth / right_u NULL: every entry -1.  bounds NULL: {0, width, 0, height}.
 *                  Errors: an id already present, an octave out of range, bad bounds: ORBFE_EBADARG, nothing changes; a grid that
 *                  exceeds the LDS counters: ORBFE_EBADSIZE (the rule of orbfe_fuse_into_keyframes).
 *   add_from_slot  the features of extraction slot `slot` of `ctx` (and, pair >= 0, that stereo pair's right_u and depth; pair < 0:
 *                  -1) device to device, ordered after the slot's pending work as orbfe_fetch_features is.  Only the feature count
 *                  comes to the host (4 bytes, so that the entry is exactly as large as it must be); ONE launch then packs the
 *                  slot's arrays into the entry and builds its grid.  *n_out (NULL: not wanted): the count.  The context's n_levels
 *                  must not exceed the store's.
 *   set_bow        the FeatureVector of a present keyframe (replacing an earlier one), checked as orbfe_create_new_map_points checks
 *                  an orbfe_tri_kf: nodes strictly ascending, offsets from 0, not decreasing, not past n, feature indices below n.
 *   erase          unknown ids are ignored.
 *   info / fetch   an unknown id: ORBFE_EBADARG.  fetch copies the arrays whose pointer is not NULL, sized as info says.  has_stereo says
 *                  whether depth and right_u were supplied at insertion (add with both arrays, add_from_slot with pair >= 0).
 * orbfe_fuse_into_keyframes_stored and orbfe_create_new_map_points_stored are orbfe_fuse_into_keyframes and
 * orbfe_create_new_map_points with the keyframes named by id: identical outputs, rules and errors, the same kernels; only the map
 * state goes up.  n_cur / orbfe_tri_state::n must equal the stored feature count (they size the caller's arrays).  cur_id may be among
 * the fuse targets.  An unknown id, a keyframe without FeatureVector (create_new_map_points_stored), n_levels below the store's:
 * ORBFE_EBADARG, nothing written.                                                                                                    */
typedef struct orbfe_kfstore orbfe_kfstore;
typedef struct orbfe_kfstore_info {
  int32_t n;                  /* features                                                                     */
  int32_t has_bow;            /* set_bow has run                                                              */
  int32_t has_stereo;         /* depth and right_u were supplied (add with both arrays, add_from_slot with a pair) */
  int32_t n_nodes, n_bow_features; /* sizes of the FeatureVector arrays (0 without one)                       */
  int32_t grid_rows, grid_cols;    /* cell_off has grid_rows * grid_cols + 1 entries, cell_feat n             */
  float bounds[4];            /* mfMinU mfMaxU mfMinV mfMaxV                                                  */
  int64_t bytes;              /* device bytes the entry occupies                                              */
} orbfe_kfstore_info;
typedef struct orbfe_fuse_pose {
  float Rcw[9], tcw[3];       /* getPose(Rcw, tcw), row-major                                                 */
} orbfe_fuse_pose;
typedef struct orbfe_tri_state { /* the map state of one stored keyframe */
  int32_t n;                     /* its feature count (must equal the stored one)                             */
  const uint8_t* flags;          /* [n] ORBFE_TRI_GOOD | ORBFE_TRI_INMAP                                      */
  float Tcw[16], Twc[16], Ow[3]; /* as orbfe_tri_kf                                                           */
  const uint8_t* unproc;         /* cur only: [n]                                                             */
  const float* unproc_pos;       /* cur only: [n][3]                                                          */
} orbfe_tri_state;
orbfe_status orbfe_kfstore_create(int32_t device_id, int32_t width, int32_t height, int32_t n_levels, int64_t slab_bytes, orbfe_kfstore** out);
void orbfe_kfstore_destroy(orbfe_kfstore* store);  /* no call on the store may still run */
orbfe_status orbfe_kfstore_add(orbfe_kfstore* store, uint64_t id, int32_t n, const orbfe_keypoint* kps, const uint8_t* desc, const double* depth,
                               const double* right_u, const float* bounds /*[4] or NULL*/);
orbfe_status orbfe_kfstore_add_from_slot(orbfe_ctx* ctx, orbfe_kfstore* store, uint64_t id, int32_t slot, int32_t pair,
                                         const float* bounds /*[4] or NULL*/, int32_t* n_out);
orbfe_status orbfe_kfstore_set_bow(orbfe_kfstore* store, uint64_t id, int32_t n_nodes, const uint32_t* nodes, const int32_t* node_offsets,
                                   const uint32_t* features);
orbfe_status orbfe_kfstore_erase(orbfe_kfstore* store, int32_t n, const uint64_t* ids);
orbfe_status orbfe_kfstore_size(orbfe_kfstore* store, int64_t* n_keyframes, int64_t* bytes_used, int64_t* bytes_reserved);
orbfe_status orbfe_kfstore_info_get(orbfe_kfstore* store, uint64_t id, orbfe_kfstore_info* out);
orbfe_status orbfe_kfstore_fetch(orbfe_kfstore* store, uint64_t id, orbfe_keypoint* kps, uint8_t* desc, double* depth, double* right_u,
                                 int32_t* cell_off, int32_t* cell_feat, uint32_t* nodes, int32_t* node_offsets, uint32_t* features);
orbfe_status orbfe_fuse_into_keyframes_stored(orbfe_ctx* ctx, orbfe_kfstore* store, uint64_t cur_id, int32_t n_cur, const orbfe_fuse_points* pts,
                                              int32_t n_kf, const uint64_t* target_ids, const orbfe_fuse_pose* poses /*[n_kf]*/,
                                              const float* z /*[n_kf]*/, const orbfe_camera* cam, float bl, const float* scale_factors,
                                              int32_t n_levels, float th, float ratio, int32_t dist_threshold, int32_t* best_idx,
                                              int32_t* best_dist, uint8_t* visible);
orbfe_status orbfe_create_new_map_points_stored(orbfe_ctx* ctx, orbfe_kfstore* store, uint64_t cur_id, const orbfe_tri_state* cur, int32_t n_nb,
                                                const uint64_t* nb_ids, const orbfe_tri_state* nbs, const orbfe_camera* cam, const float* k_inv,
                                                float bl, const float* scale_factors, int32_t n_levels, orbfe_tri_record* records, int64_t cap,
                                                int64_t* n_records, int32_t* tail, int64_t tail_cap, int64_t* n_tail, uint8_t* consumed);

/* ---- searchByBow over stored keyframes --------------------------------------------------------------------------------
 * ORBMatcher::searchByBow(pFrame, pKframe, matches, bAddMPs, bLoop) (src/ORBMatcher.cc:170-253) with verifyAngle (:1013-1051) of ONE
 * query frame against n_kf keyframes of a store in one call: what Tracking::filterKFByBow (src/Tracking.cc:446-490) runs once per
 * relocalisation candidate and LoopClosing::computeSim3 (src/LoopClosing.cc:308-326) once per loop candidate.  The candidates are named
 * by id and read where the store keeps them (features, angles, FeatureVector); the query is a stored keyframe too (from_store) or host
 * arrays (a Frame).  Map state is an argument: one flag byte per feature on either side.
 * For every candidate k, matches[match_offsets[k] .. match_offsets[k + 1]) is exactly the std::vector<cv::DMatch> the reference leaves,
 * element for element and in its order:
 *   walk        common nodes ascending; inside a node the keyframe's features in FeatureVector order
 *   filter      by mode (ORBFE_BOW_*), on the keyframe feature and on the node's query features; an empty candidate list: no match
 *   best match  getBestMatch (:967-990): first minimum (strict <); the second best is never an earlier record, INT_MAX with one candidate
 *   test        rejected iff best > dist_threshold || (float)best / (float)second > ratio (0 / 0 is accepted)
 *   queryIdx    no uniqueness check: several matches may name one query feature
 *   orientation check_orientation: diff = angle_q - angle_t in float, negative: 360 + diff; bin (int)(diff / 12.f), bin 30 -> 0; three
 *               rounds of "first strictly largest remaining bin" (empty bins never); output: the chosen bins ascending, inside a bin
 *               the order above.  (Angles no extractor gives -- NaN, a difference of 360 and more -- count as bin 0.)
 * Side effects on map points (setMapPoints, addMatchInTrack) stay with the caller.
 * match_offsets [n_kf + 1] is always set in full; a total beyond cap: ORBFE_ECAPACITY, nothing written to matches.  ORBFE_EBADARG, nothing
 * written: an unknown id, a keyframe without FeatureVector, n_kf outside 0 .. ORBFE_BOW_SEARCH_MAX_KF, an unknown mode, a malformed query
 * FeatureVector (orbfe_kfstore_set_bow's checks), n unequal to the stored count.  n_kf == 0: ORBFE_OK.  An id may appear twice, and the
 * query's own id may be among the candidates.  Locks: the context's, then the store's (shared) for the whole synchronous duration.  One
 * upload (records, flags, a host query's arrays), three launches, one download.                                                      */
#define ORBFE_BOW_SEARCH_MAX_KF 64
#define ORBFE_BOW_TRACK 0  /* bAddMPs = false, bLoop = false: keyframe features with a good point, frame features WITHOUT one */
#define ORBFE_BOW_LOOP  1  /* bLoop: no filter on either side                                                                */
#define ORBFE_BOW_ADD   2  /* bAddMPs: on both sides, features whose point is good AND in the map are left out             */
typedef struct orbfe_bow_query {
  int32_t from_store;          /* 1: the stored keyframe `id` (it needs a FeatureVector); desc / angle / the CSR below are ignored */
  uint64_t id;
  int32_t n;                   /* features; from_store: must equal the stored count                                       */
  const uint8_t* desc;         /* [n][32]                                                                                 */
  const float* angle;          /* [n] cv::KeyPoint::angle; may be NULL when check_orientation is 0                        */
  int32_t n_nodes;             /* the FeatureVector in orbfe_bow_out's layout                                             */
  const uint32_t* nodes;
  const int32_t* node_offsets;
  const uint32_t* features;
  const uint8_t* flags;        /* [n] ORBFE_TRI_GOOD | ORBFE_TRI_INMAP; NULL: all 0 (setMapPointsNull())                  */
} orbfe_bow_query;
typedef struct orbfe_bow_match { int32_t query, train, distance; } orbfe_bow_match;   /* cv::DMatch(queryIdx, trainIdx, distance) */
orbfe_status orbfe_search_by_bow_stored(orbfe_ctx* ctx, orbfe_kfstore* store, const orbfe_bow_query* q, int32_t n_kf,
                                        const uint64_t* kf_ids, const uint8_t* const* kf_flags /*[n_kf], each [n_k] or NULL = all 0*/,
                                        int32_t mode, float ratio, int32_t dist_threshold, int32_t check_orientation,
                                        orbfe_bow_match* matches, int64_t cap, int64_t* match_offsets /*[n_kf + 1]*/);

/* ---- searchBySim3 over stored keyframes --------------------------------------------------------------------------------
 * Both overloads of ORBMatcher::searchBySim3 (src/ORBMatcher.cc:370-559), the step of LoopClosing::computeSim3 between the Sim3 RANSAC
 * and OptimizeSim3 and its last step over the loop group's map points.  The keyframes are named by id and read where the store keeps
 * them (features, descriptors, bounds, area grid); only map state goes up: flags, positions, distance ranges, poses, the similarity.
 * model / s: orbfe_sim3_iterate's layout, R row-major then t, p_c = s R p_m + t (the points overload: p_c = s R p_w + t).
 *   arithmetic   a 3x3 row times a vector is the float sum a0 b0 + a1 b1 + a2 b2 left to right; alpha A x + t is
 *                (float)((double)alpha * sum + (double)t); Sim3Ret::inv: s' = 1.f / s, R^T, t' = -s' * (R^T t) in float
 *   project      u = fx * (x / z) + cx, v = fy * (y / z) + cy; rejected: z <= 0, not (u < maxU && v < maxV && u > minU && v > minV),
 *                not (d < max_dist && d > min_dist)
 *   window       octave o = predictLevel(max_dist, d) clamped to [0, min(7, n_levels - 1)]; radius th * sf[o]^2; octaves o - 1 .. o + 1
 *                (not clamped); findFeaturesInArea over the TARGET's grid: rows outer, columns inner, index order inside a cell
 *   best match   getBestMatch (:967-990): first minimum; the second best is never an earlier record, INT_MAX with one candidate
 *   accepted     the list is not empty && best <= dist_threshold && (float)best / (float)second <= ratio (0 / 0 is rejected)
 * orbfe_search_by_sim3_stored (the pair, :424-484), one launch of n_c + n_m waves:
 *   A (:446-461) feature ic of cur named by no input match, GOOD and INMAP: Rcw_C, then Scm.inv(); isInImage on CUR's bounds (the
 *                reference asks the keyframe the point comes from); d = sqrtf(x*x + y*y + z*z) / s'; target match, its features
 *                without GOOD and INMAP left out
 *   B (:463-475) feature im of match named by no input match, GOOD: Rcw_M, then Scm; MATCH's bounds; / s; target cur, same filter
 *   merge        std::map::insert: A's (ic, best), then B's (best, im) in ascending im where the key is absent; new_matches gets the
 *                new pairs in ascending query (distance 0).  A key may repeat the query of an input match (the reference does not check).
 * orbfe_search_by_sim3_points_stored (:501-549), one launch of m waves: point j with usable[j] (the caller clears it for points that
 * are null, bad, not in the map or already in vMatchedMps); isInImage on the keyframe's bounds; dWithS = (float)sqrt of the double sum,
 * d = dWithS / s; view test: rv = R * view_dir in float, rejected iff the double dot rv . p < 0.5 * (double)dWithS; no filter on the
 * keyframe's features.  best_idx[j] = the feature or -1, best_dist[j] its distance (0 with -1); the caller applies
 * vMatchedMps[best_idx[j]] = point j in ascending j (a later point overwrites an earlier one, every accept counts).
 * cur->id == match->id is allowed; n, m or n_matches of 0: ORBFE_OK; m <= 2^20.  More new pairs than cap: ORBFE_ECAPACITY with *n_new set,
 * nothing written.  ORBFE_EBADARG, nothing written: an unknown id, n unequal to the stored count, a match index out of range, s or a model
 * entry not finite or s <= 0, n_levels below the store's, a NULL array with a non-zero count, a context on another device.  Locks: the
 * context's, then the store's (shared) for the whole synchronous duration.  One upload, one launch, one download.                  */
typedef struct orbfe_sim3_side {      /* one keyframe of the pair: its id in the store and its map state                             */
  uint64_t id;
  int32_t n;                          /* must equal the stored count                                                                 */
  const uint8_t* flags;               /* [n] ORBFE_TRI_GOOD | ORBFE_TRI_INMAP of the feature's map point; NULL: all 0                */
  const float* pos;                   /* [n][3] world positions (with flags NULL not read)                                           */
  const float *max_dist, *min_dist;   /* [n] MapPoint::getDistance                                                                   */
  float Rcw[9], tcw[3];
} orbfe_sim3_side;
typedef struct orbfe_sim3_points {    /* vLoopGroupMps as arrays                                                                     */
  int32_t m;
  const uint8_t* usable;              /* [m]                                                                                         */
  const float *pos, *view_dir;        /* [m][3]                                                                                      */
  const float *max_dist, *min_dist;   /* [m]                                                                                         */
  const uint8_t* desc;                /* [m][32] MapPoint::getDesc()                                                                 */
} orbfe_sim3_points;
orbfe_status orbfe_search_by_sim3_stored(orbfe_ctx* ctx, orbfe_kfstore* store, const orbfe_sim3_side* cur, const orbfe_sim3_side* match,
                                         const float* model /*[12]*/, float s, int32_t n_matches,
                                         const orbfe_bow_match* matches /*query in cur, train in match; distance not read*/,
                                         const orbfe_camera* cam, const float* scale_factors, int32_t n_levels, float th, float ratio,
                                         int32_t dist_threshold, orbfe_bow_match* new_matches, int32_t cap, int32_t* n_new);
orbfe_status orbfe_search_by_sim3_points_stored(orbfe_ctx* ctx, orbfe_kfstore* store, uint64_t id, const orbfe_sim3_points* pts,
                                                const float* model /*[12]*/, float s, const orbfe_camera* cam, const float* scale_factors,
                                                int32_t n_levels, float th, float ratio, int32_t dist_threshold, int32_t* best_idx /*[m]*/,
                                                int32_t* best_dist /*[m]*/);

/* ---- the forward fuse over stored keyframes ----------------------------------------------------------------------------
 * ORBMatcher::fuse(pkf, mapPoints, map, bLoop, th) (src/ORBMatcher.cc:682-707) of ONE list of m map points into n_kf keyframes of a
 * store in one call: what LoopClosing::correctLoop (src/LoopClosing.cc:515-517) runs once per neighbour of the current keyframe and
 * LocalMapping::fuseMapPoints (src/LocalMapping.cc:399) once per new keyframe.  The keyframes are named by id and read where the store
 * keeps them (features, descriptors, bounds, area grid); only map state goes up: the poses, the point arrays, the scale factors.
 * best_idx[k][j] is the feature of keyframe k that searchByProjection(pkf_k, {point j}, th, matches, true) (:573-609) puts in its
 * DMatch, or -1; best_dist[k][j] its distance, 0 with -1.
 *   usable       usable[j] == 0: -1.  The caller clears it for null, bad and not-in-map points; the "already held by the keyframe"
 *                filter (:687-701) is live map state and stays with the caller, as does processFuseMps (:623-663)
 *   isInVision   MapPoint::isInVision (src/MapPoint.cc:141-171) on poses[k] and keyframe k's STORED bounds, in
 *                orbfe_project_map_points' arithmetic: rejected in this order: z < 0, not (d < max_dist && d > min_dist), not (u < maxU
 *                && v < maxV && u > minU && v > minV), cosTheta < 0.5
 *   window       octave o = predictLevel(max_dist, d) clamped to [0, min(7, n_levels - 1)]; radius ((cosTheta > 0.998f ? 2.5f : 4.0f)
 *                * th) * (sf[o] * sf[o]) in float, in that order; octaves max(0, o - 1) .. min(n_levels - 1, o + 1) (clamped, unlike
 *                searchBySim3); findFeaturesInArea over the keyframe's grid: rows outer, columns inner, index order inside a cell; no
 *                filter on the keyframe's features
 *   best match   getBestMatch (:967-990): first minimum; the second best is never an earlier record, INT_MAX with one candidate
 *   accepted     the list is not empty && best < dist_threshold && (float)best / (float)second < ratio (both strict, :591)
 * n_kf in 0 .. ORBFE_FUSE_MAX_KF, m <= 2^20; n_kf * m above ORBFE_FUSE_POINTS_MAX_PAIRS: ORBFE_EBADSIZE.  n_kf == 0 or m == 0: ORBFE_OK,
 * nothing written.  ORBFE_EBADARG, nothing written: an unknown id, n_levels below the store's, a NULL array with a non-zero count, a
 * pose entry, th or ratio not finite, a context on another device.  An id may appear twice.  Locks: the context's, then the store's
 * (shared) for the whole synchronous duration.  One upload, two launches (one thread per pair projects and lists the pairs in vision,
 * one wave per listed pair searches), one download.  The result does not depend on the order of the list.                            */
#define ORBFE_FUSE_POINTS_MAX_PAIRS (1 << 22)
orbfe_status orbfe_fuse_points_into_keyframes_stored(orbfe_ctx* ctx, orbfe_kfstore* store, int32_t n_kf, const uint64_t* kf_ids,
                                                     const orbfe_fuse_pose* poses /*[n_kf]*/, const orbfe_sim3_points* pts,
                                                     const orbfe_camera* cam, const float* scale_factors, int32_t n_levels, float th,
                                                     float ratio, int32_t dist_threshold, int32_t* best_idx /*[n_kf][m]*/,
                                                     int32_t* best_dist /*[n_kf][m]*/);

/* ---- the relocalisation refine over a stored keyframe -------------------------------------------------------------------
 * What Tracking::trackReLocalize does with ONE PnP hypothesis (src/Tracking.cc:565-584, addMatchByProject :612-629) as one call:
 * setCurrFrameAttrib's map points, Optimizer::OptimizePoseOnly with its projection post-check (src/Optimizer.cc:33-203), the 10 / 50
 * decisions, ORBMatcher::searchByProjection(frame, keyframe, matches, th) (src/ORBMatcher.cc:265-347, bFuse == false) with th_first,
 * OptimizePoseOnly again, the search with th_second.  The frame's features are the device-resident results of `slot`, the keyframe's
 * features, descriptors and octaves are read where the store keeps them; only map state goes up.
 *   seed        the edges are the features f with held[f] >= 0 and good[held[f]], in feature order; the initial estimate is
 *               Converter::ConvertTcw2SE3 of (Rcw, tcw) in fp64 (Eigen's trace / largest-diagonal branches, normalised twice, w >= 0)
 *   optimise    orbfe_pose_only_optimize's kernel on the device-built edge list
 *   post-check  VirtualFrame::project2UV with the pose the frame still has -- setPose comes last (Optimizer.cc:201): the PnP pose in the
 *               first optimisation, Tcw[0] in the second: p = Rcw * X + tcw as orbfe_project_map_points computes it, u = x / z * fx +
 *               cx, v = y / z * fy + cy in float; an inlier edge is dropped when !(z > 0) || u > max_u || u < 0 || v > max_v || v < 0;
 *               n_inliers = edges - nBad; every feature that is no inlier loses its point; Tcw = Converter::ConvertSE32Tcw of the
 *               estimate is the frame's pose from here on
 *   decide #1   n_inliers < min_inliers: REJECT_1; n_inliers >= enough: ACCEPT_1; else search #1
 *   search      twc = -(Rcw^T tcw), tlc = kf_Rcw twc + kf_tcw in float, a row times a vector summed left to right (tlc_z = tlc[2]);
 *               |tlc_z| > baseline: forward (tlc_z > 0, octaves [o, 7]) or backward ([0, o]), else [max(0, o - 1), min(o + 1, 7)];
 *               queries = the keyframe's features i with good[i], in index order, radius th * level_sigma2[o]; candidates = the frame's
 *               features of the window that hold no point (one excluded_hit per occurrence of one that does); getBestMatch; accepted when
 *               the list is not empty && (float)best / (float)second < ratio && best < min_threshold; setMapPoints in query order, the
 *               last query that picked a feature keeps it; n_added = the accepted queries
 *   decide #2   n_added[0] + n_inliers[0] < enough: REJECT_2; else optimise #2 from ConvertTcw2SE3 of Tcw[0] on what the frame holds
 *               now, and the post-check again
 *   decide #3   n_inliers[1] >= enough: ACCEPT_2; else search #2 with th_second and Tcw[1]; n_added[1] + n_inliers[1] < enough:
 *               REJECT_3, else ACCEPT_3
 * Outputs per stage s (0: first optimisation and search, 1: second): n_edges[s], n_inliers[s], inlier[s][f] (after the post-check),
 * pose_se3[s] (the estimate, qx qy qz qw tx ty tz), Tcw[s] (Rcw row-major, then tcw), tlc_z[s], n_added[s], assigned[s][f] (the keyframe
 * feature whose point frame feature f holds after search s, -1 none), excluded_hits[s][f], query_accepted[s][i]; final_assigned[f] is
 * what the frame holds when the verdict falls.  A stage that did not run leaves zeros, -1 in assigned.  Every output array is required.
 * ORBFE_EBADARG, nothing written: an unknown id, n unequal to the stored count, held[f] outside [-1, n), a pose, bounds or camera entry
 * not finite, the context's n_levels below the store's, a NULL array, a context on another device.  ORBFE_EBADSIZE: a context of more
 * than 2048 features.  Locks: the context's, then the store's (shared) for the whole synchronous duration.  One upload, one launch
 * sequence whose kernels leave at once after the verdict has fallen, one download; no synchronisation in between.                      */
typedef enum orbfe_reloc_verdict {
  ORBFE_RELOC_REJECT_1 = 1, /* fewer than min_inliers after the first optimisation (Tracking.cc:567)            */
  ORBFE_RELOC_ACCEPT_1 = 2, /* at least `enough` after the first optimisation (:579-584)                       */
  ORBFE_RELOC_REJECT_2 = 3, /* the first search added too few (:619)                                           */
  ORBFE_RELOC_ACCEPT_2 = 4, /* at least `enough` after the second optimisation (:622)                          */
  ORBFE_RELOC_REJECT_3 = 5, /* the second search added too few (:625)                                          */
  ORBFE_RELOC_ACCEPT_3 = 6
} orbfe_reloc_verdict;
typedef struct orbfe_reloc_input {
  uint64_t kf_id;                /* the candidate keyframe in the store                                                   */
  int32_t n;                     /* must equal the stored count                                                           */
  const uint8_t* good;           /* [n] the keyframe feature's map point is non-null and not bad                          */
  const float* pos;              /* [n][3] MapPoint::getPos() (read where good)                                           */
  float kf_Rcw[9], kf_tcw[3];    /* the keyframe's pose                                                                   */
  const int32_t* held;           /* [n_features] keyframe feature whose point setCurrFrameAttrib gives frame feature f, -1 */
  const double* right_u;         /* [n_features], nullable (every edge mono)                                              */
  float Rcw[9], tcw[3];          /* the PnP pose                                                                          */
  float bounds[4];               /* the frame's mfMinU mfMaxU mfMinV mfMaxV                                               */
  const float* level_sigma2;     /* [n_levels of the context]                                                             */
  const float* level_inv_sigma2; /* [n_levels of the context]                                                             */
  const orbfe_camera* cam;       /* fx fy cx cy bf (an undistorting camera: the features of the slot are the undistorted ones) */
  float baseline;                /* Camera::mfBl                                                                          */
  float th_first, th_second;     /* 10, 3 (Tracking.cc:618, 624)                                                          */
  float ratio;                   /* ORBMatcher::mfRatio (0.9)                                                             */
  int32_t min_threshold;         /* ORBMatcher::mnMinThreshold                                                            */
  int32_t min_inliers, enough;   /* 10, 50                                                                                */
} orbfe_reloc_input;
typedef struct orbfe_reloc_output {
  int32_t* verdict;          /* [1] orbfe_reloc_verdict     */
  int32_t* n_edges;          /* [2]                         */
  int32_t* n_inliers;        /* [2]                         */
  int32_t* n_added;          /* [2]                         */
  float* tlc_z;              /* [2]                         */
  double* pose_se3;          /* [2][7]                      */
  float* Tcw;                /* [2][12]                     */
  uint8_t* inlier;           /* [2][n_features]             */
  int32_t* assigned;         /* [2][n_features]             */
  int32_t* final_assigned;   /* [n_features]                */
  int32_t* excluded_hits;    /* [2][n_features]             */
  uint8_t* query_accepted;   /* [2][n]                      */
} orbfe_reloc_output;
orbfe_status orbfe_reloc_refine_stored(orbfe_ctx* ctx, int32_t slot, orbfe_kfstore* store, const orbfe_reloc_input* in,
                                       const orbfe_reloc_output* out);

/* ---- trackReference over a stored keyframe -------------------------------------------------------------------------------
 * Tracking::trackReference (src/Tracking.cc:360-371) as one call: Frame::computeBow (include/ORB_SLAM2/Frame.h:224-229),
 * ORBMatcher::searchByBow(frame, keyframe) with verifyAngle and setMapPoints (src/ORBMatcher.cc:170-253, 815-830, 1013-1051), the :365
 * decision, Optimizer::OptimizePoseOnly with its projection post-check (src/Optimizer.cc:33-203), the :370 decision.  The frame's
 * keypoints, descriptors, angles and count are the device-resident results of `slot`; the reference keyframe's features, angles and
 * FeatureVector are read where the store keeps them; only map state goes up.
 *   T1 bow        vocab != NULL: orbfe_bow_slots' transform of the slot at `levelsup`; vocab == NULL: the host FeatureVector of the input
 *                 (a frame whose computeBow has run; it must be the vector of the frame in `slot`: a feature index at or past the
 *                 slot's keypoint count is matched against nothing meaningful and never receives a point).  Exactly one of the two;
 *                 they are bit-identical by construction
 *   T2 matches    orbfe_search_by_bow_stored's list for this one candidate in mode ORBFE_BOW_TRACK: keyframe flags `good`, frame flags
 *                 `frame_good` (NULL: setMapPointsNull()), the reference's order, verifyAngle when check_orientation is set
 *   T3 assign     setMapPoints in match order: frame feature `query` takes keyframe feature `train`'s point; of several matches that
 *                 name one frame feature the last keeps it.  addMatchInTrack is the caller's, once per MATCH
 *   T4 decide #1  n_matches < min_matches: REJECT_MATCHES; matches and assigned are reported (the reference has written the frame by
 *                 then, :251 before :365), final_assigned = assigned, everything of the optimisation is zero
 *   T5 edges      the features that hold a point, their own (frame_good) or an assigned one, in feature order; Xw from frame_pos[f] or
 *                 pos[assigned[f]]; mono when right_u[f] < 0; information and thresholds as orbfe_pose_only_optimize
 *   T6 optimise   from Converter::ConvertTcw2SE3 of (Rcw, tcw) (the relocalisation refine's seed), orbfe_pose_only_optimize's kernel
 *   T7 post-check the relocalisation refine's, with the pose the frame still has (the input pose); n_inliers = edges - nBad; every
 *                 feature that is no inlier loses its point (final_assigned); Tcw = Converter::ConvertSE32Tcw of the estimate
 *   T8 decide #2  n_inliers >= min_inliers: ACCEPT, else REJECT_INLIERS
 * Outputs, every array required but bow: verdict, n_matches, matches [n] (one per keyframe feature at most), assigned [n_features] (the
 * keyframe feature whose point frame feature f holds after setMapPoints, -1 none, ORBFE_TRACKREF_OWN the point it came with), n_edges,
 * n_inliers, inlier [n_features] (after the post-check), final_assigned [n_features], pose_se3 (qx qy qz qw tx ty tz), Tcw (Rcw row-major,
 * then tcw); bow (nullable, ignored with vocab == NULL) receives the frame's BowVector and FeatureVector in orbfe_bow_slots' layout for
 * one slot -- Frame::mBowVec / mFeatVec, which KeyFrameDB needs later.
 * ORBFE_EBADARG, nothing written: an unknown id, n unequal to the stored count, a keyframe without FeatureVector, both or neither of
 * vocab and a host FeatureVector, a malformed host FeatureVector (orbfe_kfstore_set_bow's checks), a pose, bounds or camera entry not
 * finite, a NULL required array, the context's n_levels below the store's, a context on another device.  ORBFE_EBADSIZE: a context of
 * more than 2048 features.  Locks: the context's, then the store's (shared) for the whole synchronous duration.  One upload, one launch
 * sequence (transform, match, select, seed, optimise, check) whose kernels after the seed leave at once when the verdict has fallen,
 * one download; no synchronisation in between.                                                                                        */
typedef enum orbfe_trackref_verdict {
  ORBFE_TRACKREF_REJECT_MATCHES = 1, /* fewer than min_matches matches (Tracking.cc:365)   */
  ORBFE_TRACKREF_REJECT_INLIERS = 2, /* fewer than min_inliers after the optimisation (:370) */
  ORBFE_TRACKREF_ACCEPT = 3
} orbfe_trackref_verdict;
#define ORBFE_TRACKREF_OWN (-2)
typedef struct orbfe_trackref_input {
  uint64_t kf_id;                /* the reference keyframe in the store (it needs a FeatureVector)                        */
  int32_t n;                     /* must equal the stored count                                                           */
  const uint8_t* good;           /* [n] the keyframe feature's map point is non-null and not bad                          */
  const float* pos;              /* [n][3] MapPoint::getPos() (read where good)                                           */
  const uint8_t* frame_good;     /* [n_features], nullable: the frame feature came with a good point                      */
  const float* frame_pos;        /* [n_features][3], read where frame_good is set (required with frame_good)              */
  const double* right_u;         /* [n_features], nullable (every edge mono)                                              */
  float Rcw[9], tcw[3];          /* the pose the frame has: the last frame's (Tracking.cc:121)                            */
  float bounds[4];               /* the frame's mfMinU mfMaxU mfMinV mfMaxV                                               */
  const float* level_sigma2;     /* [n_levels of the context]                                                             */
  const float* level_inv_sigma2; /* [n_levels of the context]                                                             */
  const orbfe_camera* cam;       /* fx fy cx cy bf                                                                        */
  int32_t levelsup;              /* 4                                                                                     */
  float ratio;                   /* 0.7                                                                                   */
  int32_t dist_threshold;        /* ORBMatcher::mnMinThreshold                                                            */
  int32_t check_orientation;     /* 1                                                                                     */
  int32_t min_matches;           /* 10 (the comment at :355 says 15, the code at :365 says 10)                            */
  int32_t min_inliers;           /* 10                                                                                    */
  int32_t n_nodes;               /* the frame's FeatureVector in orbfe_bow_out's layout: used iff vocab == NULL           */
  const uint32_t* nodes;
  const int32_t* node_offsets;
  const uint32_t* features;
} orbfe_trackref_input;
typedef struct orbfe_trackref_output {
  int32_t* verdict;           /* [1] orbfe_trackref_verdict  */
  int32_t* n_matches;         /* [1]                         */
  orbfe_bow_match* matches;   /* [n]                         */
  int32_t* assigned;          /* [n_features]                */
  int32_t* n_edges;           /* [1]                         */
  int32_t* n_inliers;         /* [1]                         */
  uint8_t* inlier;            /* [n_features]                */
  int32_t* final_assigned;    /* [n_features]                */
  double* pose_se3;           /* [7]                         */
  float* Tcw;                 /* [12]                        */
  const orbfe_bow_out* bow;   /* nullable                    */
} orbfe_trackref_output;
orbfe_status orbfe_track_reference_stored(orbfe_ctx* ctx, int32_t slot, const orbfe_vocab* vocab, orbfe_kfstore* store,
                                          const orbfe_trackref_input* in, const orbfe_trackref_output* out);

/* ---- map points resident on the device ------------------------------------------------------------------------------
 * The half the keyframe store leaves out: one orbfe_mpstore holds, on ONE device and keyed by MapPoint::getID() (uint64), what
 * orbfe_track_local_map uploads per local map point on every frame -- a row of exactly 64 bytes: pos[3], view_dir[3], max_dist, min_dist
 * (float) and desc[32].  The host objects stay the truth: the store holds what the last upsert brought, and the caller upserts a point
 * when setPos / setDesc / updateNormalAndDepth changed it.  isBad / isInMap are not stored: they travel as flags
 * with every call.
 * A paged direct index, no hash (the ids are sequential): page id / rows_per_page, row id % rows_per_page.  A page (its rows, then one
 * presence byte per row: no value inside a row marks absence) is allocated by the first upsert that names one of its rows and never
 * moves; the page table is a device array of page pointers.  The store has its own lock and serves every context on its device: upsert
 * and erase take it exclusively; fetch, size and orbfe_track_local_map_stored take it shared for their whole (synchronous) duration.
 *   create   rows_per_page 0: 16384, at most ORBFE_MP_MAX_ROWS_PER_PAGE; max_pages 0: 4096, at most ORBFE_MP_MAX_PAGES (the defaults: 64 Mi
 *            ids; 1 MB + 16 KB of device memory per page in use).  create allocates the page table, 8 bytes per possible page.
 *   upsert   fields: which arrays of the call are written, ORBFE_MP_POS (pos) | ORBFE_MP_NORMAL_DEPTH (view_dir, max_dist, min_dist) |
 *            ORBFE_MP_DESC (desc); an array the mask does not name may be NULL.  Refused with ORBFE_EBADARG, nothing changed: an empty
 *            or unknown mask, an id the store does not hold without all three fields (no row is ever half-initialised), an id listed
 *            twice in the call.  An id at or past rows_per_page * max_pages: ORBFE_ECAPACITY, nothing changed.  One staged copy and one
 *            launch; the call returns after the rows are on the device: every later call on any context of the device sees them.
 *   erase    unknown ids are ignored.
 *   fetch    the rows of n ids (an id may repeat) into the arrays whose pointer is not NULL; an id the store does not hold:
 *            ORBFE_EBADARG, nothing written.
 *   size     n_points; bytes_used = 64 * n_points; bytes_reserved = pages in use * rows_per_page * 65.
 * orbfe_track_local_map_stored is orbfe_track_local_map with the map points named by id: ids[n_mp] in place of pos, view_dir, max_dist,
 * min_dist and desc, every other field with its meaning there.  An id may repeat.  One launch in front of the chain gathers the rows into
 * the arrays the chain reads; every output byte is what orbfe_track_local_map writes given the arrays orbfe_mpstore_fetch returns for
 * `ids`.  Still ONE synchronisation: an id the store does not hold is found on the device (its point takes no part in the chain) and
 * reported after the download -- ORBFE_EBADARG naming the first such id, none of the outputs written.  A store on another device than the
 * context, ids NULL with n_mp > 0: ORBFE_EBADARG.  More than 2048 features per frame: ORBFE_EBADSIZE.                              */
#define ORBFE_MP_POS 1u
#define ORBFE_MP_NORMAL_DEPTH 2u
#define ORBFE_MP_DESC 4u
#define ORBFE_MP_ALL 7u
#define ORBFE_MP_MAX_ROWS_PER_PAGE (1 << 20)
#define ORBFE_MP_MAX_PAGES (1 << 16)
typedef struct orbfe_mpstore orbfe_mpstore;
typedef struct orbfe_track_stored_input {
  int32_t n_mp;
  const uint64_t* ids;           /* [n_mp] MapPoint::getID()                                                       */
  const uint8_t* flags;          /* [n_mp], as orbfe_track_input                                                   */
  const int32_t* held;           /* [n_features], nullable: index into ids                                         */
  const double* right_u;         /* [n_features], nullable                                                         */
  const float* level_sigma2;     /* [n_levels]                                                                     */
  const float* level_inv_sigma2; /* [n_levels]                                                                     */
  const double* pose_se3;        /* [7]                                                                            */
  float th;
  float ratio;
  int32_t min_threshold;
  int32_t min_matches;
} orbfe_track_stored_input;
orbfe_status orbfe_mpstore_create(int32_t device_id, int32_t rows_per_page, int32_t max_pages, orbfe_mpstore** out);
void orbfe_mpstore_destroy(orbfe_mpstore* store);  /* no call on the store may still run */
orbfe_status orbfe_mpstore_upsert(orbfe_mpstore* store, int32_t n, const uint64_t* ids, uint32_t fields, const float* pos /*[n][3]*/,
                                  const float* view_dir /*[n][3]*/, const float* max_dist /*[n]*/, const float* min_dist /*[n]*/,
                                  const uint8_t* desc /*[n][32]*/);
orbfe_status orbfe_mpstore_erase(orbfe_mpstore* store, int32_t n, const uint64_t* ids);
orbfe_status orbfe_mpstore_fetch(orbfe_mpstore* store, int32_t n, const uint64_t* ids, float* pos, float* view_dir, float* max_dist,
                                 float* min_dist, uint8_t* desc);
orbfe_status orbfe_mpstore_size(orbfe_mpstore* store, int64_t* n_points, int64_t* bytes_used, int64_t* bytes_reserved);
orbfe_status orbfe_track_local_map_stored(orbfe_ctx* ctx, int32_t slot, orbfe_mpstore* store, const orbfe_frame_pose* pose,
                                          const orbfe_camera* cam, const orbfe_track_stored_input* in, const orbfe_track_output* out);

/* ---- trackMotionModel over two frame slots -------------------------------------------------------------------------------
 * Tracking::trackMotionModel (src/Tracking.cc:381-406) from processLastFrame's unProject (:384; src/Frame.cc:179-202, :262-275) to the
 * return of :405 as one call: the two ORBMatcher::searchByProjection(frame, lastFrame, matches, th) (src/ORBMatcher.cc:265-347, 815-830),
 * the :388 and :392 decisions, Optimizer::OptimizePoseOnly with its projection post-check (src/Optimizer.cc:33-203), the isInMap count of
 * :397-404.  Both frames are read where their extraction left them: `slot` / `last_slot` are the extraction slots of the current and the
 * last frame's left image on this context, `pair` / `last_pair` the stereo pairs whose device-resident results give the current frame's
 * right_u and the last frame's depth (orbfe_kfstore_add_from_slot's convention; pair < 0: every edge mono; last_pair < 0: no depth, no
 * temporary point).  Only map state goes up: one flag byte per last-frame feature and the id of its point in `store` (or, with store ==
 * NULL, its position).  The current frame arrives holding no map point (the state after createStereo / createRGBD, the only call site).
 *   M1 unProject  a last-frame feature below the last slot's count with flag bit 0 clear and depth >= 0 gets a temporary point:
 *                 x = (pt.x - cx) / fx, y = (pt.y - cy) / fy in float; p3dC = (float)(depth x), (float)(depth y), (float)depth, depth a
 *                 double; p3dW = Rwc p3dC + twc as cv::gemm does it.  A temporary point is good and not in the map (temp, temp_pos)
 *   M2 direction  twc1 = -Rcw^T tcw, tlc = last_Rcw twc1 + last_tcw; |tlc.z| > baseline: up (z > 0) or down (:270-280)
 *   M3 queries    the last frame's features that hold a good point, their own or a temporary one, in feature order: centre the
 *                 feature's position, radius th * level_sigma2[octave], octaves [o, 7] (up), [0, o] (down) or [max(0, o - 1),
 *                 min(o + 1, 7)] (:300-313), the descriptor the last slot's
 *   M4 search 1   orbfe_track_motion_model's: findFeaturesInArea, candidates that hold a good point dropped and counted
 *                 (excluded_hits; none in this search, the frame arrives empty), getBestMatch, accepted when ratio < mfRatio and
 *                 distance < mnMinThreshold; setMapPoints in query order: the last query that names a feature keeps it
 *   M5 search 2   decided on the device: n_matches < min_matches and th_second > 0.  Radius th_second * level_sigma2[octave]; the
 *                 features search 1 assigned are dropped and counted; the matches of search 1 stay; n_matches is the sum; passes = 2
 *   M6 decide #1  n_matches < min_matches: REJECT_MATCHES; assigned (= final_assigned), the hits, query_matches and the temporaries are
 *                 reported (the reference has written both frames by then), everything of the optimisation is zero
 *   M7 optimise   the edges are the features that hold a point, in feature order; mono when right_u[f] < 0; from
 *                 Converter::ConvertTcw2SE3 of (Rcw, tcw); orbfe_pose_only_optimize's kernel
 *   M8 post-check the relocalisation refine's, with the pose the frame still has (the predicted one); n_inliers = edges - nBad; a
 *                 feature that is no inlier loses its point (final_assigned); Tcw = Converter::ConvertSE32Tcw of the estimate
 *   M9 count      n_in_map = the features that still hold a point whose flags are 3 (bit 1 is read only where bit 0 is set: a
 *                 temporary point never counts)
 *   M10 decide #2 n_in_map >= min_inliers: ACCEPT, else REJECT_INLIERS
 * Inputs: last_flags [n_last], n_last = the context's feature capacity: bit 0 the feature's point is non-null and not bad, bit 1 that
 * point isInMap(); exactly one of last_ids [n_last] (read where bit 0 is set, looked up in `store`; an id may repeat) with a store and
 * last_pos [n_last][3] without one; (Rcw, tcw) the predicted pose the frame has (:385); last_Rcw, last_tcw, last_Rwc, last_twc the last
 * frame's pose after :689, the reference's float members.  Outputs, every array required: verdict, passes (1 or 2), n_matches, n_edges,
 * n_inliers, n_in_map; per frame feature [n_features]: assigned (the LAST-FRAME FEATURE whose point frame feature f holds, -1 none),
 * final_assigned, inlier, excluded_hits; per last-frame feature [n_last]: query_matches (in how many searches its query was accepted:
 * one addMatchInTrack each), temp (M1 made a point), temp_pos [n_last][3]; pose_se3 (qx qy qz qw tx ty tz), Tcw (Rcw row-major, then tcw).
 * ORBFE_EBADARG, nothing written: a NULL required array, both or neither of store + last_ids and last_pos, slot == last_slot, a slot or a
 * pair out of range, a pose, bounds or camera entry not finite, a store on another device.  An id the store does not hold is found on
 * the device and reported after the download: ORBFE_EBADARG naming the first such id, none of the outputs written.  ORBFE_EBADSIZE: more
 * than 2048 features per frame, a grid past the LDS counters.  Locks: the context's, then the store's (shared) for the whole synchronous
 * duration.  One upload, one launch sequence (prepare, search, claim, between, search, claim, edges, optimise, check) whose second
 * search leaves at once when it is not needed, one download; no synchronisation in between.                                          */
typedef enum orbfe_motion_verdict {
  ORBFE_MOTION_REJECT_MATCHES = 1, /* fewer than min_matches matches after both searches (Tracking.cc:392) */
  ORBFE_MOTION_REJECT_INLIERS = 2, /* fewer than min_inliers in-map points after the optimisation (:405)   */
  ORBFE_MOTION_ACCEPT = 3
} orbfe_motion_verdict;
typedef struct orbfe_motion_slots_input {
  const uint8_t* last_flags;     /* [n_last] bit 0: good point, bit 1: that point isInMap()                               */
  const uint64_t* last_ids;      /* [n_last] MapPoint::getID(), read where bit 0 is set (with a store)                    */
  const float* last_pos;         /* [n_last][3] MapPoint::getPos(), read where bit 0 is set (without a store)             */
  float Rcw[9], tcw[3];          /* the predicted pose the frame has (Tracking.cc:385)                                    */
  float last_Rcw[9], last_tcw[3], last_Rwc[9], last_twc[3]; /* the last frame's pose after :689                           */
  float bounds[4];               /* the frame's mfMinU mfMaxU mfMinV mfMaxV                                               */
  const orbfe_camera* cam;       /* fx fy cx cy bf                                                                        */
  float baseline;                /* Camera::mfBl                                                                          */
  const float* level_sigma2;     /* [n_levels of the context]                                                             */
  const float* level_inv_sigma2; /* [n_levels of the context]                                                             */
  float th, th_second;           /* 15, 30; th_second <= 0: no second search                                              */
  float ratio;                   /* 0.9                                                                                   */
  int32_t min_threshold;         /* ORBMatcher::mnMinThreshold                                                            */
  int32_t min_matches;           /* 20                                                                                    */
  int32_t min_inliers;           /* 10                                                                                    */
} orbfe_motion_slots_input;
typedef struct orbfe_motion_slots_output {
  int32_t* verdict;           /* [1] orbfe_motion_verdict    */
  int32_t* passes;            /* [1]                         */
  int32_t* n_matches;         /* [1]                         */
  int32_t* n_edges;           /* [1]                         */
  int32_t* n_inliers;         /* [1]                         */
  int32_t* n_in_map;          /* [1]                         */
  int32_t* assigned;          /* [n_features]                */
  int32_t* final_assigned;    /* [n_features]                */
  uint8_t* inlier;            /* [n_features]                */
  int32_t* excluded_hits;     /* [n_features]                */
  int32_t* query_matches;     /* [n_last]                    */
  uint8_t* temp;              /* [n_last]                    */
  float* temp_pos;            /* [n_last][3]                 */
  double* pose_se3;           /* [7]                         */
  float* Tcw;                 /* [12]                        */
} orbfe_motion_slots_output;
orbfe_status orbfe_track_motion_model_slots(orbfe_ctx* ctx, int32_t slot, int32_t pair, int32_t last_slot, int32_t last_pair,
                                            orbfe_mpstore* store /* nullable */, const orbfe_motion_slots_input* in,
                                            const orbfe_motion_slots_output* out);

/* ---- instrumentation ---------------------------------------------------------------------------
 * Stage timing with HIP events on the context stream.  Enable, run, then read the accumulated
 * per-stage milliseconds and launch counts.  Stage ids: see orbfe_stage.                             */
typedef enum orbfe_stage {
  ORBFE_STAGE_RESIZE = 0,
  ORBFE_STAGE_BLUR = 1,
  ORBFE_STAGE_FAST = 2,
  ORBFE_STAGE_QUADTREE = 3,
  ORBFE_STAGE_BRIEF = 4,
  ORBFE_STAGE_STEREO = 5,
  ORBFE_STAGE_MATCH = 6,
  ORBFE_STAGE_BA = 7,
  ORBFE_STAGE_COUNT = 8
} orbfe_stage;
/* on = 0: off.  on = 1: every stage timed ALONE (the overlaps between streams and the graph replay are switched off, kernels run in
 * line).  on = 2 + stage: only that stage is timed, inside the production schedule (what rocprofv3 sees for its kernels).            */
orbfe_status orbfe_profile_enable(orbfe_ctx* ctx, int32_t on);
orbfe_status orbfe_profile_read(orbfe_ctx* ctx, double* ms /*[ORBFE_STAGE_COUNT]*/, int64_t* launches /*[..]*/, int32_t reset);
const char* orbfe_stage_name(int32_t stage);

/* ---- debugging / parity aids (used by tests; stable but not part of the drop-in surface) -------
 * FAST candidates of (slot, level) in the reference's order (cell-row-major, in-cell raster), region
 * coordinates: xyr[3*i] = x, y, response.  Returns the count through n_out even if cap is too small.  */
orbfe_status orbfe_debug_candidates(orbfe_ctx* ctx, int32_t slot, int32_t level, float* xyr, int32_t cap, int32_t* n_out);
/* The device exp-map update of the pose and local-BA optimisers on n independent items: out[i] = exp(upd[i]) * poses[i] with g2o's
 * normalizeRotation (unit quaternion, w >= 0).  A pose is (qx, qy, qz, qw, tx, ty, tz), an update (omega, upsilon).  n == 0 does nothing;
 * n < 0 or a NULL array is ORBFE_EBADARG.                                                              */
orbfe_status orbfe_debug_se3_oplus(orbfe_ctx* ctx, int32_t n, const double* poses /*[n][7]*/, const double* upd /*[n][6]*/,
                                   double* out /*[n][7]*/);
/* One dense symmetric positive-definite system S x = rhs of nb 6x6 block rows through one of the four reduced-system solvers of
 * orbfe_ba_local_optimize, in the layout and through the launch code the optimiser gives that solver.  solver 0: registers (nb 1..42),
 * 1: blocked, matrix cores (43..1000), 2: LDS (1..100), 3: panel in global memory (>= 101); any other nb, a NULL argument or nb < 1 is
 * ORBFE_EBADARG.  Only the lower triangle (i >= j) of S bears on the result.  *ok = 0 and x = 0 when a pivot is not positive and finite
 * (the optimiser rejects such a trial); that is ORBFE_OK.  Callable any number of times on one context: for solver 1 the state the
 * blocked solver keeps between the trials of one optimisation (its bad-pivot flag among it) is kept between calls of one nb.         */
orbfe_status orbfe_debug_reduced_solve(orbfe_ctx* ctx, int32_t solver, int32_t nb,
                                       const double* S /*[6nb][6nb] row-major, symmetric; only i >= j is read*/,
                                       const double* rhs /*[6nb]*/, double* x /*[6nb]*/, int32_t* ok);

/* The edges of orbfe_sim3_optimize as the optimiser sees them, at the estimate est (qx qy qz qw tx ty tz s): err[i] = the errors of
 * pair i's EdgeSim3ProjectXYZ (u, v) and EdgeInverseSim3ProjectXYZ (u, v), chi2[i] their two chi2, jac[i][edge][row][d] the numeric
 * Jacobians (d: omega, upsilon; the scale column is 0 and is left out).  n == 0 does nothing; n < 0 or a NULL array is ORBFE_EBADARG. */
orbfe_status orbfe_debug_sim3_edges(orbfe_ctx* ctx, int32_t n, const float* pc /*[n][3]*/, const float* pm /*[n][3]*/,
                                    const float* uv_c /*[n][2]*/, const float* uv_m /*[n][2]*/, const double* info_c /*[n]*/,
                                    const double* info_m /*[n]*/, float fx, float fy, float cx, float cy, const double* est /*[8]*/,
                                    double* err /*[n][4]*/, double* chi2 /*[n][2]*/, double* jac /*[n][2][2][6]*/);

/* The edges of orbfe_pose_graph_optimize as the optimiser sees them, at the graph's own estimates: err[e] = log(meas * S_v0 * S_v1^-1)
 * (omega, upsilon; the scale entry is 0 and is left out), chi2[e] = err . err, jac[e][v][row][d] the numeric Jacobians of vertex 0 and
 * vertex 1 (d: omega, upsilon), all zero for a fixed vertex.  The graph is checked as orbfe_pose_graph_optimize checks it (any number
 * of non-fixed vertices); n_edges == 0 does nothing; a NULL output is ORBFE_EBADARG.                                                 */
orbfe_status orbfe_debug_pose_graph_edges(orbfe_ctx* ctx, const orbfe_pose_graph* graph, double* err /*[n_edges][6]*/,
                                          double* chi2 /*[n_edges]*/, double* jac /*[n_edges][2][6][6]*/);
/* Where the last orbfe_pose_graph_optimize of this process spent its time, in milliseconds of wall time with the stream synchronised
 * after every phase: ms[0] build (errors, Jacobians, per-edge blocks, chi2), ms[1] assemble (zero fill and block assembly), ms[2] solve
 * (launch_lba_chol), ms[3] evaluate (update, chi2, the sums and the scalars' download).  Only calls made with ORBFE_PG_PHASES set in the
 * environment are measured (and slowed down by the synchronisations); all zero otherwise.  For tools/essential_graph_bench.py.          */
orbfe_status orbfe_debug_pose_graph_phases(double* ms /*[4]*/);
/* One block-sparse symmetric positive definite system through the symbolic phase and the factor-and-solve kernel of
 * orbfe_pose_graph_optimize_ex's solver 2, in the layout the optimiser gives them.  nb block rows of 6; the n_low given blocks are (low_row[q],
 * low_col[q]), low_row >= low_col, each at most once, 36 doubles row-major each (of a diagonal block only the lower triangle is read); every
 * other block is zero.  x [6 nb]; *ok = 0 and x = 0 where a pivot is not positive and finite (the status is still ORBFE_OK); *l_blocks
 * (nullable) = the blocks of the factor.  ORBFE_EBADARG: a NULL argument, nb < 1, a block above the diagonal, out of range or given
 * twice.                                                                                                                              */
orbfe_status orbfe_debug_pg_sparse_solve(orbfe_ctx* ctx, int32_t nb, int32_t n_low, const int32_t* low_row, const int32_t* low_col,
                                         const double* blocks /*[n_low][36]*/, const double* rhs /*[6 nb]*/, double* x /*[6 nb]*/,
                                         int32_t* ok, int64_t* l_blocks /*nullable*/);

/* The reduced camera system of orbfe_ba_global_optimize's solver 2 at ONE linearisation, the given estimates and lambda, as block-CSR
 * over the non-fixed keyframes in index order: *nnzb stored 6x6 blocks, row_off[nf + 1], col[nnzb] (ascending in a row, both triangles,
 * the diagonal always present), blocks[nnzb][36] row-major, rhs[6 nf].  *nnzb and row_off are always written; col, blocks and rhs only
 * if cap_blocks >= *nnzb (call with cap_blocks = 0 to size the arrays, which may then be NULL).                                       */
orbfe_status orbfe_debug_ba_reduced_bsr(orbfe_ctx* ctx, const orbfe_ba_problem* prob, const uint8_t* pose_fixed /*nullable*/, double lambda,
                                        int32_t cap_blocks, int32_t* nnzb, int32_t* row_off, int32_t* col, double* blocks, double* rhs);
/* One block-CSR system S x = rhs of nb 6x6 block rows through the conjugate-gradient solver of orbfe_ba_global_optimize (the layout
 * above; S symmetric, both triangles stored).  tol <= 0: 1e-10, max_iter <= 0: 4 * 6 * nb.  *ok = 1: converged, *iters iterations.
 * *ok = 0 is ORBFE_OK too: a diagonal block that is missing or not positive definite (x = 0), p.Sp not positive and finite, or no
 * convergence within max_iter (x = the last iterate).  A zero right-hand side gives x = 0, *ok = 1, 0 iterations.  A column out of
 * range, a row whose columns do not ascend, nb < 1 or a NULL argument is ORBFE_EBADARG.                                              */
orbfe_status orbfe_debug_bsr_pcg(orbfe_ctx* ctx, int32_t nb, const int32_t* row_off, const int32_t* col, const double* blocks,
                                 const double* rhs, double tol, int32_t max_iter, double* x, int32_t* iters, int32_t* ok);
/* Where the last orbfe_ba_global_optimize (solver 2) of this process spent its time: ms[0] build (evaluation and normal equations),
 * ms[1] Schur (point inverses, W, the block-CSR system), ms[2] PCG, ms[3] evaluate (update, chi2, the scalars' download), in
 * milliseconds of wall time with the stream synchronised after every phase, and ms[4] = kernel launches and copies enqueued (the solver's counted, the few around it per trial a constant).  Only calls
 * made with ORBFE_GBA_PHASES set in the environment are measured; all zero otherwise.  For tools/global_ba_bench.py.                  */
orbfe_status orbfe_debug_ba_global_phases(double* ms /*[5]*/);
/* Device milliseconds, between events, of the two kernels of the last orbfe_fuse_points_into_keyframes_stored of this process that ran
 * with the MATCH stage timed (orbfe_profile_enable): ms[0] the projection, ms[1] the search; zero before.  For tools/fuse_points_bench.py. */
orbfe_status orbfe_debug_fuse_points_kernels(double* ms /*[2]*/);

#ifdef __cplusplus
}
#endif
#endif /* ORBFE_H_ */
