/*
 * lslam_c.h -- C ABI of the MI355X-native nonlinear-least-squares backend for L_SLAM.
 *
 * This is the drop-in boundary for the reference's scan-match hot path.  The
 * reference has no FFI seam; its seam is the C++ class lidar_slam::ScanMatch
 * (scan_to_scan_match/ScanMatch.h:21-61), called from
 *   odometry/LaserMatcher.cpp:327-331      (LaserMatcher::optimizeTransform)
 *   pose_graph/graph.cpp:185-190           (Graph::getFinalFeatureMap)
 *   pose_graph/loop_detector.hpp:206-223   (LoopDetector::matching_nearest)
 * Every entry point below names the reference interface it replaces.  All paths
 * are relative to /root/reference/L_SLAM/src/.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types cross the ABI.
 *   - Clouds are caller-owned host arrays of points `stride_bytes` apart, x,y,z
 *     as three consecutive floats at offset 0 (pcl::PointXYZI: stride 32;
 *     packed float4: 16; packed xyz: 12).  The library copies what it needs to
 *     HBM; the caller's buffers are only read during the call.
 *   - pose is {rot_x, rot_y, rot_z, pos_x, pos_y, pos_z} = the reference's
 *     Twist (util/Twist.h:13-36); p_map = Rz(rz)*Ry(ry)*Rx(rx)*p + pos
 *     (util/transform_utils.h:288-299).
 *   - Functions return lslam_status and never throw.  One call in flight per
 *     ctx (the reference's ScanMatch is not re-entrant either,
 *     ScanMatch.h:63-85); different ctx may be used from different threads/GPUs.
 *   - The library owns all device memory and its HIP stream.
 *   - There is NO CPU fallback: without a usable HIP device every compute entry
 *     point returns LSLAM_ERR_HIP.
 */
#ifndef LSLAM_C_H
#define LSLAM_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lslam_ctx lslam_ctx;

typedef enum {
  /* outcomes of a scan match (ScanMatch::scanMatchScan returns bool; the
   * reasons for `false` are distinguished here) */
  LSLAM_OK = 0,               /* returned true (ScanMatch.cpp:340) */
  LSLAM_TOO_FEW_REF = 1,      /* ScanMatch.cpp:57-61, pose untouched */
  LSLAM_NOT_CONVERGED = 2,    /* ScanMatch.cpp:342-346 (also when use_score is off) */
  LSLAM_LOW_SCORE = 3,        /* ScanMatch.cpp:323-328 */
  LSLAM_LOW_PERCENT = 4,      /* ScanMatch.cpp:330-335 */
  LSLAM_TOO_FEW_MATCHES = 5,  /* ScanMatch.cpp:141-145 break, then :342-346 */
  /* errors */
  LSLAM_ERR_INVALID = -1,     /* bad argument */
  LSLAM_ERR_HIP = -2,         /* HIP runtime error / no device (see lslam_last_error) */
  LSLAM_ERR_NO_MAP = -3,      /* scan match requested before lslam_map_set */
  LSLAM_ERR_NO_SCAN = -4,     /* lslam_scanmatch_run before lslam_scan_set */
  LSLAM_ERR_TREE_DEPTH = -5,  /* kd-tree deeper than the device traversal stack */
  LSLAM_ERR_TREE_BUILD = -6,  /* the device kd-tree builder hit a structure limit (lslam_last_error says which);
                                 nothing is rebuilt on the host -- the call fails */
  LSLAM_ERR_COMM = -7         /* RCCL communicator error (lslam_comm_*) */
} lslam_status;

/* Mirrors ScanMatch's constructor defaults and setters (ScanMatch.cpp:21-33,
 * ScanMatch.h:21-34). */
typedef struct {
  int32_t max_iterations;            /* ScanMatch(maxIterations = 10) */
  float delta_t_abort;               /* setConvergeThreshold, default 0.05 */
  float delta_r_abort;               /* setConvergeThreshold, default 0.05 */
  int32_t use_score;                 /* setUseCore, default 1 */
  int32_t fine_score;                /* setFineScore, default 0: after a converged loop, one more sweep at the final pose gated
                                        on d2[0] < 0.02 (corner) / 0.05 (surf) -> stats.score2 / percent2 (ScanMatch.cpp:272-321;
                                        printed by the reference, never part of the return value) */
  double score_threshold;            /* setScoreThreshold, default 800 */
  double match_percentage_threshold; /* setPercentThreshold, default 0.4 */
  /* backend knobs (no reference counterpart) */
  int32_t jtj_mode;  /* 0: VALU + wave-shuffle reduction of J^T J; 1: MFMA f32 16x16x4 */
  int32_t profile;   /* 1: bracket every sweep launch with HIP events (stats.gpu_ms_sweep) */
  int32_t scans_in_flight; /* lslam_scanmatch_run_batch: resident scans matched together by one sequence of
                              launches; more scans are taken in chunks of this size (0: up to 128; a scan
                              in flight costs ~1.3 MB of scratch in HBM for a 115 200-point scan) */
  int32_t search_mode;     /* how the 5-NN search maps to the GPU: LSLAM_SEARCH_AUTO / _LANE / _PACKET / _GRID, ORed with LSLAM_STACK_* */
  int32_t knn_cert;        /* certificate sweep (neighbour lists carried over, without a search, where a point provably kept its
                              five neighbours): 1 (default) where it pays -- throughput-bound batches; 0 never: every 5-NN search
                              of every sweep is executed; 2 whatever the size of the launch (tests) */
  float cert_try_m;        /* a scan tests certificates when its last update moved its points by less than this [m] (0.05) */
  float cert_track_m;      /* ... and its searches keep the bound a certificate needs when by less than this [m] (1.0) */
  float grid_cell;         /* LSLAM_SEARCH_GRID: edge of a grid cell [m]; 0 = the default (0.6) */
  int32_t debug_stats;     /* 1: count the points the certificate / grid sweeps leave to their second pass (lslam_debug_cert_stats) */
  int32_t ab_switches;     /* LSLAM_AB_*: measured-and-kept alternatives, off by default (DESIGN.md has the numbers); a bit
                              that is none of them is refused with LSLAM_ERR_INVALID before anything is enqueued */
} lslam_opts;
/* Environment overrides of the fields above -- LSLAM_KNN_CERT, LSLAM_CERT_TRY_M, LSLAM_CERT_TRACK_M, LSLAM_GRID_CELL,
 * LSLAM_SEARCH=lane|packet|grid, LSLAM_FORCE_STACK=deep|shallow|auto, LSLAM_AB_SWITCHES=<LSLAM_AB_* bits>,
 * LSLAM_DEBUG_CERT_STATS=1 -- are read ONCE per context, in lslam_ctx_create; the A/B switches of the builders and the loop
 * (LSLAM_UNBOUNDED_KNN, LSLAM_NO_MORTON, LSLAM_HOST_MORTON, LSLAM_TINY_PHASE, LSLAM_NO_REG_NODES, LSLAM_NO_LEVEL_BUILD, ...)
 * once per process, when the first context is created; a pose graph's (LSLAM_PG_*) when it is created.  No entry point reads
 * the environment while it runs.  The hooks tests use to force failure paths (LSLAM_DEBUG_NODE_CAP_DIV,
 * LSLAM_DEBUG_SPIN_LIMIT, LSLAM_DEBUG_PG_ABORT, LSLAM_DEBUG_GJ_ABORT, LSLAM_HUGE_MIN) are the exception, and exist only in a
 * process started with LSLAM_DEBUG_HOOKS=1 (tests/conftest.py sets it); without it they are never looked at. */
/* Bits 1, 2, 4, 8, 32 and 128 named six alternatives that measured slower than what ships (the Gauss-Newton loop as one
 * persistent launch, the solve in the sweep's tail, a second probe, unproven points resolved in place, the fit cache, the
 * second pass by persistent lanes).  They are retired -- HISTORY.md keeps their numbers and the commit that last had them --
 * and, like any bit this enum does not name, are REFUSED: a run call whose ab_switches has one returns LSLAM_ERR_INVALID
 * with the pose untouched, lslam_ctx_create does under such an LSLAM_AB_SWITCHES (lslam_last_error names the bits). */
enum { LSLAM_AB_NO_COMPACT = 64,   /* a batch through the grid sweep: launch every workgroup of every scan in every sweep (round 4's
                                      form) instead of only those of the scans whose loop is still running */
       LSLAM_AB_GRID_GENERAL = 256, /* grid sweep: the production loop's launches through the general instantiation of
                                      sweep_grid_kernel instead of the lean one (the same statements with the shuffle sums, the
                                      taps, the _fineScore gate, the unbounded search and the counters folded away
                                      at compile time, and the five neighbours' points handed from the search to the fit instead
                                      of gathered twice: 61 VGPRs and no scratch at eight wavefronts per SIMD against 72 + 36 B at
                                      seven).  Same bits.  Measured on the headline, the two taken in turn in one session: 1.466 -
                                      1.475e10 with this switch or the library before it, 1.512 - 1.517e10 without: +3.0 %
                                      (profiles/r14_grid_lean.txt).  The switch also keeps the general instantiation of the
                                      sweep's SECOND pass (sweep_queue_kernel; the lean one: the same folding, 12-byte leaf
                                      fetches, nothing carried in registers from work item to work item -- 80 VGPRs and no scratch at
                                      six wavefronts per SIMD against 96 + 68 B at five; same bits, +2.5 %: profiles/r20_queue_lean.txt) */
       LSLAM_AB_GRID_CUBIC = 512,  /* grid sweep: the first pass of a throughput-bound batch that AUTO sent to the grid sweep keeps
                                      the cubic cell table instead of the x-subdivided one (each 0.6 m cell cut into S sub-cells
                                      along x, the axis the rows run along, so that a bounded probe's rows are clipped to
                                      2 rb + c / S instead of 2 rb + c; built once per map on first use, with its own
                                      cell-sorted points).  Same five neighbours; a rare near-tie point may change passes, which
                                      moves the last bits of the sums.  S: LSLAM_GRID_XSUB in the environment the context was
                                      made in (1: off; above 1 explicit LSLAM_SEARCH_GRID calls take the fine tables too -- for
                                      tests), default LSLAM_GRID_XSUB_DEFAULT of the build (profiles/r16_grid_xsub.txt) */
       LSLAM_AB_WIDE_NF_MARGIN = 16 /* a map without kd-trees: a point whose fifth and sixth distances are within 8 ulps of each
                                      other counts as undecidable too (as an exact tie does): the trees are built and the call
                                      repeated.  Off: such a pair is ordered by its exact fp32 distances -- nanoflann's order
                                      unless its own pruning bound (nanoflann.hpp:1485, two roundings per far step) rounds
                                      across the pair: not observed in 37 139 near-tie queries built to provoke it against the
                                      reference's nanoflann (tools/nanoflann_exactness.py).  On: ~1-2 % of a mapping node's
                                      frames build the trees after all (+2.2 ms each).  Where trees exist (batches, the headline)
                                      the margin is always on and wider (100 ulps): a refused point just takes the tree walk */ };

/* 5-NN search implementations (same answer, bit for bit):
 *   LANE    one query per lane, nanoflann's traversal with an explicit per-lane stack
 *   PACKET  one wavefront walks the tree once for its 64 (Morton-neighbouring) queries: nodes and leaves
 *           arrive by scalar loads, lanes test them against their own query (csrc/lslam_packet.hpp)
 *   GRID    no tree walk for most queries: a dense cell grid over the map (cells of lslam_opts.grid_cell metres), a probe of
 *           the 27 cells around the query, and a PROOF that the five smallest distances found are the five nearest map
 *           points with no tie among the six smallest (csrc/lslam_grid.hpp); a query the proof fails for -- a sparse
 *           neighbourhood, an exact tie -- is searched by LANE.  Whole-map trees only
 *   AUTO    the faster one on MI355X: LANE (the packet search trades the divergent gathers for about twice
 *           the vector ALU work and measured slower; DESIGN.md has the numbers) */
enum { LSLAM_SEARCH_AUTO = 0, LSLAM_SEARCH_LANE = 1, LSLAM_SEARCH_PACKET = 2, LSLAM_SEARCH_GRID = 3 };
/* Traversal-stack shape of the LANE search, ORed into a search mode (same answer, bit for bit -- the shapes hold the
 * same entries; only where they live differs):
 *   DEEP     all 32 levels of a lane's stack in LDS (two workgroups per CU): what a latency-bound single-scan launch takes
 *   SHALLOW  12 levels in LDS, deeper ones in an HBM overflow area (five wavefronts per SIMD): what a launch of more than
 *            2 048 wavefronts -- a batch, the bench -- takes
 *   AUTO     by the size of the launch
 * LSLAM_FORCE_STACK=deep|shallow|auto in the environment (read by lslam_ctx_create) overrides the bits.  The parity tests run every oracle
 * comparison through both shapes; lslam_debug_sweep_launches says which kernel really ran. */
enum { LSLAM_STACK_AUTO = 0, LSLAM_STACK_DEEP = 0x100, LSLAM_STACK_SHALLOW = 0x200 };
/* lslam_sweep_ex only, ORed into LSLAM_SEARCH_GRID: run the tap's sweep the way the production loop runs a LATER sweep of a
 * Gauss-Newton loop -- bounded by the acceptance gate and by what the previous sweep of the loop carried over per point (where
 * the point was, how far its fifth neighbour: the probe's rows and cells are clipped to that bound, the second pass's tree
 * search starts from it).  The carried state is the one the last lslam_scanmatch_run* on this resident scan left (run it
 * with search_mode LSLAM_SEARCH_GRID and max_iterations = k: the tap at the pose it returned is then sweep k + 1 of the
 * loop, kernel for kernel).  Beyond the gate (d2[4] >= 5) nothing is looked up by the reference (ScanMatch.cpp:102,120) and
 * idx_out / d2_out of such a point are not nanoflann's; flags and coefficients are the reference's for every point. */
/* LSLAM_SWEEP_FIRST: the loop's FIRST sweep, kernel for kernel -- bounded by the acceptance gate only, nothing carried. */
enum { LSLAM_SWEEP_CARRIED = 0x400, LSLAM_SWEEP_FIRST = 0x800 };

/* Per-call statistics (the counters the reference prints, ScanMatch.cpp:35-40,
 * 143,269, plus timing taps). */
typedef struct {
  int32_t status;          /* same value the call returned */
  int32_t iterations;      /* GN iterations whose 6x6 solve ran */
  int32_t n_line;          /* line_match_count of the last sweep */
  int32_t n_plane;         /* plane_match_count of the last sweep */
  int32_t n_rows;          /* laserCloudSelNum of the last sweep */
  int32_t degenerate;      /* isDegenerate (ScanMatch.cpp:222-233) */
  int32_t converged;       /* ScanMatch.cpp:257-260 */
  float delta_r, delta_t;  /* of the last solve (deg, cm) */
  double score, percent;   /* ScanMatch.cpp:265-268 (valid when converged && use_score) */
  int64_t point_residuals; /* (Nc+Ns) x sweeps executed on the device */
  int32_t sweeps;          /* sweep launches that did work (not early-exited) */
  int32_t sweep_launches;  /* sweep launches timed (profile=1) */
  float gpu_ms_total;      /* HIP events around the whole device-resident GN loop */
  float gpu_ms_sweep;      /* sum of sweep-kernel durations (profile=1), else 0 */
  double score2, percent2; /* ScanMatch.cpp:317-319 (opts.fine_score && converged && use_score, else 0) */
} lslam_stats;

typedef struct {
  uint64_t n_corner, n_surf;         /* map sizes */
  uint32_t nodes_corner, nodes_surf; /* kd-tree node counts */
  int32_t depth_corner, depth_surf;  /* kd-tree depths */
  float build_ms;                    /* tree build wall time inside lslam_map_set */
  float upload_ms;                   /* H2D copy time inside lslam_map_set */
  int32_t built_on_device;           /* always 1: the HIP builder is the only one */
  int32_t build_attempts;            /* node-slot array sizes tried (1: the first, 8n/3 slots, fitted) */
} lslam_map_info;

/* ---- lifecycle --------------------------------------------------------- */

/* Creates a context on HIP device `device` with its own stream.
 * Replaces: construction of a lidar_slam::ScanMatch member
 * (odometry/LaserMatcher.h _scan_match; pose_graph/loop_detector.hpp:269). */
int lslam_ctx_create(int device, lslam_ctx **out);
void lslam_ctx_destroy(lslam_ctx *ctx);
/* Last error text for this thread ("" if none). */
const char *lslam_last_error(void);
/* Fills opts with the reference defaults (ScanMatch.cpp:21-33) -- EVERY byte of the struct: call it before setting fields. */
void lslam_default_opts(lslam_opts *opts);
/* The structs of this ABI grow from release to release (lslam_opts: 72 -> 80 bytes in round 4).  A caller compiled against
 * another header would hand the library a struct of the wrong size: compare before the first call --
 *   assert(lslam_abi_version() == LSLAM_ABI_VERSION && lslam_sizeof_opts() == sizeof(lslam_opts));
 * (the C++ mirrors do, and refuse to start otherwise). */
/* 5 (round 5): no struct changed; new entry points (lslam_debug_grid_stats, lslam_debug_knn5_wide, lslam_debug_sort_pairs), new bits (LSLAM_SWEEP_FIRST /
 * _CARRIED, LSLAM_AB_WIDE_NF_MARGIN, the fit cache's bit -- since retired) -- a program built against this header needs a library that has them. */
/* 6 (round 6): no struct changed; new entry points (lslam_fset_*, lslam_extract_features_dev, lslam_odom_*, lslam_map_epoch). */
/* 7: no struct changed; new entry points (lslam_lmap_*: the sliding-window local map). */
/* still 7: no struct changed; new entry points (lslam_sreg_*: the registration node with the IMU de-skew branch). */
/* still 7: no struct changed; new entry points and structs of their own (lslam_loc_*: the localisation node). */
/* still 7: no struct changed; new entry points and a struct of their own (lslam_oreg_*: the registration node for organised clouds). */
/* still 7: no struct changed; new entry points and a struct of their own (lslam_kfs_*: the keyframe store). */
/* still 7: no struct changed; new entry points and structs of their own (lslam_sc_*: loop candidates by appearance). */
/* still 7: no struct changed; new entry points and an enum (lslam_pg_set_robust_kernels, _edge_robust, _robust_info, _kernel_from_name: robust kernels on pose-graph edges; lslam_pg_stream). */
/* still 7: no struct changed; new entry points and a struct of their own (lslam_match_information, lslam_keyframe_edge_information, lslam_sizeof_edge_info: the match Hessian of a pose-graph edge). */
/* still 7: no struct changed, no entry point gone; six LSLAM_AB_* names retired (bits 1, 2, 4, 8, 32, 128: refused from here on, see lslam_opts.ab_switches). */
/* still 7: no struct changed; new entry points and an enum (lslam_pg_set_priors, _num_priors, _prior_robust, lslam_g2o_read_priors: unary constraints on pose-graph vertices). */
/* still 7: no struct changed; new entry points and structs of their own (lslam_floor_*, lslam_debug_floor_hypotheses: floor detection; lslam_pg_set_plane_priors, _num_plane_priors, _plane_prior_robust, lslam_g2o_read_plane_priors: plane priors). */
/* still 7: no struct changed; new entry points and structs of their own (lslam_vis_*, lslam_debug_vis_votes: visibility votes over the keyframe store). */
/* still 7: no struct changed; new entry points and structs of their own (lslam_mapq_*: map quality, mean map entropy and mean plane variance; lslam_traj_*: trajectory evaluation). */
/* still 7: no struct changed; new entry points and structs of their own (lslam_occ_*, lslam_debug_occ_integrate: the 2D occupancy grid from the keyframe store). */
/* still 7: no struct changed; new entry points and structs of their own (lslam_pg_marginals, lslam_pg_relative_covariances: marginal covariances of pose-graph vertices). */
#define LSLAM_ABI_VERSION 7
int lslam_abi_version(void);
size_t lslam_sizeof_opts(void);
size_t lslam_sizeof_stats(void);

/* ---- map (reference clouds) -------------------------------------------- */

/* Uploads the reference corner/surf clouds and builds both kd-trees.
 * Replaces: kdtreeCorner.setInputCloud / kdtreeSurf.setInputCloud,
 * ScanMatch.cpp:68-76 (util/nanoflann_pcl.h:141-148 -> nanoflann.hpp:1270-1284).
 * The map stays resident and may be reused by any number of scan matches
 * (the reference rebuilds it on every call -- quirk Q4). */
int lslam_map_set(lslam_ctx *ctx, const void *corner, size_t n_corner, const void *surf,
                  size_t n_surf, size_t stride_bytes);
int lslam_map_info_get(const lslam_ctx *ctx, lslam_map_info *info);
/* Which map is resident: a number that changes whenever ANY entry point replaces or drops the context's map (lslam_map_set,
 * lslam_cubemap_set, lslam_fmap_surround_to_map / _to_cubemap, lslam_odometry_match_trees, lslam_icp_align, a failed tree build
 * ...), 0 while there is none.  A caller that skips an upload because "my clouds are resident" (ScanMatch::setReferenceEpoch,
 * include/lslam_scan_match.hpp) records it after its map set and compares before every reuse. */
uint64_t lslam_map_epoch(const lslam_ctx *ctx);

/* Deferred kd-trees.  on != 0: a map set from now on -- one that is already in HBM (lslam_fmap_surround_to_map: the mapping
 * node's per-frame map, LaserMatcher.cpp:303-331, where the reference rebuilds both trees every frame -- quirk Q4) or host
 * clouds (lslam_map_set: ScanMatch::scanMatchScan's, uploaded as usual) -- gets its cell grids at once (bounding box, cell
 * counts, one scan, placement: about a sixth of a tree build) and its kd-trees only when something needs them.  A scan match of one small scan against such a map runs on the grids alone -- the 27-cell probe with
 * its proof, and for the points it cannot prove one wavefront each over every cell within their bound -- and gives nanoflann's
 * neighbours exactly as the tree search does; the one case the grids cannot decide, an exact distance tie among a point's six
 * nearest, makes the call build the trees and run again through them (with lslam_opts.ab_switches & LSLAM_AB_WIDE_NF_MARGIN a
 * fifth / sixth pair within 8 ulps does too: see there for what that guards against and what it costs).  Every other entry point that touches the trees (the
 * taps, LSLAM_SEARCH_LANE / _PACKET, batches, the sharded loop, lslam_icp_align, ...) builds them first.  Results do not
 * depend on the setting.  lslam_map_info reports depth 0 / 0 nodes while the trees are pending. */
int lslam_map_defer_trees(lslam_ctx *ctx, int32_t on);

/* Variant C -- the map as FeatureMap keeps it (util/FeatureMap.h): a grid of dims[0] x dims[1]
 * x dims[2] cubes of cube_size metres (50), cube of a point = round(p/cube_size) + origin
 * (worldToCube, :475-487); every cube gets its own kd-tree (as _kdtreeCorner/_kdtreeSurf,
 * :71-72,438,453).  After this call the scan-match entry points behave like
 * FeatureMap::scanMatchScan (:490-691): a scan point is searched only in the tree of the cube
 * it falls into, cubes with fewer than 5 points are skipped, and there is no
 * "reference cloud too few" guard.  The caller passes the reference's settings through
 * lslam_opts (max_iterations 10, thresholds 0.05/0.05, use_score 0).  lslam_map_set
 * switches back to the whole-map trees of ScanMatch::scanMatchScan. */
int lslam_cubemap_set(lslam_ctx *ctx, const void *corner, size_t n_corner, const void *surf,
                      size_t n_surf, size_t stride_bytes, float cube_size, const int32_t origin[3],
                      const int32_t dims[3]);

/* ---- scan (query clouds) ------------------------------------------------ */

/* Uploads the scan's corner/surf feature clouds (CornerCloud / SurfCloud of
 * ScanMatch.cpp:53-54) so that lslam_scanmatch_run works on HBM-resident data. */
int lslam_scan_set(lslam_ctx *ctx, const void *corner, size_t n_corner, const void *surf,
                   size_t n_surf, size_t stride_bytes);

/* Batch form: n_scans independent scans (e.g. keyframes) made resident together; they
 * are matched against the same resident map by ONE sequence of kernel launches, which
 * is what fills a 256-CU GPU (one 64-ring scan is only ~1800 wavefronts).
 * Replaces the per-keyframe loop of Graph::getFinalFeatureMap (pose_graph/graph.cpp:171-197)
 * and the per-candidate loop of LoopDetector::matching_nearest
 * (pose_graph/loop_detector.hpp:166-226). */
int lslam_scan_set_batch(lslam_ctx *ctx, int32_t n_scans, const void *const *corner,
                         const size_t *n_corner, const void *const *surf, const size_t *n_surf,
                         size_t stride_bytes);

/* ---- Gauss-Newton scan match ------------------------------------------- */

/* The GN loop of ScanMatch::scanMatchScan(..., Twist&), ScanMatch.cpp:78-347,
 * on the resident map and scan.  pose is in/out and is always written back
 * except for LSLAM_TOO_FEW_REF and errors (ScanMatch.cpp:324,331,338,343). */
int lslam_scanmatch_run(lslam_ctx *ctx, float pose[6], const lslam_opts *opts, lslam_stats *stats);

/* The same loop for every resident scan of a batch, each with its own pose, iteration
 * count and convergence: poses[n_scans*6] in/out, stats[n_scans] (may be NULL).
 * gpu_ms_* in every stats entry are those of the whole batch.  Returns LSLAM_OK if
 * every scan returned true, else the first non-OK outcome (errors are negative). */
int lslam_scanmatch_run_batch(lslam_ctx *ctx, int32_t n_scans, float *poses,
                              const lslam_opts *opts, lslam_stats *stats);

/* = lslam_scan_set + lslam_scanmatch_run.  Replaces scanMatchScan against a map
 * that is already resident (the FeatureMap::scanMatchScan usage, util/FeatureMap.h:490-691). */
int lslam_scanmatch_scan(lslam_ctx *ctx, const void *corner, size_t n_corner, const void *surf,
                         size_t n_surf, size_t stride_bytes, float pose[6],
                         const lslam_opts *opts, lslam_stats *stats);

/* = lslam_map_set + lslam_scan_set + lslam_scanmatch_run: the exact drop-in for
 * bool ScanMatch::scanMatchScan(refCorner, refSurf, Corner, Surf, Twist&),
 * ScanMatch.cpp:51-347, including the per-call tree rebuild. */
int lslam_scanmatch_full(lslam_ctx *ctx, const void *ref_corner, size_t n_ref_corner,
                         const void *ref_surf, size_t n_ref_surf, size_t ref_stride_bytes,
                         const void *corner, size_t n_corner, const void *surf, size_t n_surf,
                         size_t stride_bytes, float pose[6], const lslam_opts *opts,
                         lslam_stats *stats);

/* Variant B -- scan-to-scan odometry: void LaserOdometry::scanMatch()
 * (odometry/LaserOdometry.cpp:328-647): nearest neighbour + ring-window correspondences
 * refreshed every 5th iteration, motion-interpolated de-skew (transformToStart, :135-142),
 * weights from iteration 5 on, b = -0.05 d, eigenvalue threshold 10, NaN reset.
 * Clouds are {x,y,z,intensity} (intensity = ring id + relative time; at byte 16 for
 * stride >= 32 as in pcl::PointXYZI, else at byte 12); last_corner / last_surf
 * (_lastCornerCloud / _lastSurfaceCloud) must be in scan order.  pose is the persistent
 * `_transform` (in/out).  Defaults of the reference: 25 iterations, 0.1 / 0.1 (:24-25).
 * Returns LSLAM_OK when the loop converged (:642-644), LSLAM_NOT_CONVERGED otherwise,
 * LSLAM_TOO_FEW_REF when the guard of :337 fails. */
int lslam_odometry_match(lslam_ctx *ctx, const void *last_corner, size_t n_last_corner,
                         const void *last_surf, size_t n_last_surf, const void *sharp, size_t n_sharp,
                         const void *flat, size_t n_flat, size_t stride_bytes, float pose[6],
                         int32_t max_iterations, float delta_t_abort, float delta_r_abort,
                         lslam_stats *stats);

/* The same match with nearestKSearch answered by kd-trees of the two last clouds (built in the call) and one launch per step:
 * the implementation lslam_odometry_match had before the hashed grids of csrc/lslam_odom.hip.  It is what a sweep with an exact
 * distance tie is redone through (nanoflann's visit order decides there) and the A/B partner of the grid path: same result, bit
 * for bit, on tie-free clouds (tests/test_gpu_odom.py).  LSLAM_ODOM_TREES=1 in the environment routes lslam_odometry_match here. */
int lslam_odometry_match_trees(lslam_ctx *ctx, const void *last_corner, size_t n_last_corner,
                               const void *last_surf, size_t n_last_surf, const void *sharp, size_t n_sharp,
                               const void *flat, size_t n_flat, size_t stride_bytes, float pose[6],
                               int32_t max_iterations, float delta_t_abort, float delta_r_abort,
                               lslam_stats *stats);

/* LaserOdometry::transformToEnd (odometry/LaserOdometry.cpp:156-168): every point of a host
 * cloud ({x,y,z} + intensity = ring + relTime at byte 12 of 16-byte points, byte 16 of PointXYZI)
 * is de-skewed to the sweep start and moved to the sweep end, in place. */
int lslam_transform_to_end(lslam_ctx *ctx, void *cloud, size_t n, size_t stride_bytes, const float pose[6]);

/* Isometry3f <-> Twist conversion used by the Isometry overloads
 * (ScanMatch.cpp:349-360; util/transform_utils.h:308-323,54-60).  T is a
 * row-major 4x4. Host-side helpers, no device work. */
void lslam_isometry_to_pose(const float T[16], float pose[6]);
/* The odometry-prior merge that precedes the scan match in the mapping node,
 * transformAssociate(Lold, Lnew, Wold, Wnew): Wnew = Wold * Lold^-1 * Lnew
 * (util/transform_utils.h:502-507, called from LaserMatcher::transformMerge,
 * odometry/LaserMatcher.cpp:333-340).  Row-major 4x4 matrices, host helper. */
void lslam_transform_associate(const float Lold[16], const float Lnew[16], const float Wold[16],
                               float Wnew[16]);
void lslam_pose_to_isometry(const float pose[6], float T[16]);

/* ---- parity / debug taps ------------------------------------------------ */

/* Exact 5-NN of nq query points (already in the map frame) in the resident
 * corner (which_map=0) or surf (1) tree.  Replaces
 * KdTreeFLANN::nearestKSearch(p, 5, idx, d2), util/nanoflann_pcl.h:150-162.
 * idx_out[nq*5] are indices into the cloud passed to lslam_map_set (int32,
 * bit-exact with nanoflann), d2_out[nq*5] squared distances ascending. */
int lslam_knn5(lslam_ctx *ctx, int which_map, const void *queries, size_t nq,
               size_t stride_bytes, int32_t *idx_out, float *d2_out);

/* One sweep (ScanMatch.cpp:97-204) over the resident scan at a fixed pose.
 * Any output may be NULL.  Point order: corner queries then surf queries.
 *   idx_out[N*5], d2_out[N*5]  kNN of the transformed point
 *   coeff_out[N*4]             (w*dir|w*n, w*d) -- coeffSel
 *   flags_out[N]               bit0 d2[4]<5, bit1 fit found, bit2 row kept
 *   sums_out[30]               21 upper-tri A^T A (row-major) | 6 A^T b |
 *                              n_rows | n_line+n_plane | score */
int lslam_sweep(lslam_ctx *ctx, const float pose[6], int32_t jtj_mode, int32_t *idx_out,
                float *d2_out, float *coeff_out, uint8_t *flags_out, float *sums_out);

/* The two taps above with the search implementation chosen explicitly (LSLAM_SEARCH_*); n_ties (may be
 * NULL) receives the number of queries whose answer needed nanoflann's visit order (exact distance ties). */
int lslam_knn5_ex(lslam_ctx *ctx, int which_map, const void *queries, size_t nq, size_t stride_bytes,
                  int32_t search_mode, int32_t *idx_out, float *d2_out, int32_t *n_ties);
int lslam_sweep_ex(lslam_ctx *ctx, const float pose[6], int32_t jtj_mode, int32_t search_mode, int32_t *idx_out,
                   float *d2_out, float *coeff_out, uint8_t *flags_out, float *sums_out);
/* Parity tap of the search a map WITHOUT kd-trees is matched through (lslam_map_defer_trees): the wide probe -- one wavefront
 * per query over every cell of the resident cell grid within the sqrt(5) m acceptance gate -- for nq queries in the map
 * frame.  Builds no tree.  idx_out[nq*5] / d2_out[nq*5] as lslam_knn5 (-1 / FLT_MAX where the gate holds fewer than five
 * points); undecided_out[nq] = 1 where the grids cannot prove nanoflann's answer (an exact distance tie among the six nearest;
 * with nf_margin != 0 also a fifth / sixth pair within 8 ulps, LSLAM_AB_WIDE_NF_MARGIN): a scan match would build the trees. */
int lslam_debug_knn5_wide(lslam_ctx *ctx, int which_map, const void *queries, size_t nq, size_t stride_bytes, int32_t nf_margin,
                          int32_t *idx_out, float *d2_out, uint8_t *undecided_out);

/* Parity tap of the sort the per-frame map maintenance runs on (csrc/lslam_sort.hip; n <= 131 072): keys_out / values_out =
 * the n (key, value) pairs ascending by key, equal keys in ascending order of their values (distinct among equal keys: with
 * values = input positions a stable sort by key -- pcl::VoxelGrid's index order, the Morton order of the resident scans). */
int lslam_debug_sort_pairs(lslam_ctx *ctx, const uint64_t *keys, const uint32_t *values, size_t n, uint64_t *keys_out,
                           uint32_t *values_out);

/* Parity taps of the coarse alignment (lslam_icp_align, csrc/lslam_icp.hip).
 *
 * lslam_debug_icp_step: ONE correspondence pass of the alignment's loop at the transform T (row-major 4x4, source -> target),
 * through the code the loop runs: the target's kd-tree is built as lslam_icp_align builds it (the context's resident map is
 * replaced), the kernel is launched with the loop's arguments plus two tap pointers, and the fit is the loop's.  Clouds and
 * stride_bytes as lslam_icp_align takes them; max_correspondence_distance <= 0: no gate.  n_target == 0 is refused.
 *   idx_out[n_source]  the target point each source point was paired with (index into `target`), -1: beyond the gate
 *   d2_out[n_source]   fp32 squared distance of the transformed source point from its nearest target point (gated out or not)
 *   sums_out[18]       n | sum d2 | sum s (3) | sum t (3) | sum s t^T (9, row-major) | 0, s = the transformed source point
 * idx_out, d2_out and sums_out may be NULL.  out->fitted = 1 when n >= 3: R, t, W and det_sign are then what the loop would
 * compose into T (lslam_debug_icp_fit of the sums). */
typedef struct lslam_icp_step {
  double R[9], t[3], W[3]; /* the increment (row-major R) and the singular values of the cross-covariance, descending */
  int32_t det_sign;        /* sign of det(V U^T): -1 where the reflection fix was applied */
  int32_t fitted;          /* 0: fewer than 3 correspondences, the loop would stop (R, t, W are zero) */
  int32_t overflow_stack;  /* 1: icp_corr_kernel<true> ran (target tree deeper than the LDS stack), 0: icp_corr_kernel<false> */
  int32_t blocks;          /* blocks of 128 source points launched */
} lslam_icp_step;
int lslam_debug_icp_step(lslam_ctx *ctx, const void *target, size_t n_target, const void *source, size_t n_source,
                         size_t stride_bytes, const float T[16], double max_correspondence_distance, int32_t *idx_out,
                         float *d2_out, double sums_out[18], lslam_icp_step *out);
/* The rigid fit of the loop on 18 sums laid out as sums_out above (sums[0] >= 1): centroids, cross-covariance
 * H = sum s t^T - n cs ct^T, its SVD H = U diag(W) V^T with orthonormal U and V for every H (H = 0 included), R = V diag(1, 1,
 * det(V U^T)) U^T, t = ct - R cs.  Host code: needs no context and no device.  det_sign may be NULL. */
int lslam_debug_icp_fit(const double sums[18], double R[9], double t[3], double W[3], int32_t *det_sign);

/* The names SURVEY.md 8(b) gave these entry points before they were built, kept as exported aliases:
 *   lslam_residuals        = lslam_sweep with the MFMA contraction: coeff_out[N*4], valid_out[N] (the flag bits of
 *                            lslam_sweep), JtJ27_out[27] = the 21 upper-triangular A^T A sums then the 6 A^T b sums
 *   lslam_scanmatch_batch  = lslam_scanmatch_run_batch
 *   lslam_posegraph_optimize (further down) = lslam_pg_create + lslam_pg_optimize + lslam_pg_get_poses + destroy */
int lslam_residuals(lslam_ctx *ctx, const float pose[6], float *coeff_out, uint8_t *valid_out, float *JtJ27_out);
int lslam_scanmatch_batch(lslam_ctx *ctx, int32_t n_problems, float *poses, const lslam_opts *opts, lslam_stats *stats);

/* One solve/update step (ScanMatch.cpp:206-260) run by the device solve kernel
 * on caller-provided normal equations.  matP/degenerate are in/out state. */
int lslam_gn_step(lslam_ctx *ctx, const float AtA[36], const float Atb[6], int32_t iter,
                  float pose[6], float matP[36], int32_t *degenerate, float delta_r_abort,
                  float delta_t_abort, float x_out[6], float *delta_r, float *delta_t,
                  int32_t *converged);

/* ---- map maintenance ----------------------------------------
 * Replaces lidar_slam::FeatureMap<PointXYZI> (util/FeatureMap.h) for the steps either side of
 * the scan match: the cube grid, addFeatureCloud + per-cube pcl::VoxelGrid, the active area and
 * the surround concatenation -- all resident in HBM, so that the map never returns to the host
 * between frames.  Clouds handed in are {x,y,z} at offset 0 with the intensity at byte 12 of
 * 16-byte points or byte 16 of pcl::PointXYZI (32 bytes); clouds handed out are packed
 * {x,y,z,intensity}.  One in-flight call per ctx, like everything else on a ctx. */
typedef struct lslam_fmap lslam_fmap;

/* FeatureMap(cubeWidth, cubeHeight, cubeDepth), FeatureMap.h:55-68 (origin = round((size-1)/2),
 * cube 50 m, valid distance 150 m, leaves 0.2/0.2/0.6). */
int lslam_fmap_create(lslam_ctx *ctx, int32_t cube_width, int32_t cube_height, int32_t cube_depth,
                      lslam_fmap **out);
void lslam_fmap_destroy(lslam_fmap *fm);
int lslam_fmap_setup_filter_size(lslam_fmap *fm, float corner, float surf, float map);     /* :72-76 */
int lslam_fmap_setup_world_origin(lslam_fmap *fm, int32_t ox, int32_t oy, int32_t oz);     /* :78-83 */
int lslam_fmap_setup_world_cube_size(lslam_fmap *fm, float size);                          /* :85-87 */
int lslam_fmap_setup_lidar_valid_distance(lslam_fmap *fm, float dist);                     /* :89-91 */
/* update(sensorPose), FeatureMap.h:232-254: clamp the sensor's cube 3 cubes inside the grid,
 * shift() the cube contents (with the reference's swap-chain behaviour, :353-377), move the
 * origin, recompute the active area (:307-352). */
int lslam_fmap_update(lslam_fmap *fm, const float sensor_xyz[3]);
/* addFeatureCloud(corner, surf, tf), FeatureMap.h:218-230: transform by the row-major 4x4 T, push
 * every point into its cube (worldToCube, :475-487; points outside the grid are dropped), then
 * downsizeValidCloud (:288-306): VoxelGrid every cube of the active area. */
int lslam_fmap_add_feature_cloud(lslam_fmap *fm, const void *corner, size_t n_corner, const void *surf,
                                 size_t n_surf, size_t stride_bytes, const float T[16]);
/* The same without the wait at its end, for a node whose sweep ends with addFeatureCloud (LaserMapping::process,
 * LaserMapping.cpp:349-353): the clouds are copied out of the caller's memory and everything is enqueued; the rebuild is
 * waited for and committed at the head of the NEXT call on this map, whichever it is (or by lslam_fmap_wait), so the node's
 * next sweep is being prepared while the map is rebuilt.  An error of the deferred half is that next call's error. */
int lslam_fmap_add_feature_cloud_begin(lslam_fmap *fm, const void *corner, size_t n_corner, const void *surf,
                                       size_t n_surf, size_t stride_bytes, const float T[16]);
int lslam_fmap_wait(lslam_fmap *fm);
/* getSurroundFeature, FeatureMap.h:256-265: the active cubes' clouds, concatenated in
 * _cubeValidInd order.  counts first, then the copy to the host ... */
int lslam_fmap_surround_counts(lslam_fmap *fm, size_t *n_corner, size_t *n_surf);
int lslam_fmap_get_surround(lslam_fmap *fm, float *corner_xyzi, size_t cap_corner, float *surf_xyzi,
                            size_t cap_surf);
/* ... or, without leaving HBM: the surround becomes the ctx's map (what
 * LaserMatcher::prepareFeatureSurround + ScanMatch.cpp:68-76 do through the host), kd-trees
 * built on the device. */
int lslam_fmap_surround_to_map(lslam_fmap *fm);
/* The same, handing back the surround's sizes it reads anyway (getSurroundFeature's two clouds): a caller that only wants to
 * know whether there is anything to match against (LaserMatcher.cpp:303-331) need not wait for lslam_fmap_surround_counts first. */
int lslam_fmap_surround_to_map_counts(lslam_fmap *fm, size_t *n_corner, size_t *n_surf);
/* ... or as a variant-C map: one kd-tree per cube of the active area (cubes with fewer than 5
 * points skipped, FeatureMap.h:524,546), all built in one go on the device; scan points are then
 * matched against the tree of the cube they fall into (FeatureMap::scanMatchScan, :490-691). */
int lslam_fmap_to_cubemap(lslam_fmap *fm);
/* The per-cube trees persist between calls: lslam_fmap_to_cubemap rebuilds only the trees of cubes whose cloud changed
 * since their tree was built (addFeatureCloud marks the cubes that received points; shifts and loads mark all).
 * Counts of the last call: trees built in it / trees kept from earlier calls. */
int lslam_fmap_cubemap_stats(lslam_fmap *fm, int64_t *trees_built, int64_t *trees_reused);
/* How lslam_fmap_add_feature_cloud's rebuilds of the point arrays went so far (per feature type and call).  The current points
 * are an earlier rebuild's output, hence in (cube, voxel) key order: only the new points are sorted and merged in (`merged`).
 * The order is checked on the device; when it does not hold -- a cube that has just become active gets voxel keys it did not
 * have, a centroid can round onto a voxel wall -- the whole array is sorted as before (`resorted`).  Same arrays either way. */
int lslam_fmap_rebuild_stats(lslam_fmap *fm, int64_t *merged, int64_t *resorted);
/* Forget the cached trees (the next lslam_fmap_to_cubemap rebuilds the whole active area). */
int lslam_fmap_cubemap_invalidate(lslam_fmap *fm);
/* getFullMap, FeatureMap.h:267-286: per cube, VoxelGrid(map leaf) of corner then surf. */
int lslam_fmap_get_full_map(lslam_fmap *fm, float *out_xyzi, size_t cap, size_t *n_out);
/* saveCloudToFiles / loadCloudFromFiles, FeatureMap.h:378-462: one binary PCD (fields x y z
 * intensity) per non-empty (cube, type) named <count>.pcd and index.txt with lines
 * "count type i j k size"; loading runs every loaded cube through its type's VoxelGrid and
 * replaces that cube's content.  ascii and binary PCDs are read, binary_compressed is not. */
int lslam_fmap_save(lslam_fmap *fm, const char *directory);
int lslam_fmap_load(lslam_fmap *fm, const char *directory);
/* introspection: grid origin, _cubeValidInd, points held per type; any output may be NULL */
int lslam_fmap_info(lslam_fmap *fm, int32_t origin[3], int32_t *n_valid, int32_t *valid_out, size_t cap,
                    size_t *n_corner_total, size_t *n_surf_total);
/* ---- sliding-window local map (io_module/LocalFeatureMap.h, the container of odometry/LaserMappingLocal.cpp) ----------------
 * The frames of the last `queue distance` metres of path, resident in HBM: addDataFrame (FrameUpdater's path length, push,
 * clean() with its erase of n + 1 frames when n have fallen behind) and getSurroundFeature (the frames' clouds concatenated in
 * queue order, pcl::VoxelGrid with leaf 0.2 over the corners and 0.4 over the surfaces), whose result becomes the ctx's map
 * without leaving the device.  Point layouts as for lslam_fmap.  One in-flight call per ctx.
 * THE ONE DIFFERENCE from the reference: its queue grows without bound (a sensor that stands still never advances the path
 * length, so nothing is erased); device memory cannot.  The container is created with limits, and an add whose result would
 * exceed one is refused with LSLAM_ERR_INVALID (the message says which) and changes nothing.  The limits apply to the window
 * as it is after the add's clean(). */
typedef struct lslam_lmap lslam_lmap;
/* How the filtered surround is produced (same bits either way; 0 = the default, which is the measured winner: DESIGN). */
#define LSLAM_LMAP_REFILTER 1      /* gather the window and sort + filter all of it, every sweep */
#define LSLAM_LMAP_KEY_ORDERED 2   /* keep the window in voxel-key order: sort the new points only, merge them in */
#define LSLAM_LMAP_ALWAYS_RESORT 4 /* key-ordered, but the ordered array is rebuilt from the ring every sweep (its fall-back, for tests) */
/* max_points_per_type: 0 = 2^20 (30 m of path at 0.1 m per sweep: 300 VLP-16 frames of ~1000 corner / ~2500 surface points
 * after the scan filter), at most 2^24; max_frames: 0 = 4096.  The memory is taken here: 112 bytes per point and type (the key-ordered
 * filter's sort scratch, up to ~36 bytes per live point, grows with the window); all of it is returned by lslam_lmap_destroy. */
int lslam_lmap_create(lslam_ctx *ctx, size_t max_points_per_type, int32_t max_frames, int32_t flags, lslam_lmap **out);
void lslam_lmap_destroy(lslam_lmap *lm);
/* queue_distance_threshold (LocalFeatureMap.h; default 30.0 m); must be positive. */
int lslam_lmap_setup_queue_distance(lslam_lmap *lm, double metres);
/* The leaves of the two surround filters.  The reference fixes them in its constructor (0.2 / 0.4: the defaults) and has no
 * setter; this one is refused once a frame has been added (the key-ordered window is sorted by them) until lslam_lmap_clear. */
int lslam_lmap_setup_filter_size(lslam_lmap *lm, float corner, float surf);
/* featureMapUpdate + addDataFrame (LaserMappingLocal.cpp:68-83, LocalFeatureMap.h:62-82): the clouds are transformed by the
 * row-major 4x4 T_map (p' = R p + t in fp32, intensity kept), FrameUpdater::update(T_map cast to double) advances the path
 * length, the frame is pushed and clean() runs.  Both clouds go up behind one wait. */
int lslam_lmap_add_data_frame(lslam_lmap *lm, const void *corner, size_t n_corner, const void *surf, size_t n_surf,
                              size_t stride_bytes, const float T_map[16]);
/* The same for clouds that are in the ctx's device memory already, packed {x, y, z, intensity} (16 bytes per point). */
int lslam_lmap_add_data_frame_device(lslam_lmap *lm, const void *d_corner, size_t n_corner, const void *d_surf, size_t n_surf,
                                     const float T_map[16]);
/* getSurroundFeature (LocalFeatureMap.h:84-99) + ScanMatch's map set: the filtered window becomes the ctx's map (cell grids
 * only under lslam_map_defer_trees); one wait for both types.  An empty window gives the empty map.  -> the two clouds' sizes */
int lslam_lmap_surround_to_map_counts(lslam_lmap *lm, size_t *n_corner, size_t *n_surf);
/* getSurroundFeature to the host: bit for bit lslam_voxel_grid over the concatenation of the window.  A null buffer: its
 * count only. */
int lslam_lmap_get_surround(lslam_lmap *lm, float *corner_xyzi, size_t cap_corner, size_t *n_corner, float *surf_xyzi,
                            size_t cap_surf, size_t *n_surf);
/* frames in the queue, FrameUpdater's accum_distance, points held per type, frames erased so far; any output may be NULL */
int lslam_lmap_info(lslam_lmap *lm, int32_t *n_frames, double *accum_distance, size_t live_points[2], int64_t *frames_evicted);
/* Debug tap: the queue as it is, oldest frame first -- per frame its accum_distance and its {corner, surf} point counts
 * (counts[2 k], counts[2 k + 1]), and the frames' transformed points back to back per type.  Any output may be NULL. */
int lslam_lmap_get_frames(lslam_lmap *lm, int32_t cap_frames, int32_t *n_frames, double *accum, int32_t *counts,
                          float *corner_xyzi, size_t cap_corner, float *surf_xyzi, size_t cap_surf);
/* How the surrounds were produced so far, per type and sweep: new points merged into the ordered array / ordered array sorted
 * as a whole / window gathered and re-filtered. */
int lslam_lmap_stats(lslam_lmap *lm, int64_t *merged, int64_t *resorted, int64_t *refiltered);
/* Back to the state after create: no frames, path length 0, FrameUpdater's first-frame rule armed (limits, leaves and queue
 * distance stay). */
int lslam_lmap_clear(lslam_lmap *lm);

/* ---- keyframe store (pose_graph/keyframe.h's clouds; pose_graph::Graph, LoopDetector) --------------------------------------
 * The corner and surface clouds of the pose graph's keyframes, resident in HBM, and the steps of the pose-graph node that read
 * them there: a keyframe is uploaded once (lslam_kfs_add) and every later use -- the loop detector's coarse and fine alignment,
 * Graph::getFinalFeatureMap's filter, match and addFeatureCloud -- names it by its id and moves no point over PCIe in either
 * direction.  Points are packed {x, y, z, intensity}, 16 bytes; ids are 0, 1, 2, ... in order of insertion (the order of the
 * reference's `keyframes` vector).  An empty cloud (0 points) is a legal keyframe cloud.  One in-flight call per ctx.
 * Memory is slabs of slab_points points (16 bytes each) taken as the store grows.  A cloud never straddles a slab, a cloud
 * larger than a slab gets a slab of its own, and slabs are never moved: a device pointer handed out by lslam_kfs_view stays
 * valid until lslam_kfs_clear / lslam_kfs_destroy, and growing the store copies nothing.
 * As for lslam_lmap_*, the reference's container grows without bound and device memory cannot: the store has limits, and an
 * add that would exceed one is refused with LSLAM_ERR_INVALID (the message names the limit) and changes nothing.
 * LIFETIME: the rule of every per-ctx object (lslam_fmap, lslam_lmap, ...): lslam_ctx_destroy waits for the ctx's streams and
 * frees what the ctx owns, NOT the store; a store that outlives its ctx keeps its memory, refuses every call with
 * LSLAM_ERR_INVALID ("its ctx was destroyed") and is freed by lslam_kfs_destroy, which is valid before and after. */
typedef struct lslam_kfs lslam_kfs;
typedef struct lslam_kfs_stats {
  int64_t n_keyframes;
  uint64_t n_points[2];             /* corner, surf points held */
  int64_t n_slabs;
  uint64_t bytes_held;              /* device memory of the slabs */
  uint64_t cloud_bytes_uploaded;    /* point data this store's entry points moved host -> device (lslam_kfs_add) ... */
  uint64_t cloud_bytes_downloaded;  /* ... and device -> host (lslam_kfs_get, the debug tap), since creation */
} lslam_kfs_stats;
/* max_points_per_type: 0 = 2^26 (1 GiB per type), at most 2^30; max_keyframes: 0 = 65536; slab_points: 0 = 2^20 (16 MiB). */
int lslam_kfs_create(lslam_ctx *ctx, size_t max_points_per_type, int32_t max_keyframes, size_t slab_points, lslam_kfs **out);
void lslam_kfs_destroy(lslam_kfs *kfs);
/* Empties the store and frees its slabs (pointers handed out become invalid); ids start at 0 again.  Limits and byte counters stay. */
int lslam_kfs_clear(lslam_kfs *kfs);
/* A new keyframe from host clouds (stride_bytes >= 16: {x, y, z} at 0, the intensity at byte 12 of a 16-byte point, at byte 16
 * of a longer one, as pcl::PointXYZI keeps it); both clouds go up behind one wait.  -> *id */
int lslam_kfs_add(lslam_kfs *kfs, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                  int32_t *id);
/* The same for clouds that are in the ctx's device memory already, packed (lslam_odom_last_view's, a torch tensor's): copied
 * device to device, waited for -- the caller's buffers are free when the call returns. */
int lslam_kfs_add_device(lslam_kfs *kfs, const void *d_corner, size_t n_corner, const void *d_surf, size_t n_surf, int32_t *id);
int lslam_kfs_counts(lslam_kfs *kfs, int32_t id, size_t *n_corner, size_t *n_surf);
/* A cloud back on the host; which: 0 corner, 1 surf.  out_xyzi NULL: the count only. */
int lslam_kfs_get(lslam_kfs *kfs, int32_t id, int32_t which, float *out_xyzi, size_t cap, size_t *n_out);
/* The clouds where they are (device pointers, NULL for an empty cloud); any output may be NULL. */
int lslam_kfs_view(lslam_kfs *kfs, int32_t id, const float **d_corner, size_t *n_corner, const float **d_surf, size_t *n_surf);
int lslam_kfs_info(lslam_kfs *kfs, lslam_kfs_stats *stats);
/* Debug tap of the loop detector's reference clouds (loop_detector.hpp:166-200), downloaded: candidate ids[0]'s clouds as
 * they are (bit for bit), those of ids[1 .. n_cand-1] transformed by the row-major 4x4 rel_T[k] -- (estimate_0^-1 *
 * estimate_k).cast<float>(); rel_T[0] is not read -- as pcl::transformPointCloud does (x' = ((T0 x + T1 y) + T2 z) + T3 in
 * fp32, no FMA) and appended in candidate order.  1 <= n_cand <= 6; an id may repeat.  A NULL buffer: its count only. */
int lslam_kfs_debug_local_clouds(lslam_kfs *kfs, int32_t n_cand, const int32_t *ids, const float *rel_T, float *corner_out,
                                 size_t cap_corner, size_t *n_corner, float *surf_out, size_t cap_surf, size_t *n_surf);
/* LoopDetector::matching_nearest behind its gating (loop_detector.hpp:166-255), on the device: the candidates' local clouds
 * (above); stop if the surface one is empty; lslam_icp_align (transformation epsilon 0, no correspondence gate) of keyframe
 * new_id's surface cloud onto it from `guess`; stop if it did not converge; ScanMatch::scanMatchLocal -- lslam_voxel_grid
 * with leaf 0.2 / 0.4 / 0.2 / 0.4 over the local corner, local surface, new corner, new surface clouds, then
 * lslam_scanmatch_full -- from the ICP's result.  Same kernels in the same order as those calls: same bits.
 * *stage says where the call ended; guess holds the ICP's result from LSLAM_KFS_ICP_REJECTED on and the scan match's pose
 * (lslam_pose_to_isometry of it; where the filtered reference was too small for a match, of the ICP's result as a twist: what
 * ScanMatch::scanMatchLocal's mirrors hand back then) from LSLAM_KFS_MATCH_FAILED on.  fitness / icp_iterations: the ICP's; stats: the scan match's.  The ctx's map and resident
 * scan belong to the call afterwards.  Returns LSLAM_OK whatever the stage, < 0 on an error. */
#define LSLAM_KFS_EMPTY_REFERENCE 0
#define LSLAM_KFS_ICP_REJECTED 1
#define LSLAM_KFS_MATCH_FAILED 2
#define LSLAM_KFS_LOOP_ACCEPTED 3
int lslam_kfs_loop_match(lslam_kfs *kfs, int32_t n_cand, const int32_t *ids, const float *rel_T, int32_t new_id, float guess[16],
                         int32_t icp_max_iterations, const lslam_opts *opts, int32_t *stage, double *fitness,
                         int32_t *icp_iterations, lslam_stats *stats);
/* Graph::getFinalFeatureMap's match of one keyframe (graph.cpp:171-185): the keyframe's clouds through lslam_voxel_grid with
 * the two leaves, on the device; they become the ctx's resident scan and are matched against the resident map.  Return codes
 * and the pose write-back rule of lslam_scanmatch_scan. */
int lslam_kfs_scanmatch(lslam_kfs *kfs, int32_t id, float leaf_corner, float leaf_surf, float pose[6], const lslam_opts *opts,
                        lslam_stats *stats);
/* lslam_fmap_add_feature_cloud with the keyframe's clouds taken from the store (fm: a feature map of the store's ctx). */
int lslam_kfs_add_to_fmap(lslam_kfs *kfs, int32_t id, lslam_fmap *fm, const float T[16]);

/* ---- floor detection: the ground plane of a cloud, found on the device --------------------------------------------------------
 * The reference shows the intent and stops there: pose_graph/solver_g2o.h:61-65 has add_plane_node commented out, :92 a
 * commented floor_plane_node, :42 includes g2o's plane types, and graph.cpp:321 speaks of "floor coeffs in the queues" -- nothing
 * there detects a floor.  The module is modelled on hdl_graph_slam, whose floor detector is a height clip and a PCL RANSAC.
 * Neither hdl_graph_slam nor PCL is under the reference, so PARITY IS UNPINNED like the rest of the pose-graph node; the
 * semantics below are this project's own, stated completely, so that an independent reference reproduces every integer
 * decision exactly.  All fp32 expressions are evaluated as written, without FMA contraction (the convention of
 * lslam_kfs_debug_local_clouds).  u is `up` normalised in fp64; where fp32 is named, u rounded to fp32.
 *  1 CANDIDATES  h = ((ux x + uy y) + uz z) in fp32.  Point k is a candidate iff x, y, z are finite,
 *    -(sensor_height + height_clip_range) <= h <= -(sensor_height - height_clip_range) (the bounds in fp32) and, with
 *    max_range > 0, (x x + y y) + z z <= max_range * max_range (fp32).  The candidate list keeps the input order; K entries.
 *  2 HYPOTHESES  hypothesis h in [0, H) draws three candidate slots, slot j = (uint64(fmix32(seed + 0x9E3779B9 (3 h + j + 1))) K)
 *    >> 32, fmix32 MurmurHash3's 32-bit finaliser, arithmetic mod 2^32.  With a, b, c the slots' points: DEGENERATE if two slots
 *    coincide or, in fp64 from the fp32 points, n = (b - a) x (c - a) has |n|^2 <= 1e-12 |b - a|^2 |c - a|^2.  Otherwise n is
 *    normalised, flipped so that n.u >= 0, d = -n.a; STEEP, and out of the vote, if n.u < cos(max_normal_angle_deg).  The plane
 *    is rounded to fp32.
 *  3 SCORING     count_h = the candidates with fabsf(((nx x + ny y) + nz z) + d) <= inlier_threshold in fp32: integers, exact.
 *  4 BEST        the largest count; among equals the lowest index.
 *  5 REFIT       refit_iterations times: the inliers of the current plane (the test of 3 against the plane rounded to fp32);
 *    sum p, sum p p^T and the count in fp64 in one fixed order (per-tile records, a fixed tree, no floating-point atomics); on
 *    the host the centroid c, the covariance, the eigenvector of its smallest eigenvalue by 3x3 Jacobi, oriented to u, d = -n.c.
 *  6 RESULT      plane (unit normal, n.u >= 0, n.p + d = 0), n_candidates, n_inliers and rms_distance (fp64, of the inliers'
 *    distances) under the final plane, best_hypothesis, best_count, status.
 *  7 STATUS      the first that applies: FEW_CANDIDATES (K < 3 or K < min_inliers; plane zero, best_hypothesis -1),
 *    NO_HYPOTHESIS (all degenerate or steep; plane zero, best_hypothesis -1), FEW_INLIERS (a pass over the inliers -- before a
 *    refit, or the final one -- found fewer than max(3, min_inliers); the plane is the last one fitted), STEEP (a refitted normal
 *    is beyond the angle; the plane is that fit), else OK.  The calls return LSLAM_OK whatever the status (as
 *    lslam_kfs_loop_match does with its stage), < 0 on an error.
 * Everything is checked before anything runs -- LSLAM_ERR_INVALID, lslam_last_error names the cause, nothing has changed (the
 * caller's result structs included), for: a null ctx, store, cloud or result, a keyframe id out of range, an
 * up that is zero or not finite, an inlier_threshold that is not positive and finite, n_hypotheses not a multiple of 64 in
 * [64, 4096], a negative min_inliers or refit_iterations, a sensor_height that is not finite, a height_clip_range or max_range
 * that is negative or not finite, a max_normal_angle_deg outside [0, 180].  params NULL: the defaults. */
typedef struct lslam_floor_params {
  float up[3];                /* the sensor frame's up direction (any length)   (0, 0, 1) */
  float sensor_height;        /* of the sensor above the floor [m]              1.8 */
  float height_clip_range;    /* half width of the candidates' height band [m]  1.0 */
  float max_range;            /* candidates' range gate [m], 0 = off            0 */
  int32_t n_hypotheses;       /* H                                              512 */
  float inlier_threshold;     /* [m]                                            0.1 */
  int32_t min_inliers;        /*                                                512 */
  float max_normal_angle_deg; /* of a floor normal from up                      10 */
  int32_t refit_iterations;   /*                                                1 */
  uint32_t seed;              /*                                                1 */
} lslam_floor_params;
enum { LSLAM_FLOOR_OK = 0, LSLAM_FLOOR_FEW_CANDIDATES = 1, LSLAM_FLOOR_NO_HYPOTHESIS = 2, LSLAM_FLOOR_FEW_INLIERS = 3, LSLAM_FLOOR_STEEP = 4 };
typedef struct lslam_floor_result {
  double plane[4];
  double rms_distance;
  int32_t n_candidates, n_inliers, best_hypothesis, best_count, status, reserved;
} lslam_floor_result;
void lslam_floor_default_params(lslam_floor_params *params); /* writes every byte */
size_t lslam_sizeof_floor_params(void);
size_t lslam_sizeof_floor_result(void);
/* A host cloud (stride_bytes >= 16, {x, y, z} at 0 as elsewhere; the intensity is not read): uploaded, then as below. */
int lslam_floor_detect(lslam_ctx *ctx, const void *points, size_t n, size_t stride_bytes, const lslam_floor_params *params,
                       lslam_floor_result *result);
/* A cloud that is in the ctx's device memory already, packed {x, y, z, -}: read where it is. */
int lslam_floor_detect_device(lslam_ctx *ctx, const float *d_xyzi, size_t n, const lslam_floor_params *params,
                              lslam_floor_result *result);
/* The floor of each named keyframe's SURFACE cloud, where it lies in the store: results[n_ids], 0 <= n_ids <= 65535, an id may
 * repeat.  Every keyframe of the call goes through each stage in one launch (workgroups indexed by tile and keyframe); the host
 * reads one small record per keyframe and pass over the inliers (refit_iterations + 1 of them) and writes back one plane per
 * keyframe and refit.  No cloud moves in either direction: the store's byte counters stay.  Per-keyframe arithmetic does not
 * depend on the batch: the results are, bit for bit, those of lslam_floor_detect_device on each cloud.  (Named apart from
 * lslam_kfs_*: that prefix is the store's own, closed set of names.) */
int lslam_floor_detect_keyframes(lslam_kfs *kfs, int32_t n_ids, const int32_t *ids, const lslam_floor_params *params,
                                 lslam_floor_result *results);
/* Measurement tap (tools/bench_floor.py): enqueues `launches` launches of the scoring kernel alone, in the shape of the store's
 * last lslam_floor_detect_keyframes call and on its candidates and hypotheses, counting into counters of its own; not waited for
 * (time it with events on lslam_stream).  LSLAM_ERR_INVALID before such a call has run. */
int lslam_debug_floor_score(lslam_kfs *kfs, int32_t launches);
/* Debug tap of the ctx's last single-cloud detection (lslam_floor_detect, _device): the candidates' input indices
 * cand_idx[K], and per hypothesis the three slots triples[H][3] (positions in the candidate list), the fp32 plane planes[H][4]
 * (zero for a degenerate one) and counts[H] (-1 degenerate, -2 steep).  *n_candidates = K, *n_hypotheses = H; any array may be
 * NULL (call with all NULL to size them); the capacities are in entries (candidates, hypotheses). */
int lslam_debug_floor_hypotheses(lslam_ctx *ctx, int32_t *cand_idx, size_t cap_candidates, size_t *n_candidates, int32_t *triples,
                                 float *planes, int32_t *counts, size_t cap_hypotheses, size_t *n_hypotheses);

/* ---- edge information: the match Hessian of a pose-graph edge, in fp64 --------------------------------------------------------
 * Not in the reference: pose_graph/information_estimator.hpp returns the identity (its //@ todo), and graph.cpp:279-288,333-339
 * weight every edge with a constant.  These entry points give the Gauss-Newton normal matrix of a scan match at the pose it
 * returned, in the coordinates of the pose graph's edge error, so that an edge can be trusted in the directions its match
 * observed.  This comment is the specification (restated in numpy by tests/edge_information_ref.py).
 *
 * INPUT.  One sweep (lslam_sweep_ex with the search of `search_mode`, LSLAM_SEARCH_* without the LSLAM_SWEEP_* bits) over the
 * resident single scan at `pose` leaves, per scan point k (corner points, then surf points), coeff_k = (w*n | w*d) and flags_k
 * on the device.  p_k is the scan point in the sensor frame, R[i][j] = (double)T[4*i + j] of lslam_pose_to_isometry(pose, T).
 *
 * ROW, for every k with flags_k & 4 (row kept), in fp64 from the fp32 inputs, every product and sum rounded on its own (no FMA)
 * in the order written:
 *   c = (double)coeff_k.xyz          m_j = (R[0][j]*c_0 + R[1][j]*c_1) + R[2][j]*c_2          (m = R^T c)
 *   x = p_k x m:  x_0 = p_1*m_2 - p_2*m_1,  x_1 = p_2*m_0 - p_0*m_2,  x_2 = p_0*m_1 - p_1*m_0
 *   J_k = [ m_0 m_1 m_2 | 2 x_0  2 x_1  2 x_2 ]     order [t, q]          b_k = (double)coeff_k.w
 * J_k is the derivative at delta = 0 of the weighted residual c . (T * fromVectorMQT(delta) * p_k): the perturbation on the
 * RIGHT, delta_q the vector part of the unit quaternion (hence the 2).  With the measurement Z = T the error of an lslam_pg_*
 * edge, toVectorMQT(Z^-1 X_i^-1 X_j), is delta itself: H = sum_k J_k^T J_k is the information of that error up to the noise
 * scale (H / sigma^2 for residuals of standard deviation sigma).  No Euler Jacobian: nothing is singular at ry = +-90 degrees.
 *
 * SUMS.  H (21 upper-triangular entries, mirrored into the 36), sum_b2 = sum_k b_k^2, n_rows = rows kept, n_line / n_plane =
 * corner / surf points with flags_k & 2 (a line / plane was fitted: the sweep's own counters).  All accumulation is fp64 in a
 * FIXED order -- each lane serially over its points (point i of the context's ordered scan belongs to lane i mod (lanes of the
 * launch)), a butterfly over the wavefront, the wavefronts of a workgroup in order, the workgroups' partials in workgroup order
 * by one final workgroup; no floating-point atomics -- so two calls give the same bits.  Each entry lies within
 * (n_rows + 2) * 2^-53 * sum_k |J_ka J_kb| of the exact sum.
 *
 * EIGEN-DECOMPOSITION, on the host: cyclic Jacobi in fp64 on the symmetric 6x6.  eig ascending; evec row i is the unit
 * eigenvector of eig[i].
 *
 * lslam_match_information: the resident map and the resident single scan; one sweep with the taps left on the device (no
 * per-point data crosses PCIe), the reduction, one download of 25 numbers.  Errors as lslam_sweep_ex (LSLAM_ERR_NO_MAP,
 * _NO_SCAN, _INVALID for a NULL argument, a batch of scans or an unknown search mode); *out is zeroed first.  No kept rows
 * (an empty scan included): LSLAM_OK with H = 0, eig = 0, evec = identity. */
typedef struct {
  double H[36];        /* row-major, symmetric, order [t, q] */
  double eig[6];       /* ascending */
  double evec[36];     /* row i = eigenvector of eig[i] */
  double sum_b2;
  int32_t n_rows, n_line, n_plane;
} lslam_edge_info;
size_t lslam_sizeof_edge_info(void);
int lslam_match_information(lslam_ctx *ctx, const float pose[6], int32_t search_mode, lslam_edge_info *out);
/* The information of an edge between stored keyframes.  The reference is built exactly as lslam_kfs_loop_match builds it: the
 * local clouds of keyframes ref_ids under rel_T (1 <= n_ref <= 6; lslam_kfs_debug_local_clouds), lslam_voxel_grid with
 * leaf_ref_corner / leaf_ref_surf over them and leaf_corner / leaf_surf over keyframe new_id's clouds, lslam_map_set and
 * lslam_scan_set on the device, then lslam_match_information(lslam_isometry_to_pose(T), LSLAM_SEARCH_AUTO): same kernels in
 * the same order as those calls, same bits.  T: new_id's pose in ref_ids[0]'s frame (row-major 4x4), the edge's measurement.
 * A filtered reference with no corner or no surf point: LSLAM_OK with *out zero (nothing to match against).  The ctx's map and
 * resident scan belong to the call afterwards.  (Named apart from lslam_kfs_*: that prefix is the store's own, closed set of
 * entry points -- this one is a consumer of the store, as lslam_sc_* are.) */
int lslam_keyframe_edge_information(lslam_kfs *kfs, int32_t n_ref, const int32_t *ref_ids, const float *rel_T, int32_t new_id,
                               const float T[16], float leaf_ref_corner, float leaf_ref_surf, float leaf_corner, float leaf_surf,
                               lslam_edge_info *out);

/* ---- loop candidates by appearance: scan context over the keyframe store ----------------------------------------------------
 * Not in the reference: its LoopDetector only looks where the drifted estimate puts the vehicle (a sqrt(5) m radius search), so
 * a loop whose drift exceeds that is never tried.  These entry points find candidates from what a keyframe looks like: a Scan
 * Context descriptor (Kim & Kim, IROS 2018) per keyframe, built from the clouds where they lie in the store, and an exhaustive
 * comparison of a query keyframe with all earlier ones.  This comment is the specification (restated in numpy by
 * tests/place_recognition_ref.py).
 *
 * DESCRIPTOR of a keyframe: D[ring][sector], fp32, row-major, n_ring x n_sector, over the corner cloud followed by the surf
 * cloud.  up_axis 1 (y up: LOAM's frame, the reference's): (a, b, h) = (z, x, y); up_axis 2 (z up): (a, b, h) = (x, y, z); the
 * azimuth runs from +a towards +b, a right-handed rotation about the up axis.  Per point, in fp32, every operation rounded on
 * its own (no FMA):
 *   d2 = a*a + b*b;  rho = sqrtf(d2) (correctly rounded);  ring = (int)(rho * ring_scale), ring_scale = (float)n_ring / max_range
 *   (one fp32 division, on the host).  The point is dropped when a coordinate is not finite, rho == 0, !(rho < max_range) or
 *   ring >= n_ring.
 *   In fp64: ang = atan2((double)b, (double)a); if (ang < 0) ang += 2 pi; sector = min((int)(ang * sector_scale), n_sector - 1),
 *   sector_scale = n_sector / (2 pi) (fp64, on the host).
 *   v = h + height_offset (one fp32 add); a point with v <= 0 leaves its cell alone.
 * A cell holds the maximum v of its points, 0 without one.  A maximum does not depend on order: descriptors are bit-reproducible.
 *
 * DISTANCE of query Q to candidate C at shift s: over the columns j with |Q[:, j]| > 0 and |C[:, (j + s) mod n_sector]| > 0 the
 * mean of the cosines of the two columns; d(s) = max(0, 1 - mean), and 1 without such a column.  The pair's distance is
 * min_s d(s), its shift the smallest s that attains the minimum the kernel computed.  Every term is non-negative (no
 * cancellation); the order of summation is the kernel's (a column's dot over ascending rings, the columns ascending), and the
 * result is held to a float64 evaluation within (n_ring + n_sector + 8) * 2^-23: the (n - 1) u bound of the dot, the norms, the
 * quotient and the mean, with a factor of two to spare.
 * DETERMINISM: the distance and shift of a pair depend on the two descriptors only -- not on where the candidate sits in the
 * store, in a tile or in a batch -- and the same query asked twice gives the same bits.
 * SHIFT: if the query sensor is rotated by psi about the up axis relative to the candidate at the same place, the best shift is
 * round(psi / (2 pi / n_sector)) mod n_sector; the pose of the query in the candidate's frame (p_c = T p_q) is the rotation by
 * shift * 2 pi / n_sector about the up axis with zero translation -- what lslam_kfs_loop_match takes as `guess`.
 *
 * Descriptors live in device slabs that grow with the store, are never moved and are freed by lslam_kfs_clear /
 * lslam_kfs_destroy (the store's lifetime rule).  They are built lazily: a call that needs them first describes every keyframe
 * that has none, in one launch.  A store on which lslam_sc_setup was never called allocates nothing for them. */
typedef struct lslam_sc_params {
  int32_t n_ring;       /* 20    2 .. 32 */
  int32_t n_sector;     /* 60    4 .. 128 */
  float max_range;      /* 80.0  > 0 [m] */
  float height_offset;  /* 2.0   added to the height: the sensor's height above the lowest surface that should count */
  int32_t up_axis;      /* 1     1: y up, 2: z up */
} lslam_sc_params;
typedef struct lslam_sc_stats {
  lslam_sc_params params;     /* in force (zero before lslam_sc_setup) */
  int32_t is_set;             /* 1 once lslam_sc_setup succeeded */
  int64_t n_described;        /* keyframes that have their descriptor */
  uint64_t descriptor_bytes;  /* device memory of the descriptor slabs */
  int64_t describe_launches;  /* launches of the describe kernel ... */
  int64_t query_launches;     /* ... and of the query kernel, since creation */
} lslam_sc_stats;
/* Kernel shape, for tests that have to straddle it: points a workgroup takes per pass of the describe kernel, candidates per
 * workgroup of the query kernel. */
#define LSLAM_SC_POINT_CHUNK 256
#define LSLAM_SC_CAND_TILE 64
#define LSLAM_SC_MAX_TOP_K 32
/* Writes every byte of *p (the defaults above). */
void lslam_sc_default_params(lslam_sc_params *p);
/* Validates (LSLAM_ERR_INVALID, the message names the field) and installs the parameters; NULL: the defaults.  Parameters that
 * differ from those in force drop the descriptors held. */
int lslam_sc_setup(lslam_kfs *kfs, const lslam_sc_params *params);
/* Parity tap: keyframe id's descriptor (the raw maxima), downloaded; out[n_ring * n_sector]. */
int lslam_sc_descriptor(lslam_kfs *kfs, int32_t id, float *out);
/* Query q (keyframe query_ids[q]) against every keyframe 0 .. max_cand_id[q], inclusive; max_cand_id NULL: query_ids[q] - 1; a
 * value below 0: no candidate, n_out[q] = 0; a value >= n_keyframes is refused.  The top_k (1 .. 32) best are selected on the
 * device by distance ascending, then id ascending; only the lists come back, behind one host wait for the whole call:
 * ids_out / shift_out / dist_out [n_query * top_k], list q at q * top_k, n_out[q] = min(top_k, eligible) entries of it valid.
 * n_query: 0 (nothing happens) .. 65535.  The entry points are lslam_sc_*, not lslam_kfs_sc_*: the set of lslam_kfs_* names is
 * pinned by the keyframe store's own ABI test. */
int lslam_sc_query(lslam_kfs *kfs, int32_t n_query, const int32_t *query_ids, const int32_t *max_cand_id, int32_t top_k,
                       int32_t *ids_out, int32_t *shift_out, float *dist_out, int32_t *n_out);
/* Parity tap: the query kernel's distance and shift of keyframe query_id against every keyframe, itself included, without
 * selection; dist_out / shift_out [n_keyframes]. */
int lslam_sc_distances(lslam_kfs *kfs, int32_t query_id, float *dist_out, int32_t *shift_out);
int lslam_sc_info(lslam_kfs *kfs, lslam_sc_stats *out);

/* ---- visibility votes: the final map without moving objects ---------------------------------------------------------------
 * Not in the reference: its addFeatureCloud only voxel-filters, so a car that stood at a junction for two keyframes stays in the
 * saved map as a solid block.  The method is the usual one (Removert, ERASOR, OctoMap free space): a point is dynamic when other
 * keyframes looked through the place where it is.  Each keyframe gets a coarse range image, built from its clouds where they lie
 * in the store; a query point is projected into each voting keyframe's image and that keyframe votes "free" or "hit"; integer
 * votes decide, so the result does not depend on any order of summation.  This comment is the specification (restated in numpy
 * by tests/visibility_ref.py).
 *
 * PIXEL of a point p in a keyframe's sensor frame.  up_axis 1 (y up): (a, b, h) = (z, x, y); up_axis 2 (z up): (a, b, h) =
 * (x, y, z), as lslam_sc_params.  In fp32, every operation rounded on its own (no FMA):
 *   rho = sqrtf(a*a + b*b);  r = sqrtf((a*a + b*b) + h*h)
 * The point is OBSERVABLE iff its coordinates are finite, min_range <= r <= max_range (fp32) and, in fp64,
 *   rowd = (atan2((double)h, (double)rho) - el0) * row_scale   satisfies 0 <= rowd < n_row,
 * el0 = fov_down_deg * pi / 180 and row_scale = n_row / ((fov_up_deg - fov_down_deg) * pi / 180), both in fp64 from the fp32
 * parameters, on the host.  Then row = (int)rowd; ang = atan2((double)b, (double)a), plus 2 pi if negative;
 * col = min((int)(ang * col_scale), n_col - 1), col_scale = n_col / (2 pi) (fp64, on the host).
 *
 * RANGE IMAGE of a keyframe: n_row x n_col fp32, row-major, over the corner cloud followed by the surf cloud.  A pixel holds the
 * minimum r of its observable points, +inf without one (an integer atomic minimum on the bit patterns: positive floats order as
 * their bits, and a minimum does not depend on arrival order, so images are bit-reproducible).  Images are built lazily -- a call
 * that needs them first builds every keyframe's that has none, in one launch (behind one that fills them with +inf) -- live in
 * device slabs that never move and are freed by lslam_kfs_clear / lslam_kfs_destroy.  A store on which lslam_vis_setup was never
 * called allocates nothing for them.  Parameters that differ from those in force drop the images held.
 *
 * VOTE of voter k (keyframe ids[k] at poses[k]: row-major 4x4 fp32, graph <- sensor k) on query point q (graph frame).  The
 * inverse is formed on the host in fp64 as (R^T, -R^T t), row j of it (R0j, R1j, R2j | -((R0j t0 + R1j t1) + R2j t2)), rounded to
 * fp32; p = T^-1 q in fp32 as lslam_kfs_debug_local_clouds transforms: ((T0 x + T1 y) + T2 z) + T3.  p not observable: no vote.
 * Otherwise m = fmaxf(abs_margin, rel_margin * r); the window is the rows row - window .. row + window that lie in [0, n_row) and
 * the columns (col - window .. col + window) mod n_col.  FREE iff the centre pixel is finite and every finite window pixel v has
 * v > r + m (one fp32 add); HIT iff some finite window pixel has fabsf(v - r) <= m (one fp32 subtraction).  The two are counted
 * independently and exclude each other but for a difference v - r above m that rounds onto m.
 * Per point the calls return n_free | n_hit << 16 (uint32); the point is DYNAMIC iff n_free >= min_free_votes && n_free > n_hit.
 * The same id may be named more than once (it then votes more than once); n_ids is 0 .. 65535, so neither half can overflow.
 *
 * Everything is checked before anything runs -- LSLAM_ERR_INVALID, lslam_last_error names the cause, nothing has changed (the
 * caller's outputs included) -- for: a null or destroyed store, votes before lslam_vis_setup, a keyframe id out of range, a pose
 * that is not finite, null arrays with something to read or write, n above 2^31 - 1, n_ids outside 0 .. 65535, a stride under
 * 16 bytes, and in lslam_vis_setup: n_row outside 1 .. 128, n_col outside 4 .. 4096, fov angles that are not finite, outside
 * [-90, 90] or not fov_down_deg < fov_up_deg, min_range not positive and finite, max_range not finite or not above min_range,
 * window outside 0 .. 3, abs_margin / rel_margin negative or not finite, min_free_votes below 1, up_axis neither 1 nor 2. */
typedef struct lslam_vis_params {
  int32_t n_row;           /* 16     1 .. 128 */
  int32_t n_col;           /* 360    4 .. 4096 */
  float fov_down_deg;      /* -16    the lower ... */
  float fov_up_deg;        /* 16     ... and upper edge of the image's elevation range, within [-90, 90] */
  float min_range;         /* 1.0    > 0 [m] */
  float max_range;         /* 80.0   > min_range [m] */
  int32_t window;          /* 1      0 .. 3 pixels to every side */
  float abs_margin;        /* 0.5    >= 0 [m] */
  float rel_margin;        /* 0.02   >= 0, of the range */
  int32_t min_free_votes;  /* 2      >= 1 */
  int32_t up_axis;         /* 1      1: y up, 2: z up */
} lslam_vis_params;
typedef struct lslam_vis_stats {
  lslam_vis_params params;  /* in force (zero before lslam_vis_setup) */
  int32_t is_set;           /* 1 once lslam_vis_setup succeeded */
  int64_t n_images;         /* keyframes that have their range image */
  uint64_t image_bytes;     /* device memory of the image slabs */
  int64_t image_launches;   /* launches of the image kernel ... */
  int64_t vote_launches;    /* ... and of the vote kernel (the measurement tap's not counted), since creation */
} lslam_vis_stats;
/* Kernel shape, for tests that have to straddle it: query points per workgroup of the vote kernel (one per lane) and voters per
 * workgroup (grid: point tiles x keyframe chunks). */
#define LSLAM_VIS_POINT_TILE 256
#define LSLAM_VIS_KF_CHUNK 16
/* Writes every byte of *p (the defaults above). */
void lslam_vis_default_params(lslam_vis_params *p);
size_t lslam_sizeof_vis_params(void);
size_t lslam_sizeof_vis_stats(void);
/* Validates and installs the parameters; NULL: the defaults. */
int lslam_vis_setup(lslam_kfs *kfs, const lslam_vis_params *params);
int lslam_vis_info(lslam_kfs *kfs, lslam_vis_stats *out);
/* Parity tap: keyframe id's range image, downloaded; out[n_row * n_col]. */
int lslam_vis_range_image(lslam_kfs *kfs, int32_t id, float *out);
/* The votes of voters ids[n_ids] at poses[n_ids * 16] on n host points (stride_bytes >= 16, {x, y, z} at 0 as elsewhere):
 * uploaded, voted on, votes_out[n] downloaded.  These are query points of the caller's, not the store's clouds: the store's byte
 * counters stay. */
int lslam_vis_votes(lslam_kfs *kfs, int32_t n_ids, const int32_t *ids, const float *poses, const void *points, size_t n,
                    size_t stride_bytes, uint32_t *votes_out);
/* The same on points that are in the ctx's device memory, packed {x, y, z, -}; d_votes[n] in device memory.  Waited for. */
int lslam_vis_votes_device(lslam_kfs *kfs, int32_t n_ids, const int32_t *ids, const float *poses, const float *d_xyzi, size_t n,
                           uint32_t *d_votes);
/* The points that are not dynamic, in input order (a stable compaction on the device), into d_out (room for n points, must not
 * overlap d_xyzi); *n_kept of them. */
int lslam_vis_filter_device(lslam_kfs *kfs, int32_t n_ids, const int32_t *ids, const float *poses, const float *d_xyzi, size_t n,
                            float *d_out, size_t *n_kept);
/* lslam_kfs_add_to_fmap with the filter in front: keyframe id's corner and surf points are moved by T (the fp32 formula above),
 * voted on by the named voters; the survivors -- still in the sensor frame, in their order -- are compacted on the device and
 * handed to lslam_fmap_add_feature_cloud's device form with T.  n_removed[0 / 1]: corner / surf points left out.  No cloud
 * crosses PCIe: the store's byte counters stay. */
int lslam_vis_add_to_fmap(lslam_kfs *kfs, int32_t id, lslam_fmap *fm, const float T[16], int32_t n_ids, const int32_t *ids,
                          const float *poses, size_t n_removed[2]);
/* Measurement tap (tools/bench_visibility.py): enqueues `launches` launches of the vote kernel alone, in the shape of the store's
 * last lslam_vis_votes call and on its points, voters and poses, voting into a buffer of its own; not waited for (time it with
 * events on lslam_stream).  LSLAM_ERR_INVALID before such a call has run (or after lslam_kfs_clear / new parameters). */
int lslam_debug_vis_votes(lslam_kfs *kfs, int32_t launches);

/* ---- 2D occupancy grid: ray-cast votes of the keyframes ---------------------------------------------------------------------
 * Not in the reference: nothing in it produces the map a map_server / move_base stack loads.  Every point of every keyframe is a
 * ray from the sensor to the point; the cells the ray crosses were seen free, the cell it ends in -- if the point stands at
 * obstacle height above the keyframe's floor plane -- was seen occupied.  One grid per store; nothing is allocated before
 * lslam_occ_setup, and the grid itself when it is first needed; lslam_kfs_clear / lslam_kfs_destroy free it (over a clear the
 * parameters stay, and the next call that needs the grid allocates it again, zeroed).  Every decision is an integer one:
 * results are reproducible to the bit and do not depend on order, chunking or launch shape.  This comment is the specification
 * (restated in numpy and Python integers by tests/occupancy_ref.py).
 *
 * AXES.  up_axis 1 (y up): (a, b, h) = (z, x, y); up_axis 2 (z up): (a, b, h) = (x, y, z), as lslam_vis_params.  The grid has
 * `width` cells along a and `height` cells along b; cell (i, j) covers a in origin[0] + [i, i+1) * resolution and b likewise
 * with j; arrays are row-major with index j * width + i.
 *
 * A KEYFRAME'S VOTE takes its id, its pose T (row-major 4x4 fp32, graph <- sensor; only the first three rows are read) and a
 * plane (n, d) in the sensor frame, n.p + d = 0 on the floor and n pointing up (lslam_floor_result.plane), given as four fp64
 * and rounded to fp32.  Without a plane (planes NULL, or plane_valid given and 0 for the entry) the fallback (u, sensor_height)
 * is used, u the unit up axis.  The vote runs over the corner cloud followed by the surf cloud.  Per point p = (x, y, z), in
 * fp32 with every operation rounded on its own (no FMA):
 *   GATE    the point takes part iff x, y, z are finite and lo <= (x*x + y*y) + z*z <= hi, lo = min_range * min_range and
 *           hi = max_range * max_range (one fp32 product each).  No square root.
 *   HEIGHT  hgt = ((nx*x + ny*y) + nz*z) + d.  OBSTACLE iff obstacle_min <= hgt <= obstacle_max; GROUND iff
 *           fabsf(hgt) <= ground_band and ground_clears != 0 (the parameter limits make the two exclude each other); any
 *           other point is ignored: it is no ray.
 *   END     E = ((T0*x + T1*y) + T2*z) + T3 per row; the ray's origin O is the pose's translation (T3, T7, T11).
 *   FIXED POINT  s = 256.0 / (double)resolution (one fp64 division, on the host);
 *           Q(v, r) = floor(((double)v - r) * s), in fp64, nothing contracted; A = (Q(Oa, origin[0]), Q(Ob, origin[1])),
 *           B = (Q(Ea, origin[0]), Q(Eb, origin[1])).  The ray is DROPPED (counted in rays_dropped, no vote) unless all
 *           four values lie in [-2^30, 2^30) -- a value that is not finite (E overflowed) does not.  Then they are integers.
 * CELLS CROSSED.  Cell (i, j) is crossed by the ray iff the open segment A + t (B - A), 0 < t < 1, meets the open square
 * (256 i, 256 (i+1)) x (256 j, 256 (j+1)); decided exactly in integers.  A ray of zero length (A == B) crosses its own cell
 * iff A lies in its open interior.  A ray along a grid line crosses nothing; a ray through a lattice corner does not enter the
 * two cells it only touches.  The END cell is (floor(Ba / 256), floor(Bb / 256)); it need not be crossed (B may lie on a wall).
 * PER KEYFRAME k, both restricted to the grid:  HIT_k = the end cells of its obstacle rays;  FREE_k = (the crossed cells of its
 * obstacle rays, each without that ray's own end cell, and all crossed cells of its ground rays) minus HIT_k.  So a keyframe
 * votes at most once per cell and a hit beats a free: a wall seen at a grazing angle is not erased by the rays along it.
 * COUNTS.  One uint32 per cell, n_free | n_hit << 16, summed over the keyframes integrated since the last clear (an id named
 * twice votes twice).  At most 65535 keyframes may be integrated into one grid, so neither half overflows.
 * VALUES.  One int8 per cell from its count alone, on the device: with H = hit_weight * n_hit and D = H + n_free, the value is
 * -1 iff n_hit + n_free < min_observations, else (200 * H + D) / (2 * D) in integer division: 0 .. 100, round(100 H / D).
 *
 * THE KERNELS' WINDOW.  A keyframe's bits live in a window of the grid that the host derives from the pose: along axis c with
 * pose row (r0, r1, r2 | t), every E_c lies within t +- L, L = |r| * max_range * (1 + 1e-6) + 1e-6 * ((|r0| + |r1| + |r2|) *
 * max_range + |t|) + 1e-30 (Cauchy-Schwarz on the gated point, plus a bound on the four fp32 roundings of E); Q is monotone, so the
 * cells of Q(t - L) .. Q(t + L), clipped to the grid, hold every cell the keyframe can touch -- whatever the pose: it need not
 * be a rotation.  A cell outside it would make the call fail with LSLAM_ERR_HIP instead of being lost (none can).
 *
 * REFUSALS.  Everything is checked before anything runs -- LSLAM_ERR_INVALID, lslam_last_error names the cause, nothing has
 * changed (the caller's outputs included) -- for: a null or destroyed store, use before lslam_occ_setup, a keyframe id out of
 * range, a pose (first three rows) or a plane that is read and is not finite in fp32, a plane normal of zero length, null arrays
 * with something to read or write, n_ids outside 0 .. 65535, an integration that would bring the keyframes integrated above
 * 65535, and in lslam_occ_setup every limit of the table below (values that are not finite included).  Parameters that differ
 * from those in force clear the grid. */
typedef struct lslam_occ_params {
  double origin[2];        /* 0, 0   graph-frame (a, b) of the corner of cell (0, 0); finite */
  float resolution;        /* 0.1    metres per cell, >= 0.01 */
  int32_t width;           /* 0      cells along a ... */
  int32_t height;          /* 0      ... and along b: each 1 .. 8192, product <= 2^26 (the defaults are refused: set them,
                                     or let lslam_occ_fit_bounds) */
  int32_t up_axis;         /* 1      1: y up, 2: z up */
  float min_range;         /* 1.0    > 0 [m] */
  float max_range;         /* 40.0   > min_range; max_range / resolution <= 2048 (fp32 division) */
  float obstacle_min;      /* 0.3    height above the floor [m] ... */
  float obstacle_max;      /* 2.0    ... obstacle_min < obstacle_max */
  float ground_band;       /* 0.15   0 <= ground_band < obstacle_min */
  float sensor_height;     /* 1.8    d of the fallback plane; finite */
  int32_t ground_clears;   /* 1      0 or 1: ground returns clear the cells their rays cross */
  int32_t hit_weight;      /* 3      1 .. 16 */
  int32_t min_observations;/* 1      >= 1 */
  int32_t reserved;        /* 0      must be 0 */
} lslam_occ_params;
typedef struct lslam_occ_stats {
  lslam_occ_params params;      /* in force (zero before lslam_occ_setup) */
  int32_t is_set;               /* 1 once lslam_occ_setup succeeded */
  int32_t n_integrated;         /* keyframe votes summed in the counts since the last clear */
  int64_t rays_cast;            /* since the last clear: rays_obstacle + rays_ground */
  int64_t rays_dropped;         /* obstacle or ground points whose ray left the fixed-point range */
  int64_t rays_obstacle;        /* obstacle rays that voted */
  int64_t rays_ground;          /* ground rays that voted */
  uint64_t grid_bytes;          /* device memory of the counts and values */
  uint64_t scratch_bytes;       /* ... and of the bit planes of a chunk of keyframes */
  int64_t ray_launches;         /* launches, since creation and without the measurement tap's: the ray kernel, */
  int64_t merge_launches;       /* the merge of a chunk's bit planes into the counts, */
  int64_t value_launches;       /* the values from the counts */
} lslam_occ_stats;
/* Kernel shape, for tests that have to straddle it: points per workgroup of the ray kernel (whose (ray, column) items are dealt
 * to its lanes by a prefix sum of the rays' column counts) and keyframes per launch (grid: point tiles x keyframes). */
#define LSLAM_OCC_RAY_TILE 256
#define LSLAM_OCC_KF_CHUNK 8
/* Writes every byte of *p (the defaults above). */
void lslam_occ_default_params(lslam_occ_params *p);
size_t lslam_sizeof_occ_params(void);
size_t lslam_sizeof_occ_stats(void);
/* Validates and installs the parameters (NULL is refused: width and height have no default).  The same parameters again change
 * nothing; others clear the grid. */
int lslam_occ_setup(lslam_kfs *kfs, const lslam_occ_params *params);
int lslam_occ_info(lslam_kfs *kfs, lslam_occ_stats *out);
/* Zeroes the counts, n_integrated and the ray counters; the parameters stay. */
int lslam_occ_clear(lslam_kfs *kfs);
/* Adds the votes of keyframes ids[n_ids] at poses[n_ids * 16].  planes: n_ids * 4 fp64 or NULL (every keyframe uses the
 * fallback); plane_valid: n_ids flags or NULL (every plane given is used); an entry whose flag is 0 uses the fallback and its
 * plane is not read.  No cloud crosses PCIe: the store's byte counters stay.  Waited for. */
int lslam_occ_integrate(lslam_kfs *kfs, int32_t n_ids, const int32_t *ids, const float *poses, const double *planes,
                        const int32_t *plane_valid);
/* Downloads: out[width * height]. */
int lslam_occ_counts(lslam_kfs *kfs, uint32_t *out);
int lslam_occ_values(lslam_kfs *kfs, int8_t *out);
/* The device arrays themselves (either pointer may be NULL); the values are recomputed first if counts changed since.  Waited
 * for; valid until the next lslam_occ_setup with other parameters, lslam_kfs_clear or lslam_kfs_destroy. */
int lslam_occ_view(lslam_kfs *kfs, const uint32_t **d_counts, const int8_t **d_values);
/* Host only, fp64: the smallest grid with origin on multiples of the resolution that holds every pose's position +- max_range.
 * Reads resolution, max_range and up_axis of *params and writes origin, width and height.  With r = (double)resolution,
 * m = (double)max_range and, per axis, lo = min O - m, hi = max O + m over the n poses (row-major 4x4 fp32):
 *   i0 = floor(lo / r), lowered by one while i0 * r > lo, then raised by one while (i0 + 1) * r <= lo;  origin = i0 * r;
 *   cells = max(1, ceil((hi - origin) / r)), raised by one while origin + cells * r < hi, lowered by one while cells > 1 and
 *   origin + (cells - 1) * r >= hi  (the products and sums as written, in fp64).
 * Refused -- *params untouched -- for n < 1, null arguments, a position that is not finite, resolution / max_range / up_axis
 * outside lslam_occ_setup's limits, or a result that breaks a size limit (the message names the size it would need). */
int lslam_occ_fit_bounds(int32_t n, const float *poses, lslam_occ_params *params);
/* Measurement tap (tools/bench_occupancy.py): enqueues, `launches` times, the ray kernel launches of the store's last
 * lslam_occ_integrate call (every chunk, each behind the memset of its bit planes), on bit planes and counters of its own: the
 * grid and the stats do not change.  Not waited for (time it with events on lslam_stream).  LSLAM_ERR_INVALID before such a call
 * with n_ids > 0 has run (or after a clear of the store or new parameters). */
int lslam_debug_occ_integrate(lslam_kfs *kfs, int32_t launches);

/* ---- map quality: mean map entropy and mean plane variance; trajectory evaluation ------------------------------------------
 * The reference's only accuracy tool is map_evaluation/Evaluation.cpp (lidar pose against GPS: lslam_traj_eval below).  For the
 * MAP it has none; these are the usual ground-truth-free crispness measures (Droeschel et al. 2014; Razlaw et al. 2015): per
 * point the covariance of its neighbourhood within a radius, from it the differential entropy of the fitted Gaussian (MME: the
 * mean) and the variance along the neighbourhood's normal (MPV: the mean).  Lower is crisper.  This comment is the
 * specification (restated in numpy by tests/map_quality_ref.py).
 *
 * INPUTS.  A surface cloud S and a query cloud Q (Q = S when no queries are given), records {x, y, z, -} of fp32.  Non-finite
 * points of S are dropped.  Non-finite points of Q are counted in n_nonfinite; their outputs are written as for a sparse point.
 *
 * Per finite query q:
 * NEIGHBOURS.  p in S is a neighbour iff, in fp32, (dx*dx + dy*dy) + dz*dz < (float)((double)r * r), d = p - q per axis, the
 * products summed left to right and nothing contracted (the survey extractor's rule).  A query that is itself in S counts
 * itself.  k = the number of neighbours.  k < min_neighbors: the point is SPARSE -- counted in n_sparse, its eigenvalues and
 * entropy are NaN, its count is still k.
 * SUMS, exact.  Per axis d = (double)p - (double)q (exact) and D = llrint(d * 65536.0), round half to even: units of 2^-16 m,
 * a quantisation of 15 um whose variance, 2e-11 m^2, lies below every floor used here.  The nine sums  Dx, Dy, Dz, DxDx, DxDy,
 * DxDz, DyDy, DyDz, DzDz  over the neighbours are int64.  Range: a neighbour has |d| < 8 + 3e-7 per axis (r <= 8 and the fp32
 * test), so |D| <= 2^19, a product is at most 2^38, and fewer than 2^25 surface points keep every sum below 2^63.  Integer
 * sums do not depend on the order of summation: results are bit-identical from run to run, for any order of S and for any
 * launch geometry (the property the visibility votes have).
 * COVARIANCE, a fixed fp64 sequence, nothing contracted.  Each sum is converted to double (one correctly rounded conversion)
 * and scaled by 2^-16 (first moments) or 2^-32 (second moments), exactly; with K = (double)k
 *   mx = sx / K, my = sy / K, mz = sz / K;  a00 = sxx / K - mx * mx,  a01 = sxy / K - mx * my, ... a22 = szz / K - mz * mz
 * EIGENVALUES.  Ten cyclic sweeps (0,1), (0,2), (1,2) of the Jacobi rotation the survey extractor's normals use (one shared
 * definition), then the diagonal sorted ascending: l0 <= l1 <= l2.
 * PLANE VARIANCE  v = max(l0, 0).
 * ENTROPY  h = 0.5 * ((ln l0' + ln l1') + ln l2') + 4.2568155996140185, lk' = max(lk, lambda_floor); the constant is
 * 1.5 * ln(2 pi e) as that literal.  The floor keeps an exactly planar or collinear neighbourhood defined.
 *
 * AGGREGATES over the DEFINED points (finite and not sparse), exact as well:
 *   sum_entropy_q32 = sum llrint(h * 2^32),  sum_plane_var_q30 = sum llrint(v * 2^30),  sum_neighbors = sum k,  max_neighbors
 * and from them mean_entropy = ((double)sum_entropy_q32 / 2^32) / n_defined, mean_plane_variance = ((double)sum_plane_var_q30 /
 * 2^30) / n_defined, mean_neighbors = (double)sum_neighbors / n_defined; NaN, all three, when n_defined is 0 (the status is still
 * LSLAM_OK).  (|h| < 38 for lambda_floor >= 1e-12: the entropy sum then stays below 2^63 for every admissible cloud.)
 *
 * REFUSED with LSLAM_ERR_INVALID before anything runs, lslam_last_error naming the cause: 2^25 or more surface or query points;
 * radius not finite or outside (0, 8]; min_neighbors below 3; lambda_floor not finite or not positive; a stride under 12 bytes
 * or no multiple of 4; a null cloud with points; which outside {0, 1}; a keyframe id out of range; a pose that is not finite. */
typedef struct lslam_mapq_params {
  float radius;            /* 0.3    (0, 8] [m] */
  int32_t min_neighbors;   /* 5      >= 3 */
  double lambda_floor;     /* 1e-8   > 0 [m^2] */
  int32_t reserved[4];     /* zero */
} lslam_mapq_params;
typedef struct lslam_mapq_stats {
  int64_t n_surface;           /* finite surface points */
  int64_t n_query;             /* query points given */
  int64_t n_nonfinite;         /* ... not finite */
  int64_t n_sparse;            /* ... finite with fewer than min_neighbors neighbours */
  int64_t n_defined;           /* ... the others */
  int64_t sum_entropy_q32;
  int64_t sum_plane_var_q30;
  int64_t sum_neighbors;
  int64_t max_neighbors;
  double mean_entropy;         /* MME */
  double mean_plane_variance;  /* MPV [m^2] */
  double mean_neighbors;
  /* device time of the call's stages (events on the context's stream): both clouds' sorts by grid cell; the neighbourhood
   * sums; the per-point tail with the reduction of the aggregates */
  float ms_sort, ms_kernel, ms_reduce, reserved;
} lslam_mapq_stats;
/* Writes every byte of *p (the defaults above). */
void lslam_mapq_default_params(lslam_mapq_params *p);
size_t lslam_sizeof_mapq_params(void);
size_t lslam_sizeof_mapq_stats(void);
/* Host clouds ({x, y, z} at byte 0 of each record).  queries NULL: the surface queries itself (nq, qstride_bytes ignored).
 * params NULL: the defaults.  Any output may be NULL: out_lambda3[nq][3] and out_entropy[nq] doubles (NaN where undefined),
 * out_count[nq] the neighbour counts, in the order of the queries. */
int lslam_mapq_eval(lslam_ctx *ctx, const void *surface, size_t n, size_t stride_bytes, const void *queries, size_t nq,
                    size_t qstride_bytes, const lslam_mapq_params *params, lslam_mapq_stats *stats, double *out_lambda3,
                    double *out_entropy, int32_t *out_count);
/* The same on clouds that are in the ctx's device memory, packed {x, y, z, -}, with device outputs (or NULL): nothing but the
 * stats crosses PCIe.  Waited for. */
int lslam_mapq_eval_device(lslam_ctx *ctx, const float *d_surface, size_t n, const float *d_queries, size_t nq,
                           const lslam_mapq_params *params, lslam_mapq_stats *stats, double *d_lambda3, double *d_entropy,
                           int32_t *d_count);
/* The whole cube map where it lies (which: 0 corner, 1 surf), queried by itself.  An addFeatureCloud begun and not yet committed
 * is committed first. */
int lslam_mapq_fmap(lslam_fmap *fm, int32_t which, const lslam_mapq_params *params, lslam_mapq_stats *stats);
/* The named keyframes' clouds of one type, each moved by its pose (poses16[n_ids * 16]: row-major 4x4 fp32, graph <- sensor;
 * ((T0 x + T1 y) + T2 z) + T3 per row in fp32 as lslam_kfs_debug_local_clouds transforms) into ONE device cloud, queried by
 * itself: the form that scores a trajectory -- the same clouds at odometry poses against the same clouds at optimised poses.
 * No cloud crosses PCIe: the store's byte counters stay.  The same id may be named more than once. */
int lslam_mapq_keyframes(lslam_kfs *kfs, int32_t n_ids, const int32_t *ids, const float *poses16, int32_t which,
                         const lslam_mapq_params *params, lslam_mapq_stats *stats);

/* Trajectory evaluation (map_evaluation/Evaluation.cpp:39-150: lidarToMapHandler and process), on the host in fp64; needs no
 * device and no context.  est_xyz[n_est * 3], ref_xyz[n_ref * 3]; ref_stamp ascending.
 * ASSOCIATION.  Estimate i is paired with the reference sample nearest in time: scanning from the newest reference backwards
 * while |t_i - ref_stamp| strictly decreases (:44-51), so a tie goes to the later sample.  (The reference keeps the newest 1000
 * fixes in a ring and sees only those that arrived before the estimate; here every sample is there for every estimate.)
 * DIFFERENCES  |dx|, |dy|, |dz| and dist = sqrt((dx*dx + dy*dy) + dz*dz) (:53-58).
 * MAXIMA over EVERY pair -- the reference updates its maxima (:59-62) before it tests the gate (:64); kept.
 * GATE.  A pair with dist > gate (the reference's literal: 10 m; 0: no gate) is counted in n_gated and leaves everything else.
 * STATISTICS over the n_used others, summed in the order of the estimates from zero (:107-131): mean[4] of |dx|, |dy|, |dz|,
 * dist, mean_dt; var[4] = sum (x - mean)^2 / (n_used - 1) (NaN for n_used < 2; means NaN for n_used = 0).
 * ALIGNED ATE (not in the reference), with align != 0: the rigid transform (R | t) that best maps the used estimates onto their
 * references in the least-squares sense -- Kabsch on centred coordinates in fp64, the 3x3 SVD through the Jacobi
 * eigendecomposition of H^T H, det(R) = +1 enforced (the reflection case) -- then ate_rmse = sqrt(mean |R e + t - r|^2) and
 * T_align (row-major 4x4).  Fewer than three used pairs, or collinear ones (the second singular value of H, the 3x3 sum of
 * centred estimate times centred reference, not above 1e-6 of the first): aligned = 0, ate_rmse NaN, T_align the identity.
 * Without references (n_ref = 0) there are no pairs: n_used = n_gated = 0.
 * LSLAM_ERR_INVALID: null arrays with something to read, null stats, a gate that is negative or not finite. */
typedef struct lslam_traj_params {
  double gate;          /* 10.0   >= 0 [m]; 0: no gate */
  int32_t align;        /* 0 */
  int32_t reserved[3];  /* zero */
} lslam_traj_params;
typedef struct lslam_traj_stats {
  int64_t n_used, n_gated;
  double mean[4], var[4], max[4];  /* |dx|, |dy|, |dz|, dist */
  double mean_dt;
  int32_t aligned, reserved;
  double ate_rmse;
  double T_align[16];
} lslam_traj_stats;
void lslam_traj_default_params(lslam_traj_params *p);
size_t lslam_sizeof_traj_params(void);
size_t lslam_sizeof_traj_stats(void);
int lslam_traj_eval(const double *est_stamp, const double *est_xyz, size_t n_est, const double *ref_stamp, const double *ref_xyz,
                    size_t n_ref, const lslam_traj_params *params, lslam_traj_stats *stats);

/* pcl::VoxelGrid<PointXYZI>::filter with a cubic leaf on one cloud (LaserMatcher.cpp:289-301,
 * ScanMatch.cpp:362-398 scanMatchLocal): one centroid {x,y,z,intensity} per occupied voxel, in
 * ascending voxel index.  Points of a voxel are summed in input order (PCL: unspecified), in fp32, and every sum STARTS FROM
 * ZERO as PCL's does: a field in which all of a voxel's members are -0.0f comes out as +0.0f (0.0f + -0.0f = +0.0f), a lone
 * point with a -0.0f field included; every other value is unaffected.  Where nothing is filtered -- more voxels than INT_MAX
 * ("leaf too small": the input comes back as it is), and in the cube map a cube outside the active area -- the points are
 * handed on bit for bit, -0.0f included.  The same rule holds for every entry that documents itself as this filter. */
int lslam_voxel_grid(lslam_ctx *ctx, const void *cloud, size_t n, size_t stride_bytes, float leaf,
                     float *out_xyzi, size_t cap, size_t *n_out);
/* Two clouds with the same leaf in one pass -- prepareFeatureFrame's corner and surface clouds (LaserMatcher.cpp:289-301, two
 * VoxelGrid objects there): each cloud is filtered on its own (own min_b, own "leaf too small" guard), one upload, one wait,
 * one download instead of two of each.  Bit for bit what two lslam_voxel_grid calls give. */
int lslam_voxel_grid2(lslam_ctx *ctx, const void *cloud_a, size_t n_a, const void *cloud_b, size_t n_b, size_t stride_bytes,
                      float leaf, float *out_a_xyzi, size_t cap_a, size_t *n_out_a, float *out_b_xyzi, size_t cap_b, size_t *n_out_b);

/* ---- feature extraction front end ------------------------------
 * Replaces ScanRegistration::extractFeatures (odometry/ScanRegistration.cpp:190-425, with
 * setScanBuffersFor :471-531, setRegionBuffersFor :427-469, markAsPicked :533-555 and
 * pointClassify :557-687) on the ring-sorted full-resolution cloud MultiScanRegistration::process
 * builds (MultiScanRegistration.cpp:178-190).  Building that cloud from raw driver packets is the
 * caller's here (ring from the vertical angle, IMU de-skew); lslam_sreg_* further down does all of it on the device, and
 * lslam_oreg_* the same for an organised cloud whose points carry their ring (OrganisedScanRegistration). */
typedef struct lslam_reg_params {     /* RegistrationParams, ScanRegistration.h:45-112 */
  int32_t n_feature_regions;          /* 6; 1 .. 512 (the device keeps the sort words of a ring's regions in LDS) */
  int32_t curvature_region;           /* 5 */
  int32_t max_corner_sharp;           /* 2 */
  int32_t max_surface_flat;           /* 4 */
  float less_flat_filter_size;        /* 0.2 */
  float surface_curvature_threshold;  /* 0.02 */
  float blind_threshold;              /* cos(deg2rad(blindDegreeThreshold = 0.5)) */
  int32_t reserved;
} lslam_reg_params;
void lslam_reg_default_params(lslam_reg_params *p);
/* cloud: n_points points, {x,y,z} at offset 0 and, at intensity_offset_bytes, the float copied to
 * the outputs' intensity (toXYZI, util/pcl_util.h:30-37: the `curvature` field = ring id +
 * relative time).  scan_ranges: n_scans x {first, last} inclusive index ranges (a ring of more
 * than 2560 points is refused).  sharp / less_sharp / flat / less_flat: room for n_points
 * {x,y,z,intensity} each (any may be NULL); counts = their sizes.  Optional taps, n_points each:
 * curvature (0 outside the feature regions), _scanNeighborPicked right after setScanBuffersFor,
 * final region label (PointLabel values, 6 = UNKNOW). */
int lslam_extract_features(lslam_ctx *ctx, const void *cloud, size_t n_points, size_t stride_bytes,
                           size_t intensity_offset_bytes, const int32_t *scan_ranges, size_t n_scans,
                           const lslam_reg_params *params, float *sharp, float *less_sharp, float *flat,
                           float *less_flat, size_t counts[4], float *curvature_out, int8_t *picked_out,
                           int8_t *label_out);

/* MultiScanRegistration::process (odometry/MultiScanRegistration.cpp:94-190) without the IMU
 * branch (the registration node, lslam_sreg_*, has it): raw driver cloud {x,y,z} -> ring-sorted cloud {x', y', z', ring + relTime} in the
 * registration's swapped axes (x' = y, y' = z, z' = x) with its per-ring {first, last} ranges --
 * the input of lslam_extract_features (intensity offset 12).  Linear ring mapper
 * (MultiScanRegistration.h:57-87: VLP-16 = -15..15 deg / 16, HDL-32 = -30.67..10.67 / 32).  atan /
 * atan2 are evaluated on the device: ring ids equal the reference's except for points within an
 * ulp of a ring boundary, relTime agrees to ~1e-7. */
int lslam_multiscan_register(lslam_ctx *ctx, const void *cloud, size_t n_points, size_t stride_bytes,
                             float lower_deg, float upper_deg, int32_t n_rings, float scan_period,
                             float *out_xyzc, size_t cap, size_t *n_out, int32_t *ranges_out);

/* ---- the odometry node resident on the device ("fully on device ... feeds the path without a CPU hop") ----
 *
 * A sweep's four feature clouds stay in HBM between the registration node and the odometry node: lslam_extract_features_dev
 * leaves them in an lslam_fset (the /laser_cloud_sharp, /laser_cloud_less_sharp, /laser_cloud_flat, /laser_cloud_less_flat
 * messages of ScanRegistration::publishResult, odometry/ScanRegistration.cpp, without the trip through the host), and
 * lslam_odom_process runs LaserOdometry::process (odometry/LaserOdometry.cpp:288-326) on them:
 *   first sweep     the less-sharp / less-flat clouds become _lastCornerCloud / _lastSurfaceCloud (:295-303)
 *   afterwards      scanMatch (:328-647) against the last clouds when they hold > 10 / > 100 points (:337) with the persistent
 *                   _transform as the initial guess, _Tsum = _Tsum * _transform (:649-653), transformToEnd of the less-sharp /
 *                   less-flat clouds (:312-313), which become the last clouds (:315-316)
 * with nothing but the 6 + 16 floats of the result (and, if asked for, the two last clouds the mapping node subscribes to)
 * crossing PCIe.  The nearest neighbour of :359 / :425 (nearestKSearch(pointSel, 1, ...), nanoflann_pcl.h:150-162) is found
 * through two hashed cell grids per last cloud (1 m cells, then 5.02 m cells: their 27-cell probe covers the 5 m gate of
 * :363,429 completely) with the proof of csrc/lslam_grid.hpp restated for k = 1: the smallest fp32 distance among the
 * candidates is nanoflann's answer when it is below the probe's guaranteed radius and no second point has the same distance;
 * an exact tie -- the one thing only nanoflann's visit order decides -- makes the call build the kd-trees after all and run
 * through them (lslam_odom_stats.tree_fallbacks counts those).  The grids are built by the same launch sequence that moves the
 * clouds to the sweep end: no kd-tree is built per sweep.  Same result as lslam_odometry_match + lslam_transform_to_end on
 * the same clouds, bit for bit (tests/test_gpu_odom.py). */
typedef struct lslam_fset lslam_fset;
typedef struct lslam_odom lslam_odom;
/* A feature set lives on the context's device; its buffers grow on demand.  It is complete when the call that fills it
 * returns, and free for the next fill once the lslam_odom_process that consumed it has returned (a program with the two nodes
 * on two threads rotates a few of them). */
int lslam_fset_create(lslam_ctx *ctx, lslam_fset **out);
void lslam_fset_destroy(lslam_fset *fs);
/* counts[4]: points in sharp, less-sharp, flat, less-flat */
int lslam_fset_counts(const lslam_fset *fs, size_t counts[4]);
/* Host clouds {x,y,z,intensity} (stride / intensity offset as lslam_odometry_match) into a feature set: the entry for callers
 * whose registration runs elsewhere, and for tests. */
int lslam_fset_upload(lslam_ctx *ctx, lslam_fset *fs, const void *sharp, size_t n_sharp, const void *less_sharp,
                      size_t n_less_sharp, const void *flat, size_t n_flat, const void *less_flat, size_t n_less_flat,
                      size_t stride_bytes);
/* One list back to the host, packed {x,y,z,intensity} (which: 0 sharp, 1 less-sharp, 2 flat, 3 less-flat). */
int lslam_fset_download(lslam_ctx *ctx, const lslam_fset *fs, int32_t which, float *out_xyzi, size_t cap, size_t *n_out);
/* lslam_extract_features with the four lists left in HBM (same kernels, same lists bit for bit). */
int lslam_extract_features_dev(lslam_ctx *ctx, const void *cloud, size_t n_points, size_t stride_bytes,
                               size_t intensity_offset_bytes, const int32_t *scan_ranges, size_t n_scans,
                               const lslam_reg_params *params, lslam_fset *out, size_t counts[4]);

typedef struct {
  int32_t matched;         /* 0: the first sweep, or the last clouds were too small (:337): no scan match ran */
  int32_t tree_fallbacks;  /* scan matches of this node so far that were redone through kd-trees (an exact distance tie) */
  int32_t searches;        /* correspondence refreshes of this sweep's loop (every fifth iteration, :357,:423) */
  int32_t reserved;
  uint64_t sweeps;         /* sweeps processed by this node so far */
  size_t n_last_corner, n_last_surf; /* the last clouds after this sweep */
} lslam_odom_stats;
/* LaserOdometry(scanPeriod, maxIterations = 25), _deltaTAbort = _deltaRAbort = 0.1 (LaserOdometry.cpp:24-25). */
int lslam_odom_create(lslam_ctx *ctx, int32_t max_iterations, float delta_t_abort, float delta_r_abort, lslam_odom **out);
void lslam_odom_destroy(lslam_odom *od);
/* LaserOdometry::process.  transform[6] (out) = _transform after the sweep, Tsum[16] (out) = _Tsum, row-major; stats (may be
 * NULL) as lslam_odometry_match fills it (zero when nothing was matched), ostats (may be NULL) the node's own.  last_corner /
 * last_surf (may be NULL): room for cap_corner / cap_surf packed {x,y,z,intensity} points -- the two clouds
 * LaserOdometry::publishResult sends to the mapping node (/laser_cloud_corner_last, /laser_cloud_surf_last), copied out behind
 * the same wait as the result.  Returns LSLAM_OK / LSLAM_NOT_CONVERGED as lslam_odometry_match, LSLAM_TOO_FEW_REF when nothing
 * was matched, a negative status on errors. */
int lslam_odom_process(lslam_odom *od, lslam_fset *fs, float transform[6], float Tsum[16], lslam_stats *stats,
                       lslam_odom_stats *ostats, float *last_corner, size_t cap_corner, float *last_surf, size_t cap_surf);
/* The last clouds as they are in HBM now (any pointer may be NULL; counts in lslam_odom_stats). */
int lslam_odom_last_clouds(lslam_odom *od, float *last_corner, size_t cap_corner, float *last_surf, size_t cap_surf);
/* Publishing without a copy on the host: with n_buffers > 0 every lslam_odom_process also leaves the two last clouds in one of
 * n_buffers page-locked buffers of the node, taken in turn, and lslam_odom_last_view hands out where (packed {x,y,z,intensity};
 * NULL / 0 before the first sweep).  A view stays valid until n_buffers further sweeps have been processed -- size the ring
 * for the sweeps the consumer (the mapping node) may lag behind -- or until the next lslam_odom_set_publish / _destroy.
 * n_buffers = 0 (the default) switches it off. */
int lslam_odom_set_publish(lslam_odom *od, int32_t n_buffers);
int lslam_odom_last_view(lslam_odom *od, const float **last_corner, size_t *n_corner, const float **last_surf, size_t *n_surf);
/* Profiling tap (a node made in a process with LSLAM_DEBUG_HOOKS=1 and LSLAM_ODOM_SEARCH_TAP=1): per query of the node's LAST
 * search launch four words -- 10 ns ticks, candidates looked at for the nearest neighbour, for the ring categories, bit 0 / 1 a
 * coarse-level pass in the former / the latter.  Returns the number of queries copied (0: tap off). */
int lslam_debug_odom_search(lslam_odom *od, uint32_t *out, size_t cap_queries);
/* Parity tap: ONE iteration of the loop of :328-647 -- the odometry counterpart of lslam_sweep_ex.  The sharp / flat lists of
 * fs are matched against the last clouds the node holds (after at least one lslam_odom_process), from `pose`, as iteration
 * `iter` of the loop (iter decides the weights of feature_utils.h; the correspondences are refreshed when iter % 5 == 0 or
 * refresh != 0 -- without a refresh the ones the previous call of this tap left for the same clouds are used).
 *   path 0  the launch loop's step: search (if refreshing), residual pass, solve
 *   path 1  the persistent kernel: search, then one generation -- iter must be 4, 9, ... or max_iterations - 1, so that the
 *           kernel leaves after one iteration by its own rule; at most 64 blocks; no per-point taps
 * The launch arguments are the ones lslam_odom_process builds.  Neither the last clouds nor the node's _transform change.
 * Any output but `out` may be NULL.  n = sharp + flat queries, sharp first:
 *   ind_out[3][n]   closest / second / third point (-1: none)      sel_out[n][3]   pointSel of the residual pass
 *   coeff_out[n][4] the coefficients as the row takes them (zeros where no second / third point)
 *   kept_out[n]     1: the row was kept                            sums_out[32]    the reduced sums the solve consumed
 * Returns LSLAM_TOO_FEW_REF when the node would not match (:337). */
typedef struct lslam_odom_step {
  float pose[6], x[6];  /* after the solve */
  int32_t n_rows, n_line, n_plane, degenerate, converged, done, loop_iter, solves;
  int32_t tie;        /* a nearest neighbour needed nanoflann's visit order */
  int32_t refreshed;  /* the search ran */
} lslam_odom_step;
int lslam_debug_odom_step(lslam_odom *od, lslam_fset *fs, const float pose[6], int32_t iter, int32_t refresh, int32_t path,
                          int32_t *ind_out, float *sel_out, float *coeff_out, uint8_t *kept_out, double sums_out[32],
                          lslam_odom_step *out);
/* How many matches of the node ran their loop in the persistent kernel and how many by one launch per step (more than 64
 * blocks of queries, LSLAM_ODOM_PERSISTENT=0, or after an exchange gave up).  Either pointer may be NULL. */
int lslam_debug_odom_runs(const lslam_odom *od, uint64_t *persistent_runs, uint64_t *launch_runs);
/* Start again from the first sweep (keeps the buffers). */
int lslam_odom_reset(lslam_odom *od);

/* ---- the registration node resident on the device, with the IMU branch ------------------------------------------------
 *
 * MultiScanRegistration (odometry/MultiScanRegistration.cpp:78-200 on ScanRegistration.cpp:89-188, :684-707) as one object: the
 * raw driver cloud goes up once, ring and relTime (as lslam_multiscan_register computes them, bit for bit), the projection of
 * every point to the sweep start with the interpolated IMU state (setIMUTransformFor + transformToStartIMU, whenever an IMU
 * has been heard), the grouping by ring, the per-ring ranges and the feature extraction all run on the device, the four lists
 * stay in an lslam_fset for lslam_odom_process, and the host waits once.  Without an IMU state the lists, the cloud and the
 * ranges are those of lslam_multiscan_register + lslam_extract_features_dev, bit for bit.
 *
 * IMU branch: the history lives on the host (lslam_sreg_imu_push = handleIMUMessage after getRPY: gravity removed in double,
 * position and velocity integrated in float, the ring buffer overwriting its oldest state) and reaches the device with the
 * sweep's upload.  The reference walks one index forward through the history while it visits the points in arrival order;
 * with stamps that increase that index is f(the largest relTime among the kept points so far, at least 0), f(t) = the first
 * state with (scanTime - stamp).toSec() + t <= 0 or the last state -- an inclusive prefix maximum and a binary search on the
 * device.  THEREFORE a stamp that is not later than the previous state's is refused.  States used as they are (index 0, or
 * a point later than the last state) keep the sine / cosine the host's C library cached when they were pushed; interpolated
 * angles get sin / cos on the device as a double evaluation rounded once to float (the correctly rounded value except within
 * ~1e-16 of a rounding boundary; glibc's sinf / cosf, which the reference calls, differ from that by one ulp for ~1.3 % of
 * angles), so the de-skewed coordinates agree with a CPU restatement to a bound, not bit for bit: PARITY UNPINNED, as the
 * reference's registration needs ROS and PCL to build (tests/scan_registration_ref.py is the CPU statement). */
typedef struct lslam_sreg lslam_sreg;
typedef struct lslam_sreg_stats {
  uint64_t sweeps;     /* sweeps this node has registered */
  size_t n_points;     /* points kept in this sweep's registered cloud */
  int32_t imu_states;  /* IMU states sent with this sweep (0: none heard, no de-skew) */
  int32_t launches;    /* kernels the node itself launches per sweep (7, 8 with the IMU branch), counted from the code; the
                          grouping's sort and scan (the library's) and the memsets of the extraction are not in it */
  size_t bytes_up;     /* host -> device, this sweep */
  size_t bytes_down;   /* device -> host, this sweep: the result words, the ranges and the grouping's three words */
} lslam_sreg_stats;
/* params NULL: lslam_reg_default_params.  Ring mapper and scan period as lslam_multiscan_register; imu_history_size: the
 * reference's imuHistorySize (200), 1 .. 512.  The node's buffers are its own and go with it; the grouping's scratch is the
 * context's. */
int lslam_sreg_create(lslam_ctx *ctx, const lslam_reg_params *params, float lower_deg, float upper_deg, int32_t n_rings,
                      float scan_period, int32_t imu_history_size, lslam_sreg **out);
void lslam_sreg_destroy(lslam_sreg *sr);
/* handleIMUMessage (ScanRegistration.cpp:89-120) after tf's getRPY: stamp in nanoseconds, roll / pitch / yaw in radians,
 * linear_acceleration {x, y, z} in the IMU's axes.  A stamp that is not later than the previous one is refused. */
int lslam_sreg_imu_push(lslam_sreg *sr, int64_t stamp_ns, double roll, double pitch, double yaw, const double linear_acceleration[3]);
/* States held, and the newest state's accumulated position / velocity (any pointer may be NULL). */
int lslam_sreg_imu_info(const lslam_sreg *sr, int32_t *size, double last_position[3], double last_velocity[3]);
/* Forget the history, _imuStart, _imuCur and the shift: the node is again one that has heard no IMU. */
int lslam_sreg_imu_clear(lslam_sreg *sr);
/* MultiScanRegistration::process(cloud, scanTime): cloud = n_points raw driver points {x,y,z} stride_bytes apart in arrival
 * order, scan_time_ns the cloud's stamp.  out receives the four lists (counts[4] their sizes, may be NULL); imu_trans (may be
 * NULL) the /imu_trans message: {start pitch, yaw, roll}, {current pitch, yaw, roll}, the shift and the velocity change in the
 * start frame (all zero while no IMU has been heard).  A sweep without a kept point succeeds with empty lists and leaves
 * _imuCur as it was.  Refused (LSLAM_ERR_INVALID, outputs zeroed, out reads empty): bad arguments and an empty cloud, found
 * before anything is enqueued -- the node is exactly as before, the last sweep's cloud included; a ring of more than 2560
 * points, found on the device and reported behind the same wait -- the IMU history, _imuStart, _imuCur and the shift are as
 * before and the node is usable, but its scratch has been written: lslam_sreg_cloud has nothing to hand out until the next
 * sweep succeeds. */
int lslam_sreg_process(lslam_sreg *sr, const void *cloud, size_t n_points, size_t stride_bytes, int64_t scan_time_ns,
                       lslam_fset *out, size_t counts[4], float imu_trans[12], lslam_sreg_stats *stats);
/* The last sweep's registered cloud (/velodyne_cloud_2: {x', y', z', ring + relTime}, ring-sorted) and its n_rings x {first,
 * last} ranges, on request (either pointer may be NULL; *n_out = the cloud's size). */
int lslam_sreg_cloud(lslam_sreg *sr, float *out_xyzc, size_t cap, size_t *n_out, int32_t *ranges_out);

/* ---- the registration node for organised clouds, resident on the device ------------------------------------------------
 *
 * OrganisedScanRegistration (odometry/OrganizedScanRegistration.cpp:82-150 on ScanRegistration.cpp:89-188, :684-707) as one
 * object: a height x width image whose points carry their own ring goes up once; the validity test (finite coordinates, then
 * x*x + y*y + z*z < blind_radius^2 drops the point -- strictly less: a point on the radius stays), relTime = (float)(scan_period
 * * (double)column / width), the 4th channel (float)ring + relTime -- the point's ring field, NOT its row --, the per-row clouds
 * concatenated in row order (a stable compaction of the row-major image: no sort, no atan), the height x {first, last} ranges
 * and the feature extraction all run on the device, the four lists stay in an lslam_fset for lslam_odom_process, and the host
 * waits once.  x, y, z are copied unchanged: this node has no axis swap.  Every number of it is exact float arithmetic in the
 * reference's order, so the cloud, the ranges and the lists equal a CPU restatement bit for bit
 * (tests/organised_registration_ref.py).
 *
 * IMU: the class inherits the subscription (lslam_oreg_imu_push = lslam_sreg_imu_push, the same history type), but its
 * process() never calls setIMUTransformFor / transformToStartIMU.  So with an IMU heard the points are NOT de-skewed, _imuCur
 * and _imuPositionShift stay as constructed (zero) for the life of the node, and /imu_trans is {start pitch, yaw, roll}, zeros,
 * the rotated zero shift, rotateYXZ(0 - _imuStart.velocity, -yaw, -pitch, -roll): host arithmetic on the history alone.  No IMU
 * state reaches the device. */
typedef struct lslam_oreg lslam_oreg;
typedef struct lslam_oreg_stats {
  uint64_t sweeps;     /* sweeps this node has registered */
  size_t n_cells;      /* height * width of this sweep's image */
  size_t n_points;     /* points kept in this sweep's registered cloud */
  int32_t imu_states;  /* IMU states held when this sweep was processed (0: none heard) */
  int32_t launches;    /* kernels the node itself launches per sweep (6: count, place, ranges, the extraction's three), counted
                          from the code; the memsets of the extraction are not in it */
  size_t bytes_up;     /* host -> device, this sweep: one block (result words, ranges, row counters, column times, cells) */
  size_t bytes_down;   /* device -> host, this sweep: the result words and the ranges */
} lslam_oreg_stats;
/* params NULL: lslam_reg_default_params.  scan_period > 0 (the reference's 0.1), blind_radius finite and >= 0 (the reference's
 * blindRaduis parameter, 2.5), imu_history_size 1 .. 512 (200).  The node's buffers are its own and go with it. */
int lslam_oreg_create(lslam_ctx *ctx, const lslam_reg_params *params, float scan_period, float blind_radius,
                      int32_t imu_history_size, lslam_oreg **out);
void lslam_oreg_destroy(lslam_oreg *og);
/* As lslam_sreg_imu_push / _imu_info / _imu_clear: a stamp that is not later than the previous one is refused. */
int lslam_oreg_imu_push(lslam_oreg *og, int64_t stamp_ns, double roll, double pitch, double yaw, const double linear_acceleration[3]);
int lslam_oreg_imu_info(const lslam_oreg *og, int32_t *size, double last_position[3], double last_velocity[3]);
int lslam_oreg_imu_clear(lslam_oreg *og);
/* OrganisedScanRegistration::process(cloud, scanTime): cloud = the row-major image, height * width points stride_bytes apart,
 * {x, y, z} floats at byte 0 of each point and the ring as a uint16 at ring_offset_bytes (the reference's PointXYZIT: stride 32,
 * ring at 26).  The device format is 16 bytes per cell, {x, y, z, word} with the ring in the low 16 bits of word (the upper 16
 * are ignored): a caller who has that layout (stride 16, ring at 12) is uploaded as is, anything else is repacked on the host.
 * out receives the four lists (counts[4] their sizes, may be NULL); imu_trans (may be NULL) the /imu_trans message described
 * above (all zero while no IMU has been heard).  A sweep that keeps nothing succeeds with empty lists.  A width above 2560 is
 * fine as long as no row KEEPS more than 2560 points.
 * Refused (LSLAM_ERR_INVALID, outputs zeroed, out reads empty) before anything is enqueued, the node exactly as before, the last
 * sweep's cloud included: null node, null cloud, a feature set on another device; height 0, width 0, height > 4096, height *
 * width > 0x3FFFFFFF; stride_bytes < 12 or not a multiple of 4, ring_offset_bytes + 2 > stride_bytes.  Refused on the device,
 * behind the same wait: a row that keeps more than 2560 points (the extraction's LDS limit) -- the node is usable, but
 * lslam_oreg_cloud has nothing to hand out until the next sweep succeeds. */
int lslam_oreg_process(lslam_oreg *og, const void *cloud, size_t height, size_t width, size_t stride_bytes, size_t ring_offset_bytes,
                       int64_t scan_time_ns, lslam_fset *out, size_t counts[4], float imu_trans[12], lslam_oreg_stats *stats);
/* The last sweep's registered cloud ({x, y, z, ring + relTime}, the rows concatenated) and its height x {first, last} ranges
 * (height = that sweep's), on request (either pointer may be NULL; *n_out = the cloud's size).  ranges_out is written only on
 * success. */
int lslam_oreg_cloud(lslam_oreg *og, float *out_xyzc, size_t cap, size_t *n_out, int32_t *ranges_out);

/* ---- coarse alignment of a loop-closure candidate ------------------------------
 * Replaces LoopDetector::corseMatching (pose_graph/loop_detector.hpp:232-255), i.e.
 * pcl::IterativeClosestPoint<PointXYZI, PointXYZI> with default settings: point-to-point ICP of `source`
 * onto `target` from the initial guess T (row-major 4x4, in/out = getFinalTransformation()).  PCL is not
 * part of the reference tree: PARITY UNPINNED (csrc/lslam_icp.hip states the restated defaults;
 * oracle/icp_oracle.py is the independent CPU statement).  max_iterations <= 0: 10; transformation_epsilon
 * 0 and max_correspondence_distance <= 0 (unlimited) are PCL's defaults.  *converged = hasConverged(),
 * *fitness = getFitnessScore().  An empty target returns converged = 0 (:233-235), fitness 0.  Fewer than 3
 * correspondences at the guess (a source of 0, 1 or 2 points, a gate that leaves as few): converged = 0,
 * iterations = 0, T untouched, and the fitness of the guess -- DBL_MAX when no source point has a correspondence
 * (an empty source included), which is what getFitnessScore() returns then.  A target of any rank gives a rigid
 * T (one point, two points, a line: the SVD's factors are completed to orthonormal ones, as Eigen's are).  The
 * context's resident map is replaced by the target's kd-tree (like lslam_odometry_match). */
int lslam_icp_align(lslam_ctx *ctx, const void *target, size_t n_target, const void *source, size_t n_source,
                    size_t stride_bytes, float T[16], int32_t max_iterations, double transformation_epsilon,
                    double max_correspondence_distance, double *fitness, int32_t *converged, int32_t *iterations);

/* ---- SE(3) pose-graph Levenberg-Marquardt ------------------------------------
 * Replaces pose_graph::SolverG2O (pose_graph/solver_g2o.cpp:51-95): add_se3_node /
 * add_se3_edge build the arrays passed to lslam_pg_create, optimize() becomes
 * lslam_pg_optimize.  g2o conventions (VertexSE3 / EdgeSE3 / "lm_var"): a pose is
 * {tx,ty,tz, qx,qy,qz,qw}; an edge e has vertices ij[2e], ij[2e+1], measurement
 * meas7[7e..] and a row-major 6x6 information matrix over [translation, rotation]
 * (pose_graph/graph.cpp:279-288: diag(0.8,0.4,0.8,1,2,1) for odometry, :333-339: 2*I
 * for loop closures); vertex `fixed_vertex` is held fixed (solver_g2o.cpp:55-59).  fp64.
 *
 * The damped system is solved by preconditioned CG (block Jacobi + a coarse level of rigid-body motions of graph
 * aggregates, csrc/lslam_posegraph.hip) instead of g2o's sparse Cholesky: same optimum (tests/test_posegraph_bench_fixture.py).
 * When a workgroup per aggregate fits the device at once (the 5 000-keyframe bench graph does: 88 aggregates) the whole PCG
 * loop of a damped solve, and the inverse of the coarse matrix, each run as ONE persistent cooperative launch
 * (lslam_pg_stats.fused_solves counts them); larger graphs take a launch-per-step loop with the same arithmetic.  A
 * cooperative launch wants its workgroups resident together; if they are not (another process's persistent kernel on the
 * same device) a grid exchange runs into its spin limit, the kernel raises an abort flag instead of hanging, the solve is
 * redone by the launch-per-step loop and the graph stays on that loop (tested through a debug hook).
 *
 * Multi-GPU (one process per GPU): every rank creates the same graph and takes an edge range
 * (lslam_pg_set_shard); the block system [diagonal blocks | off-diagonal blocks | b | chi2 | flag] is summed
 * across ranks once per linearisation -- by the library's RCCL communicator on the solver's stream
 * (lslam_pg_set_comm, further up) or through the callback of lslam_pg_set_shard for hosts with their own
 * transport; the damped solve is replicated and bit-identical on every rank. */
typedef struct lslam_pg lslam_pg;

typedef struct {
  int32_t iterations;     /* LM iterations (SparseOptimizer::optimize return value) */
  int32_t lm_trials;      /* damped solves, accepted + rejected */
  int32_t cg_iterations;  /* total preconditioned-CG iterations */
  int32_t status;
  double chi2_initial, chi2_final, lambda;
  float gpu_ms_total;
  int32_t fused_solves;   /* damped solves whose whole PCG loop ran in the persistent kernel (the rest took the
                             launch-per-step loop: graph too large for one workgroup per aggregate to be co-resident) */
} lslam_pg_stats;

/* In-place SUM over all ranks of `count` doubles at DEVICE address `buf`; must have
 * completed when it returns. */
typedef void (*lslam_allreduce_fn)(void *user, double *buf, size_t count);

/* ---- collectives: RCCL inside the library (north star: "RCCL all-reduce over xGMI of
 * the block Hessian") ------------------------------------------------------------------------
 * One process per GPU.  Rank 0 makes an id (lslam_comm_unique_id), the host program carries its 128
 * bytes to the other ranks (MPI, a file, torch.distributed ...), every rank creates a communicator
 * on its device and attaches it to a context (lslam_ctx_set_comm) and / or a pose graph
 * (lslam_pg_set_comm).  The sharded paths then enqueue ncclAllReduce on the library's own stream
 * between the producing and the consuming kernel: no host round trip per iteration.  librccl is
 * dlopen'ed on first use.  The lslam_allreduce_fn callbacks below remain for hosts that bring their
 * own transport (and for tests on one GPU, where RCCL refuses two ranks on one device). */
#define LSLAM_COMM_ID_BYTES 128
typedef struct lslam_comm lslam_comm;
int lslam_comm_unique_id(uint8_t id[LSLAM_COMM_ID_BYTES]);
int lslam_comm_create(int device, const uint8_t id[LSLAM_COMM_ID_BYTES], int32_t rank, int32_t world,
                      lslam_comm **out);
void lslam_comm_destroy(lslam_comm *comm);
/* ncclGetVersion of the librccl the library loaded (e.g. 22606 = 2.26.6) */
int lslam_comm_version(int32_t *version);
/* rank and rank count as the RCCL communicator itself reports them (ncclCommUserRank, ncclCommCount) */
int lslam_comm_info(const lslam_comm *comm, int32_t *rank, int32_t *world);
/* In-place SUM of `count` doubles at DEVICE address buf over all ranks, enqueued on hip_stream. */
int lslam_comm_allreduce_f64(lslam_comm *comm, double *device_buf, size_t count, void *hip_stream);
/* Attach (or, with NULL, detach) a communicator: lslam_scanmatch_run_sharded then needs no callback.
 * The communicator must outlive its use by the context. */
int lslam_ctx_set_comm(lslam_ctx *ctx, lslam_comm *comm);

/* ONE scan's points sharded over the ranks (the reference has no such seam: it is the
 * data-parallel form of ScanMatch.cpp:97-209 -- every point's row is independent given the
 * pose, the only coupling is the sum A^T A, A^T b and the counters).  Each rank holds its
 * contiguous shard of the corner and surf points (lslam_scan_set) and the whole map; per
 * Gauss-Newton iteration the rank's 32 fp64 sums (21 upper-triangular A^T A, 6 A^T b, rows,
 * line matches, plane matches, score, spare) are copied to xchg32 (DEVICE, 32 doubles, caller
 * owned -- e.g. a torch tensor the hook can all-reduce over RCCL), fn sums them over the
 * ranks in place, and every rank runs the same 6x6 solve on the same numbers.  The summation
 * order differs from the single-GPU loop: poses agree to ~1e-6, not bit for bit.
 * With a communicator attached (lslam_ctx_set_comm) fn and xchg32 may be NULL: the sums are then
 * all-reduced by RCCL on the library's stream and the whole loop stays device-resident. */
int lslam_scanmatch_run_sharded(lslam_ctx *ctx, float pose[6], const lslam_opts *opts,
                                lslam_allreduce_fn fn, void *user, double *xchg32,
                                lslam_stats *stats);

/* ---- joint LiDAR + stereo term (BASELINE configs[4]) ------------------
 *
 * The reference only announces this (README.md:51-71: ORB-SLAM2 on a ZED stereo camera, "planning
 * to extend the LOAM module to integrate Lidar and Visual SLAM methods"): it holds no code for a
 * visual term, so there is nothing to cite line by line and PARITY IS UNPINNED.  The
 * arithmetic restated here (and in oracle/lslam_oracle.c) is the published one of ORB-SLAM2's
 * pose-only stereo edge (g2o EdgeStereoSE3ProjectXYZOnlyPose as used by
 * Optimizer::PoseOptimization): a landmark X_w (map frame) seen at (uL, v, uR) projects as
 *   X_c = R_cl * (R^T (X_w - t)) + t_cl          (R, t: the Twist being optimised, sensor -> map)
 *   uL' = fx x/z + cx,  v' = fy y/z + cy,  uR' = uL' - bf/z
 * error e = (uL'-uL, v'-v, uR'-uR), chi2 = |e|^2 * inv_sigma2, Huber weight with
 * delta = sqrt(7.815) (sqrt(5.991) for a monocular observation, uR < 0: two rows), optional
 * outlier gate chi2 > delta^2.  Its rows, scaled by sqrt(weight * inv_sigma2 * w_huber), are added
 * to the LOAM rows of ScanMatch.cpp:134-204 in the SAME 6x6 A^T A / A^T b of every Gauss-Newton
 * iteration (Jacobian taken with respect to the same six Twist parameters), followed by the same
 * solve / degeneracy / convergence steps (ScanMatch.cpp:206-260). */
typedef struct {
  float fx, fy, cx, cy;   /* rectified pinhole intrinsics */
  float bf;               /* stereo baseline times fx (ORB-SLAM2's mbf) */
  float T_cl[12];         /* camera-from-lidar rigid transform, row-major 3x4 [R_cl | t_cl] */
  float weight;           /* lambda: scale of the stereo block against the LiDAR block */
  float huber_stereo;     /* sqrt(7.815) */
  float huber_mono;       /* sqrt(5.991) */
  int32_t gate_outliers;  /* 1: skip observations whose chi2 exceeds delta^2 at the current pose */
  float min_depth;        /* observations with camera z <= min_depth are skipped */
} lslam_stereo_cam;
void lslam_stereo_default_cam(lslam_stereo_cam *cam);
/* Makes n observations resident on the context: landmarks_xyz[n][3] (map frame),
 * obs[n][3] = (uL, v, uR; uR < 0: monocular), inv_sigma2[n] (NULL: all 1).  From then on
 * lslam_scanmatch_run / _scan / _run_sharded of a SINGLE resident scan assemble the joint
 * system (under _run_sharded each rank holds its own shard of the observations; the stereo sums
 * travel in the same 32-double all-reduce).  n = 0 removes the term. */
int lslam_stereo_set(lslam_ctx *ctx, const float *landmarks_xyz, const float *obs, const float *inv_sigma2,
                     size_t n, const lslam_stereo_cam *cam);
/* Removes the term, whichever form set it. */
int lslam_stereo_clear(lslam_ctx *ctx);
/* Parity tap: the stereo term alone at `pose`: sums32 = {21 upper-triangular A^T A, 6 A^T b,
 * rows, 0, 0, 0, observations used} (fp64 reduction of the per-block fp32 partials).  A term of
 * more than one set is refused: lslam_stereo_sums_batch. */
int lslam_stereo_sums(lslam_ctx *ctx, const float pose[6], double sums32[32]);
/* The joint system for a batch of resident scans (keyframe re-matching, loop candidates): K
 * observation sets, one per resident scan, packed: set p is observations
 * [offsets[p], offsets[p+1]) of landmarks_xyz[n][3] / obs[n][3] / inv_sigma2[n] (NULL: all 1),
 * offsets[0] = 0, offsets[K] = n, non-decreasing.  One camera for all sets.  An empty set leaves
 * its scan LiDAR-only.  n = 0 removes the term.  lslam_stereo_set is the case K = 1; setting one
 * form replaces the other.  At run time K must equal the number of resident scans
 * (lslam_scanmatch_run_batch; _run, _scan and _run_sharded take K = 1 only), otherwise the call
 * returns LSLAM_ERR_INVALID and nothing changes.  Scan p of the batch gives, bit for bit, what it
 * gives matched alone with set p through lslam_stereo_set. */
int lslam_stereo_set_batch(lslam_ctx *ctx, int32_t n_sets, const float *landmarks_xyz, const float *obs,
                           const float *inv_sigma2, const size_t *offsets, const lslam_stereo_cam *cam);
/* Parity tap: each set's stereo term alone at its own pose -> sums32[K][32] (layout of lslam_stereo_sums). */
int lslam_stereo_sums_batch(lslam_ctx *ctx, int32_t n_sets, const float *poses, double *sums32);

int lslam_pg_create(int device, int32_t n_vertices, const double *poses7, int32_t n_edges,
                    const int32_t *ij, const double *meas7, const double *info36,
                    int32_t fixed_vertex, lslam_pg **out);
void lslam_pg_destroy(lslam_pg *pg);
const char *lslam_pg_last_error(void);
/* Edge shard [e_begin, e_end) of this rank; fn == NULL: single GPU.  system_buf: optional
 * caller-owned DEVICE buffer of lslam_pg_system_doubles() doubles to assemble into.
 * Unary constraints (lslam_pg_set_priors, further down) are not sharded: the rank whose range starts at 0 and is not empty
 * carries all of them, every other rank none, so the sum over the ranks counts each once. */
int lslam_pg_set_shard(lslam_pg *pg, int32_t e_begin, int32_t e_end, lslam_allreduce_fn fn,
                       void *user, double *system_buf);
/* The same with the library's own RCCL communicator instead of a callback (NULL detaches). */
int lslam_pg_set_comm(lslam_pg *pg, lslam_comm *comm);
size_t lslam_pg_system_doubles(const lslam_pg *pg);
/* ONE solve shared by the ranks (large graphs: the replicated solve above does not get faster with more GPUs).  Every rank also
 * takes a range of vertex ROWS [v_begin, v_end) -- whole 21-vertex row blocks, lslam_pg_row_shard_range gives an even
 * partition -- and the damped system is then solved by a row-sharded block-Jacobi PCG: each rank multiplies, updates and
 * preconditions its own rows; per iteration the ranks exchange one scalar (p . A p) and the vector z with r . z, r . r behind it
 * (each rank's rows in a zero-padded buffer of 6 n + 2 doubles: its all-reduce IS the gather; or a true all-gather, see
 * lslam_pg_set_row_gather below), through the same transport as
 * the linearisation (callback or RCCL communicator; the buffer is the tail of the system buffer).  Same iterates as the
 * single-process block-Jacobi solve up to the order of the sums.  The dense second level of the preconditioner is a
 * single-device structure: it is not used (and does not switch itself on) in this mode; with LSLAM_PG_COARSE=1 the solve
 * stays replicated.  (-1, -1) returns to the replicated solve. */
void lslam_pg_row_shard_range(int32_t n_vertices, int32_t rank, int32_t world, int32_t *v_begin, int32_t *v_end);
int lslam_pg_set_row_shard(lslam_pg *pg, int32_t v_begin, int32_t v_end);
int32_t lslam_pg_row_sharded_solves(const lslam_pg *pg); /* damped solves that took the row-sharded form so far */
/* The exchange of z as an ALL-GATHER of the owned segments instead of the zero-padded all-reduce (half the bytes on the wire,
 * no zeroing pass): taken whenever every rank's rows are lslam_pg_row_shard_range's partition -- each rank can then name every
 * segment without asking -- and the transport can gather.  The RCCL communicator (lslam_pg_set_comm) can: one ncclBroadcast per
 * segment rooted at its owner, all in one group = one launch; each rank's parts of r . z and r . r travel in the same group
 * and are summed in rank order on every rank (same bits everywhere).  A host with its own transport registers a second
 * callback type: in-place, segment r of buf = doubles [offsets[r], offsets[r + 1]), valid on rank r on entry and on every
 * rank on return; complete when it returns.  Ranges that are not the canonical partition, or no gather transport: the
 * all-reduce form.  Which form is taken is ONE decision of all ranks, taken by every row-sharded solve: each rank sums a
 * "not from me" flag over the ranks -- raised without a gather transport or with a range that is not the canonical one -- (one
 * scalar all-reduce through the linearisation's transport) and follows the result: a rank cannot see the others' ranges or
 * transports, and every rank takes part in that sum whatever its own setting.  At most 64 ranks. */
typedef void (*lslam_allgatherv_fn)(void *user, double *buf, const int64_t *offsets, int32_t world);
int lslam_pg_set_row_gather(lslam_pg *pg, lslam_allgatherv_fn fn, void *user, int32_t rank, int32_t world);
int32_t lslam_pg_row_gathered_solves(const lslam_pg *pg); /* ... of which exchanged by all-gather */
int32_t lslam_pg_num_offdiag(const lslam_pg *pg);
/* Relative residual |r| / |b| at which a damped solve's PCG stops.  Default 1e-8: to the LM schedule the solves are then what
 * g2o's direct factorisation ("lm_var", solver_g2o.cpp:16) gives it -- the trajectory of iterates is the oracle's.  A looser
 * value is an inexact Levenberg-Marquardt: fewer PCG iterations per solve, a different trajectory (accept / reject decisions
 * move), the same optimum -- on the bench graph 1e-3 ends at the same chi2 to 1e-6 relative and the same keyframe positions
 * to 1e-4 m in a comparable number of iterations at about twice the rate (tests/test_posegraph_bench_fixture.py; bench.py
 * reports it next to the default, never instead of it). */
int lslam_pg_set_solve_tolerance(lslam_pg *pg, double rel_tol);
/* SolverG2O::optimize (solver_g2o.cpp:79-95): up to max_iters LM iterations. */
int lslam_pg_optimize(lslam_pg *pg, int32_t max_iters, lslam_pg_stats *stats);
int lslam_pg_get_poses(lslam_pg *pg, double *poses7);
/* One-call form: poses7 is in/out; single GPU. */
int lslam_posegraph_optimize(int device, int32_t n_vertices, double *poses7, int32_t n_edges, const int32_t *ij,
                             const double *meas7, const double *info36, int32_t fixed_vertex, int32_t max_iters,
                             lslam_pg_stats *stats);
/* SolverG2O::save (solver_g2o.cpp:97-100): the graph with its current estimates in g2o's text
 * format (VERTEX_SE3:QUAT / FIX / EDGE_SE3:QUAT with the 21 upper-triangular information
 * entries) -- the route to cross-check this solver against an external g2o. */
int lslam_pg_save_g2o(lslam_pg *pg, const char *path);
/* Reader for that format (host only).  *n_vertices / *n_edges: in = capacity of the arrays, out =
 * what the file holds (call with NULL arrays to size them); vertex ids are renumbered 0..n-1 in
 * order of appearance; *fixed_vertex = first FIX id or -1. */
int lslam_g2o_read(const char *path, int32_t *n_vertices, double *poses7, int32_t *n_edges, int32_t *ij,
                   double *meas7, double *info36, int32_t *fixed_vertex);
/* Parity taps: the assembled system at the current estimate (diag[n_v*36],
 * off[n_off*36] with its (i<j) pairs off_ij[n_off*2], b[n_v*6], chi2), and one damped
 * solve (H + lambda I) dx = b. Any output may be NULL. */
int lslam_pg_linearize(lslam_pg *pg, double *diag_out, double *off_out, int32_t *off_ij_out,
                       double *b_out, double *chi2_out);
int lslam_pg_solve(lslam_pg *pg, double lambda, double *dx_out, int32_t *cg_iters);

/* ---- robust kernels on pose-graph edges ------------------------------------------------------------------------------
 * The reference only shows the intent (pose_graph/solver_g2o.h:25-26 includes g2o's robust-kernel headers, solver_g2o.cpp:27-28
 * fills and prints the kernel factory, information_estimator.hpp has a weight() nobody calls): no edge there carries a kernel,
 * and g2o itself is not pinned by it, so PARITY IS UNPINNED like the rest of this solver.  The semantics are g2o's published
 * ones (BaseBinaryEdge::constructQuadraticForm, robust_kernel_impl.cpp).  With e2 = e^T Omega e and the kernel parameter delta,
 * rho = (rho0, rho1):
 *   NONE    (e2, 1)
 *   HUBER   e2 <= delta^2: (e2, 1), else (2 delta sqrt(e2) - delta^2, delta / sqrt(e2))
 *   CAUCHY  a = e2 / delta^2 + 1: (delta^2 ln a, 1 / a)
 *   DCS     s = 2 delta / (delta + e2): s >= 1: (e2, 1), else (s^2 e2, s^2)   -- rho1 is g2o's, not d rho0 / d e2
 * The edge adds rho1 J^T Omega J to H, -rho1 J^T Omega e to b and rho0 to chi2 (the second-order rho2 term is dropped, as g2o
 * drops it).  lslam_pg_optimize then runs its unchanged schedule on the sum of rho0 (g2o's activeRobustChi2): chi2_initial,
 * chi2_final and every accept / reject decision; lslam_pg_linearize returns the weighted system and that sum.  A sharded run
 * needs nothing more: each rank weights its own edges (every rank sets the same arrays, indexed by global edge id).
 * Huber is convex: it bounds an outlier's pull but cannot reject it.  Cauchy and DCS can (DESIGN, pose-graph section).
 * While no edge carries a kernel -- the default -- the solver launches exactly the kernels it launched before these entry points
 * existed.  The .g2o text format has no place for a kernel: lslam_pg_save_g2o writes none, a graph read back has plain edges. */
enum { LSLAM_PG_KERNEL_NONE = 0, LSLAM_PG_KERNEL_HUBER = 1, LSLAM_PG_KERNEL_CAUCHY = 2, LSLAM_PG_KERNEL_DCS = 3 };
/* "NONE" / "Huber" / "Cauchy" / "DCS" (the names the C++ mirrors take) -> LSLAM_PG_KERNEL_*; anything else -1. */
int lslam_pg_kernel_from_name(const char *name);
/* kind[n_edges], delta[n_edges] (delta ignored where kind is NONE); (NULL, NULL) clears: the plain solver again.  A delta that
 * is not finite and > 0, an unknown kind, or one array without the other: LSLAM_ERR_INVALID, lslam_pg_last_error says which,
 * and nothing has changed. */
int lslam_pg_set_robust_kernels(lslam_pg *pg, const int32_t *kind, const double *delta);
/* per edge at poses7 (NULL: the current estimate); any output may be NULL: e2[n_edges], rho[n_edges] = rho0, weight[n_edges] = rho1 */
int lslam_pg_edge_robust(lslam_pg *pg, const double *poses7, double *e2, double *rho, double *weight);
/* edges carrying a kernel; of those, edges with weight < 1 at the current estimate; the plain sum of e2 */
int lslam_pg_robust_info(lslam_pg *pg, int32_t *n_robust, int32_t *n_downweighted, double *chi2_plain);

/* ---- unary constraints on keyframes: GPS position and absolute-pose priors --------------------------------------------
 * The reference shows the intent and stops there: pose_graph/keyframe.h:40-41 gives every keyframe an optional utm_coord ("UTM
 * coord obtained by GPS") and imu_quat, kf_fusion/fpdReceiver.cpp and utmProjection.cpp produce the fixes,
 * map_evaluation/Evaluation.cpp scores the lidar pose against them -- and nothing consumes the two keyframe fields.  The module
 * is modelled on hdl_graph_slam, where they become unary edges (EdgeSE3PriorXYZ, EdgeSE3PriorQuat).  Neither hdl_graph_slam nor
 * g2o is under the reference, so PARITY IS UNPINNED like the rest of this solver; the semantics are their published ones, in
 * this solver's conventions (update X <- X * fromVectorMQT(d), error in toVectorMQT coordinates).  A prior sits on one vertex v
 * with estimate X = (t, q):
 *   LSLAM_PG_PRIOR_XYZ   a GPS fix: e = t - z in the graph frame (3 rows), J = [R(q) | 0]; the information is the upper-left
 *                        3x3 of info36, the rest is ignored; of meas7 only x, y, z are read
 *   LSLAM_PG_PRIOR_POSE  an absolute pose: e = toVectorMQT(Z^-1 X) (6 rows), the binary edge's error with Xi = identity, 6x6
 *                        information.  Positive SEMI-definite information is legal: a zero translation block makes it an
 *                        orientation prior (keyframe.h:41's imu_quat), only z / roll / pitch entries a ground-plane prior.
 * A prior adds J^T Omega J to its vertex's diagonal block, -J^T Omega e to its segment of b and e^T Omega e to chi2: the
 * sparsity pattern, the PCG, the coarse level and the sharded layouts do not change.  With a robust kernel (kind / delta, the
 * LSLAM_PG_KERNEL_* semantics above: rho1 scales H and b, rho0 goes to chi2) an outlying fix -- GPS multipath -- can be
 * rejected.  Several priors on one vertex are legal; they are summed in prior order behind the vertex's edges (one fixed order,
 * no atomics).  A prior on the fixed vertex adds its rho0 to chi2 and nothing to H or b (g2o's behaviour for an active edge on
 * a fixed vertex).  Priors can fix the gauge: a graph created with fixed_vertex = -1 holds no vertex, and is well posed once its
 * priors pin all six degrees of freedom.
 * lslam_pg_linearize and lslam_pg_optimize include the priors; lslam_pg_robust_info and lslam_pg_edge_robust keep their meaning
 * (edges only).  While a graph has no priors -- the default -- the solver launches exactly the kernels it launched before these
 * entry points existed.
 * SHARDED RUNS (lslam_pg_set_shard): the system is summed over the ranks, so every prior must be counted once.  Every rank sets
 * the same priors; the rank whose edge range starts at 0 and is not empty linearises all of them, every other rank none.  No
 * new transport is needed.  (A graph without edges has nothing to shard: its one range [0, 0) carries the priors.) */
enum { LSLAM_PG_PRIOR_XYZ = 0, LSLAM_PG_PRIOR_POSE = 1 };
/* Replaces the whole set; n_priors = 0 clears.  vertex[n], type[n], meas7[n][7] = {x, y, z, qx, qy, qz, qw}, info36[n][36]
 * row-major; kind[n] / delta[n] as lslam_pg_set_robust_kernels, both NULL: no kernels.  Everything is checked before anything
 * changes -- LSLAM_ERR_INVALID, lslam_pg_last_error names the cause, for: a vertex out of range, an unknown type, a non-finite
 * measurement, a zero-norm quaternion on a POSE prior, a used information block that is not finite, not symmetric (beyond 1e-12
 * of its largest entry) or has a negative diagonal entry, kind without delta or the reverse, an unknown kind, a delta that is
 * not finite and > 0.  A POSE prior's quaternion need not be unit: it is normalised before it reaches the device (the file
 * lslam_pg_save_g2o writes carries it as given).  A device error (LSLAM_ERR_HIP) while the new set is uploaded leaves the graph
 * with no priors. */
int lslam_pg_set_priors(lslam_pg *pg, int32_t n_priors, const int32_t *vertex, const int32_t *type, const double *meas7,
                        const double *info36, const int32_t *kind, const double *delta);
int32_t lslam_pg_num_priors(const lslam_pg *pg);
/* per prior at poses7 (NULL: the current estimate); any output may be NULL: e2[n_priors], rho[n_priors] = rho0, weight[n_priors] = rho1 */
int lslam_pg_prior_robust(lslam_pg *pg, const double *poses7, double *e2, double *rho, double *weight);
/* lslam_pg_save_g2o writes the priors behind the edges: one "PARAMS_SE3OFFSET 0 0 0 0 0 0 0 1" line when a POSE prior exists,
 * "EDGE_SE3_PRIOR v 0 <meas7> <21 upper-triangular>" per POSE prior (g2o's own tag) and "EDGE_SE3_PRIORXYZ v x y z <6
 * upper-triangular>" per XYZ prior (hdl_graph_slam's tag); robust kernels have no place in the format.  lslam_g2o_read ignores
 * these lines; this reader returns them, in file order (host only).  *n_priors: in = capacity of the arrays, out = what the file
 * holds (call with NULL arrays to size them); vertices are numbered as lslam_g2o_read numbers them. */
int lslam_g2o_read_priors(const char *path, int32_t *n_priors, int32_t *vertex, int32_t *type, double *meas7,
                          double *info36);

/* ---- plane priors: a plane known in the graph frame, measured in a keyframe's sensor frame ------------------------------------
 * The reference shows the intent and stops there (pose_graph/solver_g2o.h:61-65 add_plane_node commented out, :92 the floor
 * plane node, :42 g2o's plane types; graph.cpp:321 "floor coeffs").  The module is modelled on hdl_graph_slam's floor
 * constraint.  Neither hdl_graph_slam nor g2o is under the reference, so PARITY IS UNPINNED like the rest of this solver; the
 * semantics are this project's own, in this solver's conventions (update X <- X * fromVectorMQT(d)).  A POSE prior with only
 * z / roll / pitch information is NOT this constraint: its error's coordinates turn with yaw, a plane seen from the sensor does not.
 * A plane prior sits on one vertex v with estimate X = (t, R), R sensor -> graph.  world4 = (n_w, d_w) is the plane in the graph
 * frame, meas4 = (n_m, d_m) the plane measured in the sensor frame (n.p + d = 0; both are scaled to unit normals before they
 * reach the device).  The world plane in the sensor frame: n_l = R^T n_w, d_l = d_w + n_w.t.  Tangent basis of n_m: a = the unit
 * axis of the smallest |n_m| component (the lowest index among equals), b1 = normalise(n_m x a), b2 = n_m x b1.
 *   e = (b1.n_l, b2.n_l, d_l - d_m)          3 rows
 *   J = rows 0, 1: [0 | 2 (b_k x n_l)^T], row 2: [n_l^T | 0]
 *   Omega = info9, 3x3 row-major in (tangent 1, tangent 2, distance) coordinates; positive SEMI-definite is legal
 * It adds rho1 J^T Omega J to its vertex's diagonal block, -rho1 J^T Omega e to its segment of b and rho0 to chi2 (kind / delta:
 * the LSLAM_PG_KERNEL_* semantics): the sparsity pattern, the PCG and the sharded layouts do not change.  In the per-vertex sum
 * the plane priors follow the vertex's edges and its POSE / XYZ priors, in plane-prior order (one fixed order, no atomics).  On
 * the fixed vertex a plane prior adds its rho0 to chi2 only.  lslam_pg_linearize and lslam_pg_optimize include them; sharded runs
 * follow the priors' rule (every rank sets the same set, the rank whose edge range starts at 0 linearises all of it).  This set
 * is separate from lslam_pg_set_priors': lslam_pg_num_priors, lslam_pg_prior_robust and lslam_g2o_read_priors keep their meaning.
 * While a graph has no plane priors -- the default -- the solver launches exactly the kernels it launched before. */
/* Replaces the whole set; n_priors = 0 clears.  vertex[n], world4[n][4], meas4[n][4], info9[n][9]; kind[n] / delta[n] as
 * lslam_pg_set_priors.  Everything is checked before anything changes -- LSLAM_ERR_INVALID, lslam_pg_last_error names the
 * cause, for: a vertex out of range, a plane that is not finite or has a zero normal, information that is not finite, not
 * symmetric (beyond 1e-12 of its largest entry) or has a negative diagonal entry, kind without delta or the reverse, an unknown
 * kind, a delta that is not finite and > 0, and a pair whose normals lie in opposite hemispheres at the vertex's current
 * estimate (n_l.n_m < 0: one of the planes is given upside down).  A device error while the new set is uploaded leaves the
 * graph with no plane priors. */
int lslam_pg_set_plane_priors(lslam_pg *pg, int32_t n_priors, const int32_t *vertex, const double *world4, const double *meas4,
                              const double *info9, const int32_t *kind, const double *delta);
int32_t lslam_pg_num_plane_priors(const lslam_pg *pg);
/* per plane prior at poses7 (NULL: the current estimate); any output may be NULL: e2[n], rho[n] = rho0, weight[n] = rho1 */
int lslam_pg_plane_prior_robust(lslam_pg *pg, const double *poses7, double *e2, double *rho, double *weight);
/* lslam_pg_save_g2o writes the plane priors behind the other priors, one line each with THIS PROJECT'S OWN tag (no g2o or
 * hdl_graph_slam type reads it): "EDGE_SE3_PRIOR_PLANE v <world4> <meas4> <6 upper-triangular>", the planes as given.
 * lslam_g2o_read and lslam_g2o_read_priors skip these lines; this reader returns them, in file order (host only), with the
 * two-call pattern and the vertex numbering of lslam_g2o_read_priors. */
int lslam_g2o_read_plane_priors(const char *path, int32_t *n_priors, int32_t *vertex, double *world4, double *meas4, double *info9);

/* ---- marginal covariances of pose-graph vertices ----------------------------------------------------------------------------
 * What g2o's computeMarginals offers the reference's solver: selected blocks of H^-1, H being the system lslam_pg_linearize
 * exports at the CURRENT estimate (robust weights, priors, plane priors and the identity row of the fixed vertex included),
 * at lambda = 0.  The 6 unit columns of every listed vertex are solved for on the device by a preconditioned CG that works
 * on PANELS of 60 columns: per iteration the block system is read once per panel, every column keeps its own step lengths,
 * residual and done flag, a converged column is frozen, and every sum has a fixed order -- a vertex's blocks are THE SAME
 * BITS whether it is asked for alone or in a long list, first or last, once or twice in the list, now or in a second call.
 *
 * COORDINATES: the solver's own increment coordinates -- those dx of lslam_pg_solve is in and an accepted step applies
 * (X <- X * [dt, dq]): BODY-frame translation [m] first, then the vector part of the unit quaternion, which is HALF the rotation
 * angle [rad] -- multiply the rotational rows and columns by 2 for an angle covariance.  Blocks are 6x6 row-major.
 *
 * cov36[k] is the diagonal block of vertices[k], returned symmetrised, 1/2 (X + X^T), hence bit-symmetric; cross36 (may be
 * NULL) is [n_q][n_q][36] with cross36[a][b] = Cov(vertices[a], vertices[b]), cross36[b][a] its exact transpose and
 * cross36[a][a] = cov36[a].  The fixed vertex has zero covariance: its block and its cross blocks are exact zeros (its
 * block of H^-1 is the identity by construction of the row and is not reported).
 *
 * LSLAM_ERR_INVALID, with nothing written and lslam_pg_last_error saying why, for: a vertex out of range; a queried vertex
 * whose connected component holds neither the fixed vertex nor any unary constraint (no gauge: the block is not defined); a
 * column that does not reach the tolerance within max_iters (a component held by plane priors alone, for example -- the
 * message names the vertex); a sharded graph (lslam_pg_set_shard, _set_comm, _set_row_shard); coarse = 1 on a graph too large
 * for the dense second level.  The graph itself is left as lslam_pg_linearize leaves it and optimises as before. */
typedef struct {
  double rel_tol;     /* |r|/|e| per column; 0: the solver's own default (1e-8, lslam_pg_set_solve_tolerance) */
  int32_t max_iters;  /* 0: 6 n_v, CG's exact-arithmetic bound, but at least 100.  In fp64 block-Jacobi PCG can need several times
                       * that on a small ill-conditioned graph (a 22-keyframe chain with random rotations: 214 on the device): the
                       * call then fails with LSLAM_ERR_INVALID and the caller passes a larger cap, or coarse = 1 on a large graph */
  int32_t coarse;     /* -1: as the graph's solves decide, 0: block-Jacobi only, 1: two-level */
} lslam_pg_marginal_opts;

typedef struct {
  int32_t columns, panels, iters_max, iters_sum, coarse_used; /* columns: 6 per DISTINCT vertex asked for, the reference vertex of lslam_pg_relative_covariances included; iters_sum: over the columns solved */
  double worst_rel_residual;
} lslam_pg_marginal_stats;

/* opts NULL: {0, 0, -1}; stats may be NULL. */
int lslam_pg_marginals(lslam_pg *pg, int32_t n_q, const int32_t *vertices, const lslam_pg_marginal_opts *opts,
                       double *cov36 /* [n_q][36] */, double *cross36 /* NULL, or [n_q][n_q][36] */,
                       lslam_pg_marginal_stats *stats);
/* Covariance of the RELATIVE pose X_ref^-1 X_j for j = vertices[k], in the coordinates of an edge error (translation in the
 * frame of ref, quaternion vector):  S_rel = [J_r J_j] S_(r,j) [J_r J_j]^T  with S_(r,j) the joint 12x12 marginal and J_r, J_j
 * the Jacobians the solver's own edge has for an edge (ref, j) whose measurement is the current relative pose, evaluated on
 * the device by the edge's device function; the 6x6 products run on the host in fp64.  Symmetrised; j == ref gives exact
 * zeros.  Costs the 6 columns of ref once plus 6 per distinct query.  Errors as lslam_pg_marginals. */
int lslam_pg_relative_covariances(lslam_pg *pg, int32_t ref, int32_t n_q, const int32_t *vertices,
                                  const lslam_pg_marginal_opts *opts, double *cov36 /* [n_q][36] */,
                                  lslam_pg_marginal_stats *stats);
/* Test tap: the six columns of H^-1 of one free vertex as the panel solve left them -- x[6 n_v][6] row-major, every row,
 * nothing symmetrised or zeroed -- so that a test can form the true residual H x - e.  Errors as lslam_pg_marginals. */
int lslam_debug_pg_marginal_columns(lslam_pg *pg, int32_t vertex, const lslam_pg_marginal_opts *opts, double *x /* [6 n_v][6] */,
                                    lslam_pg_marginal_stats *stats);

/* Device handle tap, as lslam_stream: the stream every kernel of this graph runs on (hipStream_t), for harnesses that time a
 * linearisation with events (tools/bench_robust_linearize.py). */
void *lslam_pg_stream(lslam_pg *pg);

/* Device handle taps for harnesses that time on the library's stream. */
void *lslam_stream(lslam_ctx *ctx); /* hipStream_t */
/* Sweep launches of this context so far, per kernel instantiation: [0] whole stack in LDS, [1] the same with the HBM
 * overflow (trees deeper than 33 levels), [2] the shallow-stack batch kernel sweep_kernel<256,true,false,12>, [3] per-cube
 * trees, [4] per-cube trees with overflow, [5] packet search.  [6] and [7] counted two retired kernels (the persistent
 * Gauss-Newton loop, the solve fused into the sweep's tail): the slots keep their places and always read 0. */
void lslam_debug_sweep_launches(lslam_ctx *ctx, uint64_t counts[8]);
/* ... and of the grid sweep (sweep_grid_kernel; LSLAM_SEARCH_GRID) */
uint64_t lslam_debug_grid_launches(lslam_ctx *ctx);
/* ... of which those that took the lean instantiation (sweep_grid_kernel<256, false, false, true>: the production loop's launch) */
uint64_t lslam_debug_grid_lean_launches(lslam_ctx *ctx);
/* ... of which those whose second pass took ITS lean instantiation (sweep_queue_kernel<256, true, 12, 1, true>; LSLAM_QUEUE_LEAN=0
   in the environment a context is made in keeps the general one) */
uint64_t lslam_debug_queue_lean_launches(lslam_ctx *ctx);
/* ... of the lean ones, those that took the instantiation with the in-range fit (sweep_grid_kernel<256, true, *, true>, and
   sweep_queue_kernel<256, true, 12, 1, true, true> where the second pass is lean; LSLAM_FIT_INRANGE=0 in the environment a
   context is made in, or a build with -DLSLAM_FIT_INRANGE_DEFAULT=0, keeps `/` and sqrtf in the lean kernels' fit) */
uint64_t lslam_debug_fit_inrange_launches(lslam_ctx *ctx);
/* The in-range fit's parts on their own (for the tests).  _ops: for n operand pairs out8[8 i ..] = div_inrange(a, b), a / b,
 * sqrt_inrange(a), sqrtf(a), the guard's verdict on a and b (an int32 in a float's place: bits 0, 1), the refined reciprocal of
 * b, the literal the divisions by 5 start from, div_inrange(a, 5).  _fits: one plane fit (is_surf) or line fit with its
 * coefficient per element, on five neighbours nb_xyzw[20 i ..] and the point x_xyzw[4 i ..], in range and as every other kernel
 * fits: out_*8[8 i ..] = plane[4] (or A[3], B[0]) and coeff[4]; flags[i]: bits 0 / 1 the coefficient kept (in range / general),
 * bits 2 / 3 the fit matched, bit 4 the plane fit's guard refused an operand. */
int lslam_debug_fit_inrange_ops(lslam_ctx *ctx, const float *a, const float *b, size_t n, float *out8);
int lslam_debug_fit_inrange_fits(lslam_ctx *ctx, const float *nb_xyzw, const float *x_xyzw, size_t n, int32_t is_surf, float *out_inr8, float *out_gen8,
                                 int32_t *flags);
/* The whole fit of the same elements (for the tests that hold it to float64: tests/fit_ref.py): out_*12[12 i ..] = A[3], B[3], 0, 0,
 * coeff[4] of a line fit, plane[4], 0, 0, 0, 0, coeff[4] of a plane fit; inputs and flags as lslam_debug_fit_inrange_fits has them.
 * A fit that did not match leaves its coefficient zero. */
int lslam_debug_fit_stage(lslam_ctx *ctx, const float *nb_xyzw, const float *x_xyzw, size_t n, int32_t is_surf, float *out_inr12, float *out_gen12,
                          int32_t *flags);
/* ... of which those whose first pass read the x-subdivided cell tables (LSLAM_AB_GRID_CUBIC), lean or general */
uint64_t lslam_debug_grid_fine_launches(lslam_ctx *ctx);
/* the x-subdivided tables of the resident map: out[0], out[1] sub-cells per cell used (corner, surf; lowered where the table's
 * limits ask for it), out[2], out[3] their cells; build_ms (or null): host time of their one build.  All 0 while there are none
 * (no call has wanted them, the trees are deferred, the switch is off). */
void lslam_debug_grid_fine_info(lslam_ctx *ctx, uint64_t out[4], float *build_ms);
/* Debug export of one of them (which_map 0: corner, 1: surf), after building it once more when `rebuild` is set: dims_out =
 * {nx (sub-cells), ny, nz, sub-cells per cell}, geom_out = {org x, y, z, cell edge, inv_cx}, the first cap_cells words of
 * cell_start[nx ny nz + 1], the first cap_pts cell-sorted points {x, y, z, bitcast(original index)}.  Any output may be null.
 * Returns the number of points, or a negative LSLAM_ERR_* (LSLAM_ERR_INVALID: the map has no such table). */
int lslam_debug_grid_fine_table(lslam_ctx *ctx, int which_map, int32_t rebuild, int32_t dims_out[4], float geom_out[5],
                                uint32_t *cell_start_out, size_t cap_cells, float *pts_out, size_t cap_pts);
/* (counted a retired single-launch form for a map without trees: always 0) */
uint64_t lslam_debug_grid_wide_launches(lslam_ctx *ctx);
/* cells of the resident map's two cell tables (corner, surf); 0 while a type has no grid */
void lslam_debug_grid_cells(lslam_ctx *ctx, uint64_t out[2]);
/* out[0] maps set with deferred trees, out[1] of those whose trees were built after all, out[2] 1 while the resident map's are pending */
void lslam_debug_lazy_trees(lslam_ctx *ctx, uint64_t out[3]);
/* Debug tap of the certificate sweep (csrc/lslam_kernels.hip sweep_body): out[2] = second-pass launches of this
 * context since its creation; out[0] = points the certificate-testing workgroups left to the second pass and out[1] = points
 * of those workgroups, counted only when the process runs with LSLAM_DEBUG_CERT_STATS=1 (two atomics per workgroup). */
void lslam_debug_cert_stats(lslam_ctx *ctx, uint64_t out[3]);
/* ... and the grid sweep's (lslam_opts.debug_stats = 1 during the runs): out[((type * 8) + sweep) * 2 + {0, 1}] = points the
 * probe could not prove (left to the tree search) / points swept, by feature type (0 corner, 1 surf) and sweep of the
 * Gauss-Newton loop (0 = a loop's first sweep; slot 7 = the eighth and every later one).  Counted by the planner of the second
 * pass from the lists' lengths: the sweep kernel itself runs the same code with the tap on. */
void lslam_debug_grid_stats(lslam_ctx *ctx, uint64_t out[32]);
/* Test tap: what the certificate sweep carries per resident scan point after a lslam_scanmatch_run* that ran it -- the
 * map-frame position of the point's last SEARCH (q_xyz0: 4 floats per point, the fourth unused) and the lower bound taken
 * there of the squared distance of every map point outside its five neighbours (lb; 0: none).  Resident order: per scan its
 * corner points, then its surf points (each in the library's own order).  Returns the number of points copied (at most
 * cap_points) or a negative status. */
int lslam_debug_cert_state(lslam_ctx *ctx, float *q_xyz0, float *lb, size_t cap_points);

/* ---- the localisation node resident on the device (odometry/LaserLocalization.cpp over util/FeatureMap.h) ------------------
 * L_SLAM's second operating mode: a map built once (saveCloudToFiles / lslam_fmap_save) is loaded, every cube with at least five
 * points of a type gets its kd-tree ONCE (loadCloudFromFiles, FeatureMap.h:415-462, builds them at :438,453), and every later
 * sweep is matched against it by FeatureMap::scanMatchScan (:490-691): a scan point is searched in the tree of the cube it
 * falls into, whichever loaded cube that is.  The node owns its map, its trees and its scratch; it never touches the
 * context's resident map (lslam_map_set / lslam_cubemap_set on the same context in between change nothing for it, and it
 * changes nothing for them).  One call in flight per ctx, like everything else on a ctx.
 *
 * The search.  What variant C fixes is the RESULT of nearestKSearch in the query's cube tree.  A cell grid over the cubes the
 * sensor can reach (those within lidar-valid-distance of the sensor's cube, fewer if the cell tables would not hold them)
 * proves, for most points, the five nearest among ALL points of those cubes with a margin to the sixth (csrc/lslam_grid.hpp);
 * when the proven five all belong to the query's own cube they are the five nearest inside it, in the same order.  A point the
 * probe cannot prove (a sparse neighbourhood, an exact tie among its six nearest), whose five are not all in its cube, or whose
 * cube the grid does not cover is searched in its cube's tree.  A point farther than the sqrt(5) m gate from every grid point
 * of a covered cube is rejected as the reference rejects it.  The grid is rebuilt only when the sensor's cube changes.
 *
 * Differences from the reference, on purpose:
 *   - FeatureMap::update shifts the cube array when the sensor comes within 3 cubes of the grid's edge but leaves the kd-tree
 *     arrays where they were (shift(), :353-376, swaps clouds only): what it then matches against is an accident.  A sweep
 *     whose prior pose is that close to the edge is refused with LSLAM_ERR_INVALID and leaves the node as it was.  (With an
 *     initial pose pending such a sweep is not matched -- its result would be discarded anyway -- and only takes the pose.)
 *   - prepareFeatureSurround only feeds a publisher in this node: it is not run per sweep (lslam_loc_get_surround does it).
 *   - the UKF (imu_que) is not part of the node: pose, velocity and stamp are what imu_que.correct would be handed. */
typedef struct lslam_loc lslam_loc;
/* lslam_loc_process flags */
enum { LSLAM_LOC_DROPPED = 1,        /* no initial pose yet (LaserLocalization.cpp:169): nothing was done, nothing changed */
       LSLAM_LOC_HAS_VELOCITY = 2,   /* velocity_out is valid (absent on the first processed sweep, :157) */
       LSLAM_LOC_POSE_RESET = 4,     /* a pending initial pose replaced this sweep's match result (:142-145) */
       LSLAM_LOC_VELOCITY_ZEROED = 8,/* |v| > 30 (:159-160) */
       LSLAM_LOC_SECOND_WAIT = 16    /* the scan filter's key range did not hold: the sweep was run again behind a second wait */ };
typedef struct {
  int64_t cubes_loaded[2];      /* cubes that hold points, per type (corner, surf) */
  int64_t cubes_with_tree[2];   /* ... of which have a kd-tree (>= 5 points) */
  uint64_t n_points[2];
  int64_t structure_builds;     /* forest builds since creation (one per map set / load) */
  int64_t grid_builds;          /* cell-grid builds since creation (one per change of the sensor's cube, both types together) */
  int32_t grid_cube[3];         /* the sensor cube the grids were built for */
  int32_t grid_reach;           /* cubes on every side of it the grids cover */
  int32_t grid_on[2];           /* 1 while the type has a grid (0: every point of the type goes to its cube tree) */
  int32_t tree_depth;           /* of the deepest cube tree */
  int32_t reserved;
} lslam_loc_map_stats;
typedef struct {                /* [0] the last sweep (all its Gauss-Newton iterations), [1] since creation */
  uint64_t swept[2];            /* points looked at (points whose cube has no tree included) */
  uint64_t grid_proven[2];      /* decided by the grid: five proven in the point's cube, or proven beyond the gate */
  uint64_t cube_refused[2];     /* proven by the grid but refused by the cube check alone */
  uint64_t to_trees[2];         /* searched in their cube's tree (cube_refused included) */
  uint64_t fallback_sweeps[2];  /* sweeps that fell back to the trees entirely (0: a tie sends only its own point to its tree) */
  uint64_t host_waits[2];
  uint64_t bytes_up[2], bytes_down[2];
} lslam_loc_search_counts;
/* FeatureMap(cubeWidth, cubeHeight, cubeDepth) of LaserLocalization's _feature_map; defaults: origin round((size-1)/2), cube
 * 50 m, valid distance 150 m, scan filters 1.0 / 1.0 (LaserMatcher.cpp:80-85), map filters 1.0 / 1.0 (:87-92,116). */
int lslam_loc_create(lslam_ctx *ctx, int32_t cube_width, int32_t cube_height, int32_t cube_depth, lslam_loc **out);
void lslam_loc_destroy(lslam_loc *loc);
int lslam_loc_setup_scan_filter_size(lslam_loc *loc, float corner, float surf);
int lslam_loc_setup_map_filter_size(lslam_loc *loc, float corner, float surf);   /* applied by lslam_loc_load / _set_map */
int lslam_loc_setup_world_origin(lslam_loc *loc, int32_t ox, int32_t oy, int32_t oz);
int lslam_loc_setup_world_cube_size(lslam_loc *loc, float size);
int lslam_loc_setup_lidar_valid_distance(lslam_loc *loc, float dist);
/* Debug switch: 0 = every point through its cube tree (the per-cube walk alone); 1 (default) = the grid path.  Same poses, bit for bit. */
int lslam_loc_setup_search(lslam_loc *loc, int32_t use_grid);
/* loadCloudFromFiles (FeatureMap.h:415-462) into an empty map: each listed cube through its type's VoxelGrid, a later entry
 * for a cube replaces the earlier one, a missing PCD is skipped; then every tree, in one forest build. */
int lslam_loc_load(lslam_loc *loc, const char *directory);
/* The same from host clouds: points pushed into their cubes in input order (as lslam_cubemap_set); filter != 0: every cube
 * through its type's VoxelGrid (the map filters) as the load does. */
int lslam_loc_set_map(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                      int32_t filter);
/* Adopt the map a mapping session has just built (same context, same cube-grid dimensions), device to device; cube size, origin
 * and valid distance are taken from it; nothing is filtered. */
int lslam_loc_set_map_from_fmap(lslam_loc *loc, lslam_fmap *fm);
int lslam_loc_info(lslam_loc *loc, lslam_loc_map_stats *out);
/* initialPoseHandler without its ROS sign conventions: T (row-major 4x4) becomes the pending pose and the node is initialised. */
int lslam_loc_set_initial_pose(lslam_loc *loc, const float T[16]);
/* LaserLocalization::process (:168-188) for one sweep: transformMerge on the host (lslam_transform_associate), both clouds
 * voxel-filtered on the device (lslam_voxel_grid2's arithmetic), scanMatchScan with <= 10 iterations, 0.05 / 0.05 and no score
 * gate, transformUpdate with its reset-after-match rule, the velocity (t_new - t_last) / dt in float.  One host wait.
 * mapped_out: _lidarMappedNew; stats: the match's (may be NULL).  Returns the match's outcome (LSLAM_OK / LSLAM_NOT_CONVERGED /
 * LSLAM_TOO_FEW_MATCHES; the pose is updated in every case, as the reference ignores scanMatchScan's result) or an error. */
int lslam_loc_process(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                      const float odom[16], int64_t stamp_ns, float mapped_out[16], float velocity_out[3], int32_t *flags,
                      lslam_stats *stats);
/* The same for clouds in the context's device memory, packed {x, y, z, intensity} (lslam_odom_last_view's). */
int lslam_loc_process_device(lslam_loc *loc, const void *d_corner, size_t n_corner, const void *d_surf, size_t n_surf,
                             const float odom[16], int64_t stamp_ns, float mapped_out[16], float velocity_out[3], int32_t *flags,
                             lslam_stats *stats);
/* prepareFeatureFrame + optimizeTransform alone, from a given Twist (in/out); the node's pose state is not touched. */
int lslam_loc_match(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                    float pose[6], lslam_stats *stats);
/* prepareFeatureSurround on request: FeatureMap::update at the node's pose + getSurroundFeature.  A null buffer: its count only. */
int lslam_loc_get_surround(lslam_loc *loc, float *corner_xyzi, size_t cap_corner, size_t *n_corner, float *surf_xyzi,
                           size_t cap_surf, size_t *n_surf);
int lslam_loc_search_stats(lslam_loc *loc, lslam_loc_search_counts *out);
/* Parity tap of the search the Gauss-Newton loop runs (the same kernels): nq queries in the map frame against the corner
 * (which = 0) or surf (1) structures -> the five neighbours' coordinates xyz_out[nq][5][3], their squared distances
 * d2_out[nq][5] and how each query was decided, how_out[nq]: 0 skipped (no cube, or a cube with < 5 points: outputs zero),
 * 1 grid, 2 cube tree.  Unlike the loop the tap has no gate: a query beyond sqrt(5) m of everything goes to its tree. */
int lslam_loc_debug_knn5(lslam_loc *loc, int32_t which, const void *queries, size_t nq, size_t stride_bytes, float *xyz_out,
                         float *d2_out, uint8_t *how_out);

/* ---- the paged mode of the localisation node (util/DynamicFeatureMap.h, the dynamicMode branch of LaserMatcher) --------------
 * A second mode of lslam_loc, entered with lslam_pmap_open in place of lslam_loc_load / _set_map*: the cube_width x
 * cube_height x cube_depth cubes of lslam_loc_create are a WINDOW addressed by GLOBAL cube index round(p / cube_size) that
 * follows the sensor.  update(sensor position) loads exactly the listed cubes that enter the window (index2.txt plus
 * <count>.pcd, each through its type's VoxelGrid with the map leaf, a kd-tree when at least five points remain); the cubes
 * that stay are not touched, the ones that left give their room back.  The match is the static mode's (same kernels, same
 * arithmetic) with the cube of a query looked up relative to the window centre.  The static mode is unchanged.  The entry
 * points of the window carry the prefix lslam_pmap_ and take the node's handle; lslam_loc_process / _process_device / _match /
 * _get_surround / _debug_knn5 / _info work in either mode (match updates the window at the Twist's translation first, the tap
 * searches the window as it stands, get_surround updates at the node's pose).
 *
 * A step on the device: the entering files' points in one upload with their segment numbers, one VoxelGrid run per feature type
 * over all entering cubes (lslam::voxel_filter_segments), their bounds and their placement into arena extents (pm_bounds_kernel,
 * pm_place_kernel), one forest build over the entering cubes only, the window tables rewritten from pinned memory.  Work and
 * bytes follow the entering cubes, not the window.  A step that is refused (capacity, LSLAM_ERR_TREE_DEPTH, a HIP error) has
 * changed nothing live: the node answers the next call as it did before.
 *
 * Differences from the reference, on purpose:
 *   - a query whose cube lies outside the window is skipped (the reference indexes _indexMap out of range);
 *   - an even window dimension and ceil(valid distance / cube size) > min(W, H, D) / 2 are refused (same reason);
 *   - the edge refusal of the static mode does not exist here;
 *   - lslam_index_convert writes every input line once (the reference's eof() loop repeats the last one);
 *   - addFeatureCloud / downsizeValidCloud / saveCloudToFiles / getFullMap are not built (DESIGN 8c says why). */
typedef struct {
  int32_t paged;                /* 1 once lslam_pmap_open succeeded */
  int32_t have_window;          /* 1 after the first update */
  int32_t centre[3];            /* sensorGloIdx of the last update */
  int32_t dims[3];
  int64_t steps;                /* updates that changed the window (the first included) */
  int64_t refused_steps;
  int64_t resident[2];          /* listed cubes in the window, per type (corner, surf) */
  int64_t resident_with_tree[2];
  int64_t staged[2];            /* cubes held in spare room by lslam_pmap_stage, not part of the window */
  int64_t entered[2], left[2], adopted[2];   /* of the last step; adopted: entered from the staged set instead of from disk */
  int64_t entered_total[2], left_total[2], adopted_total[2], staged_dropped_total[2];
  int64_t files_read, files_read_total;      /* PCDs read by the last step / since open (lslam_pmap_stage's reads included in the total) */
  int64_t files_missing, files_missing_total;/* listed but missing or unreadable: the cube stays empty */
  int64_t trees_built, trees_built_total;    /* kd-trees built by the last step / since open; a surviving cube's tree is never rebuilt */
  int64_t forest_builds_total;
  uint64_t bytes_uploaded, bytes_uploaded_total;  /* by the last step / by all steps and stagings */
  int32_t step_kernels;         /* of the last step: launches of its own kernels (bounds, placement) */
  int32_t step_filter_runs;     /* ... VoxelGrid runs (each a fixed number of launches) */
  int32_t step_forest_builds;   /* ... forest builds (1; more only when the node pool had to grow) */
  int32_t step_host_waits;      /* ... host waits */
  uint64_t arena_points_used, arena_points_capacity;  /* filtered points held (resident and staged) / room of the arena */
  uint64_t arena_nodes_used, arena_nodes_capacity;
  uint64_t active_cubes;        /* computeActiveAera of the last update */
} lslam_loc_window_stats;
/* setupFilesDirectory: reads directory/index2.txt (lines "count type i j k size"; type 0 corner, anything else surf; (i, j, k)
 * the signed global cube index; a later line for the same (type, cube) replaces the earlier one).  Nothing is read from the
 * PCDs until the first update.  Uses the cube size, valid distance and map filter sizes set before it.  A missing index2.txt:
 * LSLAM_ERR_INVALID, the node as it was. */
int lslam_pmap_open(lslam_loc *loc, const char *directory);
/* Upper bound of the filtered points the node keeps per feature type (resident and staged together; 0: no bound, the arena
 * grows).  A step that would need more is refused with LSLAM_ERR_INVALID after the staged cubes were dropped. */
int lslam_pmap_setup_capacity(lslam_loc *loc, size_t max_points_per_type);
/* DynamicFeatureMap::update: the window follows pos (a step if its cube changed), then computeActiveAera. */
int lslam_pmap_update(lslam_loc *loc, const float pos[3]);
/* Reads, filters and builds the cubes a window centred on pos's cube would need and the node does not hold, into spare room;
 * no table changes.  A later step adopts a staged cube instead of reading it; results do not depend on staging.  Called by
 * the host between sweeps with its predicted position; there is no library thread. */
int lslam_pmap_stage(lslam_loc *loc, const float pos[3]);
/* getSurroundFeature of the window as the last update left it (lslam_loc_get_surround updates at the node's pose first). */
int lslam_pmap_get_surround(lslam_loc *loc, float *corner_xyzi, size_t cap_corner, size_t *n_corner, float *surf_xyzi,
                                  size_t cap_surf, size_t *n_surf);
int lslam_pmap_window_info(lslam_loc *loc, lslam_loc_window_stats *out);
/* convertIndexFile: every line "count type i j k size" of in_path (an index.txt of lslam_fmap_save) written to out_path with
 * i - ox, j - oy, k - oz, so that a map saved by the mapping node can be opened paged.  No device is needed. */
int lslam_index_convert(const char *in_path, int32_t ox, int32_t oy, int32_t oz, const char *out_path);

/* ---- global re-localisation of the localisation node: a pose without an initial pose -----------------------------------------
 * lslam_loc_process drops every sweep until somebody gives the node a pose (a click in RViz or a GPS fix in the reference, whose
 * README names a "Re-Localization module" that was never written).  This stage finds the pose from one sweep and the loaded
 * map alone: very many pose hypotheses are scored against an occupancy set of the map, the best few are refined with the
 * node's own matcher, and the verdict says whether the answer is unambiguous.  The entry points take the node's handle and
 * carry the prefix lslam_reloc_.  Static maps only: a node in the paged mode answers LSLAM_ERR_INVALID, as does a node
 * without a map.  This comment is the specification; tests/relocalization_ref.py restates it in numpy.
 *
 * Occupancy sets.  Per feature type (0 corner, 1 surf) the set of voxels that hold at least one point the node holds after
 * lslam_loc_load / _set_map / _set_map_from_fmap (map filter included, cubes with fewer than five points too).  Voxel edge
 * `voxel` metres (0: 2.0); inv = 1.0f / voxel (one fp32 division on the host); the voxel of a point is
 * (int)floorf(x * inv) per axis, one fp32 multiply, then floor.  A point one of whose three floors is not finite, or not in
 * [-2^20, 2^20), has no voxel: it is not in the set and as a query it is not occupied.  The sets are exact (an open-addressing
 * table of packed 64-bit keys at a load of at most 1/2, filled with 64-bit compare-and-swap), built at the first use and
 * again when the map or `voxel` changes.
 *
 * Hypotheses.  h = r * n_pos + j for rotation r < n_rot and position j < n_pos; n_rot <= 4096, n_rot * n_pos <= 2^26.  A
 * rotation is a Twist angle triplet (rx, ry, rz); its matrix R is the rotation block of lslam_pose_to_isometry for
 * (rx, ry, rz, 0, 0, 0).  A position is float[3].
 *
 * Scan.  Both clouds through the node's scan filters (prepareFeatureFrame, the device step of lslam_loc_match).  With
 * max_points > 0 and n > max_points filtered points of a type, the points 0, s, 2 s, ... with s = ceil(n / max_points) are
 * scored, in the filter's order.
 *
 * Score.  q = R p + t in fp32 as ((r0 * x + r1 * y) + r2 * z) + t, every operation rounded on its own (no contraction).  A
 * point of type T counts when q has a voxel and that voxel is in set T.  score(h) = corner hits + surf hits.  A hypothesis
 * whose position's cube (round(p / cube_size) + origin, lslam_loc_process's rule) lies within 3 cubes of the cube array's edge
 * on any axis scores -1 and is counted in `skipped`.
 *
 * Selection.  On the device: the top_m (0: 256; <= 1024) hypotheses by score descending, then index ascending; -1 is never
 * selected; only this list comes back, behind the one host wait of the coarse stage.  On the host: greedy non-maximum
 * suppression in that order -- a hypothesis is dropped when a kept one has max|dpos| <= nms_m (0: 2.0) and a rotation index
 * within nms_rot (0: 2; negative: the same index only), compared cyclically modulo n_rot when rot_cyclic is set.  The first
 * max_candidates (0: 8; <= 64) survivors are refined.
 *
 * Refinement and verdict.  Each candidate runs lslam_loc_match's arithmetic (the same kernels over the scan prepared once)
 * from the hypothesis' Twist, again from its own result while it returns LSLAM_NOT_CONVERGED, at most refine_rounds (0: 3)
 * times: bit for bit what that many lslam_loc_match calls by hand return.  Candidates are visited in the order of their
 * sensor cube, so the cell grids are rebuilt once per distinct cube; afterwards the node's grids, counters of lslam_loc_info
 * and pose state are as they were.  The winner is the candidate whose last match returned LSLAM_OK with the largest n_rows
 * (ties: the better coarse rank); fraction = n_rows / (filtered corner + surf points, before subsampling); accepted when
 * fraction >= min_fraction (0: 0.4, the reference's match_percentage_threshold).  runner_up is the best such candidate
 * whose refined position is farther than nms_m (max|dpos|) from the winner's, or -1.
 * Returns LSLAM_OK with accepted = 1, LSLAM_NOT_CONVERGED when no candidate converged (winner = -1), LSLAM_TOO_FEW_MATCHES
 * when the winner is below min_fraction; the result is filled in all three.  With apply != 0 an accepted result is handed to
 * the node exactly as lslam_loc_set_initial_pose(T) would be; otherwise the node is left as it was. */
typedef struct {
  float voxel;             /* m; 0: 2.0 */
  int32_t max_points;      /* per type; 0: every filtered point */
  int32_t top_m;           /* 0: 256; <= 1024 */
  int32_t max_candidates;  /* 0: 8; <= 64 */
  float nms_m;             /* 0: 2.0 */
  int32_t nms_rot;         /* 0: 2; negative: the same rotation index only */
  int32_t rot_cyclic;      /* rotation indices wrap around (a full yaw sweep) */
  int32_t refine_rounds;   /* 0: 3 */
  float min_fraction;      /* 0: 0.4 */
  int32_t apply;
} lslam_reloc_opts;
typedef struct {
  int32_t hypothesis;      /* r * n_pos + j */
  int32_t coarse_score;
  int32_t status;          /* of the last match */
  int32_t rounds;          /* matches run */
  int32_t n_rows;
  float pose[6];           /* the refined Twist */
} lslam_reloc_candidate;
typedef struct {
  int32_t accepted;
  int32_t winner, runner_up;    /* indices into candidates, -1: none */
  float fraction;
  float T[16];                  /* the winner's pose, row-major 4x4 (identity without a winner) */
  int64_t n_hypotheses, skipped;
  int32_t n_points[2];          /* filtered scan points per type, before subsampling */
  int32_t n_scored[2];          /* ... of which were scored */
  int64_t occupied_voxels[2];
  int32_t n_selected;           /* length of the downloaded top list */
  int32_t n_candidates;
  lslam_reloc_candidate candidates[64];  /* in coarse rank order */
  float ms_coarse, ms_refine;   /* host wall clock of the two stages */
} lslam_reloc_result;
typedef struct {
  int64_t occupied_voxels[2];   /* of the sets as last built (0 before the first build) */
  uint64_t table_slots;         /* 64-bit slots of both tables together */
  int64_t builds;               /* set builds since creation */
  float voxel;                  /* the edge they were built with */
  int32_t valid;                /* 1 while they match the loaded map */
} lslam_reloc_map_stats;
/* Kernel shape, for tests that have to straddle it: positions per workgroup and scan points per LDS chunk. */
#define LSLAM_RELOC_POS_TILE 32
#define LSLAM_RELOC_CHUNK 1024
int lslam_reloc_relocalize(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                           const float *rot_xyz, size_t n_rot, const float *pos_xyz, size_t n_pos, const lslam_reloc_opts *opts,
                           lslam_reloc_result *result);
/* Parity tap: the same kernels up to the selection, no refinement; scores_out[n_rot * n_pos].  top_idx / top_score (room for
 * top_m each, may both be NULL) receive the downloaded list, *n_top its length; result (may be NULL) is filled up to
 * n_selected. */
int lslam_reloc_scores(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                       const float *rot_xyz, size_t n_rot, const float *pos_xyz, size_t n_pos, const lslam_reloc_opts *opts,
                       int32_t *scores_out, int32_t *top_idx, int32_t *top_score, int32_t *n_top, lslam_reloc_result *result);
/* The host half of the selection alone (no device needed): greedy NMS over a top list -> keep_out[<= max_candidates] (positions
 * in the list), returns their number or a negative status. */
int lslam_reloc_nms(const int32_t *top_idx, int32_t n_top, const float *pos_xyz, size_t n_rot, size_t n_pos,
                    const lslam_reloc_opts *opts, int32_t *keep_out);
/* Tap of the occupancy sets: out[i] = 1 when query point i (map frame) has a voxel and it is in set `which`. */
int lslam_reloc_occupied(lslam_loc *loc, int32_t which, float voxel, const void *queries, size_t nq, size_t stride_bytes,
                         uint8_t *out);
int lslam_reloc_info(lslam_loc *loc, lslam_reloc_map_stats *out);

/* ---- Survey-cloud feature map extractor (io_module/feature_extracter.cpp:43-130 over util/pcl_util.h:39-62,107-182 and
 * util/voxel_grid_partition.hpp:80-330): a dense survey cloud -> the corner / surf cube map the localisation node loads.
 * Per partition block: VoxelGrid with a minimum point count, radius-search PCA normals over the block, a K-nearest graph,
 * region growing, the angle-gap boundary test, VoxelGrid again, the axis permutation (x, y, z) <- (y, z, x) and worldToCube.
 * PCL is not part of the parity here: the yardstick is the numpy restatement tests/survey_map_ref.py, and where PCL's answer
 * is version dependent or unspecified the choice is fixed by this library (DESIGN "Survey-cloud extractor").  In short:
 *   - blocks in ascending partition cell, input order inside a block, processed one after another (device memory follows the
 *     largest block); non-finite points dropped; the "leaf too small" guard of the partition gives an empty result;
 *   - a neighbour of q is p with fp32 dx*dx + dy*dy + dz*dz < (float)((double)r * r); mean and covariance in fp64 over
 *     (double)p - (double)q, summed in ascending (search-grid cell (z, y, x), index) order; the eigenvector of the smallest
 *     eigenvalue by a fixed cyclic Jacobi iteration in fp64; flipped towards (0, 0, 0); curvature l0 / (l0 + l1 + l2); one
 *     rounding to fp32.  Fewer than 3 neighbours: the normal is undefined, the point leaves the later stages (counted);
 *   - neighbour lists: the K nearest by (fp32 squared distance, index), the point itself included;
 *   - region growing as the min-ancestor fixpoint of label[j] = min(label[j], label[i]) over the edges i -> j
 *     (j in i's list, fabsf(ni . nj) >= cosf-threshold), labels starting as (curvature, index) ranks;
 *   - the largest angle gap in fp64 with Eigen's unitOrthogonal basis. */
typedef struct lslam_survey lslam_survey;
typedef struct lslam_survey_params {
  double boundary_angle;         /* 3.14159 / 2.0 * 0.9 (the literal, not pi): a point is a boundary point iff its gap is larger */
  float partition_leaf;          /* 50.0   voxelPartition */
  int32_t partition_min_points;  /* 1000 */
  float filter_leaf;             /* 0.05   voxelFilter of a block */
  int32_t filter_min_points;     /* 3 */
  float normal_radius;           /* 0.05   normalEstimate, search surface = the block */
  int32_t knn_k;                 /* 60     RegionGrowing::setNumberOfNeighbours; 1 .. 64 */
  float smoothness_angle;        /* (float)(3.0 / 180.0 * M_PI); the edge threshold is (float)cos((double)smoothness_angle) */
  float curvature_threshold;     /* 1.0    above every curvature: each reached point grows on.  Values below 1/3 are refused */
  int32_t cluster_min;           /* 50 */
  int32_t cluster_max;           /* 1000000 */
  float boundary_radius;         /* 0.1 */
  float feature_leaf;            /* 0.2    voxelFilter of the planar and the boundary cloud */
  int32_t feature_min_points;    /* 3 */
  float cube_size;               /* 50.0   FeatureMap(21, 21, 21), setupWorldOrigin(10, 5, 10), setupWorldCubeSize(50.0) */
  int32_t cube_dims[3];
  int32_t cube_origin[3];
  float knn_cell;                /* cell of the K-nearest search grid [m]; 0: 4 * filter_leaf.  Results do not depend on it */
  int32_t reserved;
} lslam_survey_params;
typedef struct lslam_survey_stats {
  int64_t points_in;           /* finite points of the cloud */
  int64_t points_nonfinite;    /* dropped before the partition */
  int64_t blocks_kept;         /* partition cells with at least partition_min_points points */
  int64_t blocks_dropped;      /* occupied cells below it */
  int64_t max_block_points;
  int64_t filtered_points;     /* after the first filter, all blocks */
  int64_t undefined_normals;   /* of those: fewer than 3 neighbours */
  int64_t clusters_kept;       /* regions inside [cluster_min, cluster_max] */
  int64_t clusters_dropped;
  int64_t label_sweeps;        /* launches of the label sweep, all blocks (depends on scheduling: not part of the parity) */
  int64_t planar_points;       /* before the second filter */
  int64_t boundary_points;
  int64_t n_corner;            /* the result: boundary points in the cubes */
  int64_t n_surf;              /* ... planar points */
} lslam_survey_stats;
/* Writes every byte of *p (the reference's literals above). */
void lslam_survey_default_params(lslam_survey_params *p);
/* The whole extraction of a host cloud (x, y, z floats at the head of every stride_bytes record).  The result stays on the
 * device in *out (which owns it; lslam_survey_destroy frees it; scratch of the call is freed before it returns).  An empty
 * cloud and a cloud whose cells are all below the minimum give an empty result and LSLAM_OK. */
int lslam_survey_extract(lslam_ctx *ctx, const void *cloud, size_t n, size_t stride_bytes, const lslam_survey_params *params,
                         lslam_survey **out);
/* The same from a PCD file, read by the reader of lslam_fmap_load (DATA ascii or binary; binary_compressed and a missing file
 * are refused with LSLAM_ERR_INVALID, lslam_last_error says which). */
int lslam_survey_extract_file(lslam_ctx *ctx, const char *pcd_path, const lslam_survey_params *params, lslam_survey **out);
int lslam_survey_info(lslam_survey *sv, lslam_survey_stats *out);
/* Both clouds {x, y, z, intensity = 0} in block order (a null buffer is skipped; cap in points, at least the stats' count). */
int lslam_survey_get(lslam_survey *sv, float *corner_xyzi, size_t cap_corner, float *surf_xyzi, size_t cap_surf);
/* saveCloudToFiles: directory/index.txt and <count>.pcd in the layout lslam_fmap_save writes, points of a cube in block order. */
int lslam_survey_save(lslam_survey *sv, const char *directory);
void lslam_survey_destroy(lslam_survey *sv);
/* pcl::VoxelGrid with setMinimumPointsNumberPerVoxel(min_points): lslam_voxel_grid's arithmetic, voxels with fewer points
 * give no output.  min_points = 1: bit for bit lslam_voxel_grid. */
int lslam_voxel_grid_min(lslam_ctx *ctx, const void *cloud, size_t n, size_t stride_bytes, float leaf, int32_t min_points,
                         float *out_xyzi, size_t cap, size_t *n_out);
/* Stage taps (tests): each works on caller-supplied host arrays of packed {x, y, z, w} float records.
 * normals: out_normal[q] = {nx, ny, nz, curvature} (NaN when undefined), out_count[q] = neighbours in radius. */
int lslam_debug_survey_normals(lslam_ctx *ctx, const float *surface_xyzw, size_t n_surface, const float *query_xyzw, size_t n_query,
                               float radius, float *out_normal, int32_t *out_count);
/* out_lists[i * k + t]: the t-th nearest point of i (itself included), -1 past the cloud's size.  cell <= 0: chosen here. */
int lslam_debug_survey_knn(lslam_ctx *ctx, const float *pts_xyzw, size_t n, int32_t k, float cell, int32_t *out_lists);
/* normals_curv = {nx, ny, nz, curvature}; out_labels[i] = the index of the seed point whose region i joins; sweeps_out: launches. */
int lslam_debug_survey_region(lslam_ctx *ctx, const float *normals_curv, size_t n, const int32_t *lists, int32_t k, float cos_threshold,
                              int32_t *out_labels, int32_t *sweeps_out);
int lslam_debug_survey_boundary(lslam_ctx *ctx, const float *pts_xyzw, const float *normals_xyzw, size_t n, float radius,
                                double angle_threshold, uint8_t *out_flags, double *out_gaps);

#ifdef __cplusplus
}
#endif
#endif /* LSLAM_C_H */
