/*
 * lsgpu_icp.h -- C ABI of the MI355X-native ICP scan-matching path (liblsgpu_icp.so).
 *
 * The reference exposes no FFI for this path: `icp_` is a concrete PointMatcher::ICP member
 * (laser_slam/include/laser_slam/laser_track.hpp:217, incremental_estimator.hpp:70) and the two
 * call sites are
 *     icp_.compute(last_scan.scan, sub_map, T_init)        laser_slam/src/laser_track.cpp:496
 *     icp_.compute(sub_map_b, sub_map_a, T_init)           laser_slam/src/incremental_estimator.cpp:108
 * This header is the seam a maintainer binds instead (INTEGRATION.md shows the C++ shim): one
 * handle == one `icp_` member == one device + one HIP stream.  Handles are independent (tracks run
 * concurrently, laser_track.hpp:211 holds one mutex per track); a handle is not thread safe.
 *
 * Data layout == PointMatcher<float>::DataPoints (laser_slam/include/laser_slam/common.hpp:14-17):
 *   features    (dim+1) x N column major  ->  AoS x,y,z,1 float, 16 B / point  ("xyz1")
 *   descriptors "normals" 3 x N column major -> 12 B / point
 *   TransformationParameters 4x4 float column major; p_reference = T * p_reading.
 * Every pointer argument may be host memory or device (HBM) memory of the handle's device; the
 * library detects which.  Host buffers are copied, never retained.  No exceptions cross this ABI.
 *
 * Stream contract: every call does its device work on the HANDLE'S OWN stream (created non-blocking: it does not
 * synchronise with the null stream or with any stream of the caller) and returns after that work has completed, so
 * outputs are valid on return.  Device INPUTS must be complete before the call: a buffer still being written by
 * the caller's stream has to be synchronised first (hipStreamSynchronize / an event wait on the producing stream).
 * The Python twin (laser_slam_amd/icp.py) synchronises torch's current stream before every call that passes a
 * device tensor.
 *
 * Modules: the chain of icp_default.yaml, PointToPointErrorMinimizer in place of PointToPlaneErrorMinimizer
 * (lsgpu_icp_config.error_minimizer), KDTreeMatcher with knn 1..LSGPU_MATCHER_KNN_MAX (lsgpu_icp_config.matcher_knn) and
 * maxDist (matcher_max_dist), any subset of Trimmed- / Max- / Min- / MedianDistOutlierFilter (outlier_*), and
 * SurfaceNormalDataPointsFilter in place of SamplingSurfaceNormalDataPointsFilter as the reference filter
 * (lsgpu_chain_config.sn_knn), and RobustOutlierFilter (lsgpu_icp_set_robust_filter), and SurfaceNormalOutlierFilter with
 * SurfaceNormalDataPointsFilter on the reading and ObservationDirection- + OrientNormalsDataPointsFilter on either cloud
 * (lsgpu_icp_set_normals), and PointToPlaneWithCovErrorMinimizer: the point-to-plane step plus the 6x6 covariance of the result
 * (lsgpu_icp_set_covariance, lsgpu_icp_get_quality), and MaxDensityDataPointsFilter behind the reference's
 * SurfaceNormalDataPointsFilter with keepDensities 1 (lsgpu_icp_set_max_density), and ShadowDataPointsFilter behind the normals
 * of either filter section (lsgpu_icp_set_shadow), and CovarianceSamplingDataPointsFilter as the last thinning step of either
 * (lsgpu_icp_set_cov_sampling).
 */
#ifndef LSGPU_ICP_H_
#define LSGPU_ICP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 still: the four chain fields of lsgpu_icp_config (matcher_max_dist ...) took reserved ints that had to be 0, the struct
 * kept its size and every offset, and 0 means what it meant -- a caller built against the earlier header runs unchanged.
 * lsgpu_chain_load and the two *_config_why accessors are additions: new symbols and new structs, nothing that existed
 * changed its layout or its meaning. */
#define LSGPU_ABI_VERSION 4

/* Return codes.  NO_CONVERGENCE is PointMatcher::ConvergenceError: laser_track.cpp:499-502 catches it
 * and keeps the odometry guess; incremental_estimator.cpp:108 lets it propagate. */
enum {
  LSGPU_OK = 0,
  LSGPU_NO_CONVERGENCE = 1,
  LSGPU_BAD_CONFIG = 2,
  LSGPU_HIP_ERROR = 3,
  LSGPU_BAD_ARG = 4
};

typedef struct lsgpu_icp lsgpu_icp;

/* Device-side part of the chain in laser_slam/configurations/icp_default.yaml:9-27. */
typedef struct lsgpu_icp_config {
  float trim_ratio;       /* TrimmedDistOutlierFilter ratio            yaml:16  (0.75)  */
  int   max_iterations;   /* CounterTransformationChecker              yaml:23  (40)    */
  float min_diff_rot;     /* Differential... minDiffRotErr   [rad]     yaml:25  (0.001) */
  float min_diff_trans;   /* Differential... minDiffTransErr [m]       yaml:26  (0.01)  */
  int   smooth_length;    /* Differential... smoothLength              yaml:27  (4)     */
  float cell_size;        /* finest voxel edge [m]; <= 0: automatic; NaN / +inf: BAD_CONFIG (see "The voxel grid's geometry") */
  int   profile_kernels;  /* 1: HIP-event time every kNN launch (see lsgpu_icp_stats)    */
  int   reserved[1];      /* reserved[0] = 1 disables the trimmed-radius cap (debug)       */
  int   error_minimizer;  /* LSGPU_MINIMIZER_* (0, the default: point-to-plane); any other value: LSGPU_BAD_CONFIG */
  int   matcher_knn;      /* KDTreeMatcher knn: 0 or 1 one neighbour; 2..LSGPU_MATCHER_KNN_MAX k nearest matches; other: BAD_CONFIG */
  /* 0 (what lsgpu_icp_config_yaml / _default and a zero-filled struct hold) = absent; see "maxDist and outlier-filter chains" */
  float matcher_max_dist;       /* KDTreeMatcher maxDist [m]: a match is valid iff d2 <= maxDist^2; +inf = absent           */
  float outlier_max_dist;       /* MaxDistOutlierFilter maxDist [m]: keep d2 <= maxDist^2; +inf = absent                    */
  float outlier_min_dist;       /* MinDistOutlierFilter minDist [m]: keep d2 >= minDist^2                                   */
  float outlier_median_factor;  /* MedianDistOutlierFilter factor: keep d2 <= factor * median(d2)                           */
  int   reserved_[1];
} lsgpu_icp_config;

/* The voxel grid's geometry (lsgpu_icp_config.cell_size; read by every lsgpu_icp_set_reference, reported by
 * lsgpu_icp_get_info).  The level-0 cell edge starts at h0 = cell_size if cell_size > 0, else 0.125 m (any value <= 0,
 * -inf included, is "automatic").  With ext the longest edge of the reference's bounding box: bits_per_axis grows from 11
 * to 13 (fine_bits falls from 5 to 3) while h0 * (2^bits - 1) < 1.0001 ext, then h0 doubles until the box fits.  So every
 * finite positive cell_size is legal, however small (the doubling ends after at most a few hundred steps) or large (the whole
 * cloud in one cell); it changes the time a search takes, never a result.  NaN and +inf are LSGPU_BAD_CONFIG from
 * lsgpu_icp_create, checked before the device is touched.  A reference with a NaN or infinite coordinate is LSGPU_BAD_ARG
 * from lsgpu_icp_set_reference ("non-finite coordinates" in lsgpu_last_error); the handle then holds no reference. */

/* maxDist and outlier-filter chains.  All comparisons on squared distances in float; maxDist * maxDist etc. are one
 * float multiply.
 *   matcher_max_dist: a match further than maxDist is INVALID: index -1, d2 +inf, weight 0 under every outlier filter and with
 *     none.  With knn = k each of the k entries is judged on its own; the valid ones come first, in the usual order.  The
 *     search never looks further than maxDist, from its first launch on.  lsgpu_knn / lsgpu_knn_k on such a handle return
 *     -1 / +inf for invalid matches.
 *   Quantiles (the trim limit, the median) are taken over the m valid matches only: sorted(finite d2)[min(m - 1,
 *     (int64)((float)m * q))] -- as lsgpu_trim_limit, which skips +inf inputs (none finite: LSGPU_NO_CONVERGENCE).
 *   Outlier filters: trim_ratio (TrimmedDist, 1 = none), outlier_max_dist, outlier_min_dist, outlier_median_factor; every
 *     filter sees the same matches, the 0/1 weights are multiplied, so a pair is kept iff it passes every filter and the order
 *     of the modules does not matter.  lsgpu_iter_trace.limit / lsgpu_icp_stats.final_limit are the iteration's effective
 *     upper limit: the smallest of {trim limit, outlier_max_dist^2, factor * median} present; n_used counts kept pairs.
 *     Nothing kept: LSGPU_NO_CONVERGENCE, T_out = T_init.
 *   Negative or NaN values, and +inf for outlier_min_dist / outlier_median_factor, are LSGPU_BAD_CONFIG from lsgpu_icp_create
 *   (checked before the device is touched).  A handle with any of the four fields searches with the k-best kernels for every
 *   knn and runs the full select in every iteration (csrc/lsgpu_policy.h, plan_chain); lsgpu_icp_comm_init refuses it. */

/* KDTreeMatcher knn (lsgpu_icp_config.matcher_knn), epsilon 0.  With knn = k >= 2 every reading point is paired with its k
 * nearest reference points (Matches: k x N dists / ids): TrimmedDistOutlierFilter ranks all k N distances (limit =
 * sorted(d2)[floor(float(k N) * ratio)]), the error minimizer adds every pair with weight 1 (the reading point once per
 * kept match; point-to-plane with the matched point's normal), lsgpu_icp_stats.final_n_used and the trace's n_used count
 * pairs.  Checkers, the update and the composition of T are those of knn 1.  The k matches of a point are in ascending
 * d2, ties to the smaller index of the handle's Morton-sorted reference (csrc/lsgpu_knn_k.hip.h).  A reference with fewer
 * than k points is LSGPU_BAD_ARG; the split-scan mode (lsgpu_icp_comm_init) refuses a k-match handle (LSGPU_BAD_CONFIG). */
#define LSGPU_MATCHER_KNN_MAX 8

/* errorMinimizer modules (lsgpu_icp_config.error_minimizer).  Point-to-plane (yaml:18-19) solves the 6x6 normal
 * equations of J = [p x n; n] and needs the reference normals.  Point-to-point (libpointmatcher's
 * PointToPointErrorMinimizer) needs none: with the trimmed pairs' centroids p_, q_ and M = sum (q - q_)(p - p_)^T
 * = U S V^T, R = U V^T (U diag(1,1,-1) V^T if det < 0), t = q_ - R p_, and T_iter <- [R t] T_iter.  Sums in double,
 * the 3x3 solve in double (Horn's quaternion, Jacobi eigen-solver with an exact stopping rule), R and t rounded to
 * float.  A point-to-point handle never reads reference normals: set_reference / align_batch accept NULL normals, and
 * lsgpu_chain_config.ssn_knn = 0 (no reference filter module) is accepted. */
#define LSGPU_MINIMIZER_POINT_TO_PLANE 0
#define LSGPU_MINIMIZER_POINT_TO_POINT 1

/* icp_default.yaml values / ICP::setDefault() values (laser_track.cpp:17,20). */
void lsgpu_icp_config_yaml(lsgpu_icp_config* c);
void lsgpu_icp_config_default(lsgpu_icp_config* c);

typedef struct lsgpu_icp_stats {
  int     iterations;
  int     converged;         /* 1 stopped by the differential checker, 0 by the counter */
  float   final_limit;       /* last trimmed squared-distance limit                     */
  int64_t final_n_used;      /* pairs with weight 1 in the last iteration               */
  int64_t stragglers;        /* queries resolved by the exact fallback search, summed   */
  double  t_total_ms;        /* host wall time of the call                              */
  double  t_knn_ms;          /* sum of kNN time, main + fallback (HIP events; profile_kernels=1) */
  int     knn_launches;
  double  t_knn_main_ms;     /* k_knn_main only                                         */
  double  t_knn_fallback_ms; /* k_knn_fallback only                                     */
  int     cap_retries;       /* iterations repeated because the radius-cap prediction failed */
  int     pad_;              /* iterations whose predicted select missed and was redone in full (info)  */
  double  t_reserved[1];     /* lsgpu_icp_compute: milliseconds in the two filters + set_reference */
  double  t_select_ms;       /* sum over the iterations: trimmed-distance select kernels (profile_kernels=1) */
  double  t_ne_ms;           /* sum over the iterations: normal equations + solve + checkers (profile_kernels=1) */
  int     committed_select_iterations;  /* iterations whose trim limit came from the search kernels' own tables (no select launch) */
  int     spread_tiles;                 /* 64-query tiles whose queries share no candidates (searched row-wise by the front of the tile kernel) */
  int     reference_reused;             /* lsgpu_icp_align_batch: 1 if this pair kept the previous pair's reference structures (no set_reference) */
  int     comm_calls;                   /* split-scan mode, profile_kernels=1: RCCL calls of the loop ... */
  double  t_comm_ms;                    /* ... and the time between their first and last kernel on the stream, summed */
  int     direction_index_launches;     /* searches served by the direction index (k_knn_cone) instead of the voxel grid */
  float   direction_index_occupancy;    /* reference points per occupied bin of that index (0: not built / not looked at);
                                           above LSGPU_CONE_MAX_OCC (7) the settled searches stay on the voxel grid */
  float   direction_index_heavy_share;  /* share of the searching queries whose windows in that index would be long (priced by the
                                           search before its first use, again before every later look at the loop state while
                                           it keeps the alignment off the index; -1: not priced); above LSGPU_CONE_HEAVY_SHARE
                                           (csrc/lsgpu_tuning.h: 0.07) the alignment stays on the voxel grid */
} lsgpu_icp_stats;

/* One record per iteration (optional parity/debug trace; replaces the VTKFileInspector dump of
 * icp_default.yaml:32-40). */
typedef struct lsgpu_iter_trace {
  float   T_iter[16];
  float   limit;
  int64_t n_used;
  double  A[36];
  double  b[6];
  double  x[6];             /* point-to-point handles: A[0..8] = the centred M (row major, rest 0), b = {p_, q_},
                             * x = {rotation vector of R, t} */
  float   knn_main_us;      /* k_knn_tile duration (HIP events; 0 unless profile_kernels) */
  float   knn_fallback_us;  /* k_knn_fallback duration                                    */
  uint32_t stragglers;      /* queries resolved by the fallback in this iteration         */
  uint32_t reserved;        /* development counter: heavy tiles a wide launch (first iterations) counted -- the first 1024 go to the
                             * wave-per-query pass; 0 in the settled iterations */
} lsgpu_iter_trace;

int  lsgpu_icp_create(const lsgpu_icp_config* cfg, int device, lsgpu_icp** out);
void lsgpu_icp_destroy(lsgpu_icp* h);

/* Steps 2-3 of ICP::compute: centre the (already filtered) reference on its mean, build the voxel
 * grid.  `normals` = the descriptor SamplingSurfaceNormalDataPointsFilter attached (yaml:5-7); may be NULL (a
 * point-to-point handle reads no normals). */
int lsgpu_icp_set_reference(lsgpu_icp* h, const float* ref_xyz1, const float* ref_normals, int64_t nr);

/* Steps 5-7 of ICP::compute on the (already filtered) reading.  T_out = T_init on failure.  A T_init that is not rigid
 * (lsgpu_check_rigid: |1 - det R| > 1e-3) is LSGPU_BAD_ARG -- step 5 is a RigidTransformation::compute, which throws
 * PointMatcher's TransformationError for it; neither call site of the reference corrects its guess
 * (laser_track.cpp:489-496, incremental_estimator.cpp:92-108). */
int lsgpu_icp_align(lsgpu_icp* h, const float* reading_xyz1, int64_t nq, const float T_init[16],
                    float T_out[16], lsgpu_icp_stats* stats);

/* ---- many independent scan pairs on one GPU (BASELINE config 3) --------------------
 * Replaces a loop of `icp_.compute` calls over independent pairs (laser_slam/src/laser_track.cpp:496 has
 * no state across calls).  Pair i runs {set_reference, align} on handles[i % n_handles]; the handles work
 * concurrently, each on its own HIP stream driven by its own host thread, so that small clouds (200 k
 * points do not fill 256 CUs) overlap on the device.  Results do not depend on n_handles.  All handles
 * must live on the same device.  rc[i] receives pair i's return code (LSGPU_NO_CONVERGENCE leaves
 * T_out[i] = T_init[i], like lsgpu_icp_align); the function returns the first non-OK, non-NO_CONVERGENCE
 * code, else LSGPU_NO_CONVERGENCE if any pair failed to converge, else LSGPU_OK.
 * T_init / T_out: 16 floats per pair, column major.  stats and rc may be NULL.
 * reference_normals[i] may be NULL for point-to-point handles (LSGPU_MINIMIZER_POINT_TO_POINT).
 * Reference reuse: a pair whose reference_xyz1[i], reference_normals[i] and n_reference[i] equal those of the previous
 * pair of the same handle (pair i - n_handles) skips set_reference -- the sorted reference, chunks and cell tables depend
 * on the reference alone (stats[i].reference_reused = 1 for such a pair).  Results are bit-identical either way. */
int lsgpu_icp_align_batch(lsgpu_icp* const* handles, int n_handles, int64_t n_pairs,
                          const float* const* reference_xyz1, const float* const* reference_normals,
                          const int64_t* n_reference, const float* const* reading_xyz1,
                          const int64_t* n_reading, const float* T_init, float* T_out,
                          lsgpu_icp_stats* stats, int* rc);

/* ---- one scan pair split over several GPUs (BASELINE config 4) -------------------------
 * Every rank holds the whole reference (set_reference with the same cloud) and ITS shard of the reading.
 * After lsgpu_icp_comm_init, lsgpu_icp_align treats its `reading_xyz1` as the local shard: per iteration
 * the three select histograms (3 x 2048 u32) and the 29 normal-equation sums are all-reduced over RCCL on
 * the handle's stream, so every rank computes the same limit, the same 6x6 system and the same T.
 * The unique id comes from rank 0 (lsgpu_comm_get_unique_id) and travels to the other ranks by any
 * means (torch.distributed broadcast in laser_slam_amd/sharding.py).  Every rank needs >= 1 point. */
#define LSGPU_COMM_ID_BYTES 128
int lsgpu_comm_get_unique_id(void* id /* LSGPU_COMM_ID_BYTES */);
int lsgpu_icp_comm_init(lsgpu_icp* h, int rank, int nranks, const void* id);

/* Per-iteration records of the last align; returns the number written.  The records stay in device memory until this
 * call fetches them (one synchronous copy); the next alignment on the handle overwrites them. */
int lsgpu_icp_get_trace(lsgpu_icp* h, lsgpu_iter_trace* out, int cap);

/* Geometry of the voxel-hash pyramid built by the last set_reference (for roofline accounting). */
typedef struct lsgpu_icp_info {
  int64_t  n_reference;
  int      bits_per_axis;      /* level 0 has 2^bits cells per axis        */
  int      fine_bits;          /* key bits per axis below level 0           */
  float    cell_size;          /* level-0 edge [m]                          */
  uint32_t n_chunks;           /* <=64-point chunks (32 B descriptor each)  */
  uint32_t cells[17];          /* occupied cells per level                  */
  uint64_t table_bytes;        /* hash tables, all levels                   */
} lsgpu_icp_info;
int lsgpu_icp_get_info(lsgpu_icp* h, lsgpu_icp_info* out);

/* What the handle's launch policy remembers ACROSS calls (nothing of it changes a result; it decides what a call costs).
 * The per-alignment decisions are in lsgpu_icp_stats; these outlive an alignment. */
typedef struct lsgpu_policy_info {
  int   index_rest;          /* alignments that will still leave the direction index alone: the handle found it slower than
                                the voxel grid (two timed searches per alignment); LSGPU_NO_INDEX_REST=1 switches the
                                judgement off, a reference of another size resets it */
  float pay_voxel_us;        /* the two timings of the last alignment that took them (0: none yet): the voxel-grid search in */
  float pay_index_us;        /* front of the index's first use / the first settled search through the index */
  int   ssn_sort_fallbacks;  /* reference filters this handle had to repeat with the segmented sorts because the sort-free
                                levels gave up (more candidates around a median than a workgroup selects among) */
  int   ssn_calls;           /* reference filters run by this handle */
  int   reserved[3];
} lsgpu_policy_info;
int lsgpu_icp_get_policy_info(lsgpu_icp* h, lsgpu_policy_info* out);

/* The float mean subtracted from the reference (T_refIn_refMean translation). */
int lsgpu_icp_get_reference_mean(lsgpu_icp* h, float mean[3]);

/* ---- kernel-level entry points (parity tests / profiling); all in the reference-MEAN frame ---- */

/* KDTreeMatcher::findClosests knn=1 eps=0 (yaml:9-12): ids index the reference as given to
 * set_reference, d2 = squared distance.  T (may be NULL = identity) is applied to each query on load. */
int lsgpu_knn(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16], int32_t* ids,
              float* d2);
/* KDTreeMatcher::findClosests knn=k eps=0, 1 <= k <= LSGPU_MATCHER_KNN_MAX: ids / d2 hold k entries per query, query
 * major (query i at [i k, i k + k) -- the k x N column-major Matches), each query's in ascending d2 (ties: see
 * matcher_knn), ids indexing the reference as given to set_reference.  LSGPU_BAD_ARG if the reference has fewer than k
 * points or k nq does not fit the loop's 32-bit counts. */
int lsgpu_knn_k(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16], int k, int32_t* ids, float* d2);
/* TrimmedDistOutlierFilter (yaml:14-16): limit = sorted(d2)[floor(n*ratio)], n counting the finite inputs only (+inf = an
 * invalid match, skipped; the count and the rank are taken on the device); LSGPU_NO_CONVERGENCE if none is finite.  A ratio
 * <= 0 asks for rank 0, the smallest input, whatever the count (rank from the host, as before). */
int lsgpu_trim_limit(lsgpu_icp* h, const float* d2, int64_t n, float ratio, float* limit);
/* PointToPlaneErrorMinimizer accumulation (yaml:18-19): out = 21 upper-tri of sum J J^T (row major
 * order a<=c), 6 of -sum J r, sum w, sum w r^2  -> double[29].  w = 1 for the pairs with ids >= 0 and a finite
 * d2 <= limit (+inf and NaN = an invalid match, as in lsgpu_trim_limit: a limit of +inf keeps every valid pair). */
int lsgpu_normal_eq(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16],
                    const int32_t* ids, const float* d2, float limit, double out[29]);
/* PointToPointErrorMinimizer accumulation, same inputs as lsgpu_normal_eq: out[0..2] = sum p, [3..5] = sum q,
 * [6..14] = sum q p^T (row major), [15..26] = 0, [27] = sum w, [28] = sum w |p - q|^2 (p - q in float) -> double[29]. */
int lsgpu_point_to_point(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16],
                         const int32_t* ids, const float* d2, float limit, double out[29]);
/* The point-to-point step from those 29 sums: T_out = dT (4x4 float, column major).  Host only (no GPU, no handle);
 * the same function the device loop runs, bit for bit.  LSGPU_NO_CONVERGENCE for sum w = 0 ("no point to minimize")
 * or a non-finite result. */
int lsgpu_point_to_point_solve(const double sums[29], float T_out[16]);
/* RigidTransformation::compute on features (laser_track.cpp:265,485): out = T * xyz1. */
int lsgpu_transform_points(lsgpu_icp* h, const float T[16], const float* xyz1, int64_t n, float* out);
/* RigidTransformation::compute on a 3-row descriptor of the cloud (`normals`, `observationDirections`: the descriptors
 * upstream rotates, laser_track.cpp:265,485,630,643 when stored scans carry them): out = R * d, 3 floats per point
 * (a 3 x N column-major matrix), same fma chain as the points without the translation.  LSGPU_BAD_ARG if T is not rigid
 * (TransformationError upstream). */
int lsgpu_rotate_descriptors(lsgpu_icp* h, const float T[16], const float* desc3, int64_t n, float* out);

/* ---- the whole of ICP::compute on the device ----------------------------------
 * The sampling filters of icp_default.yaml:1-7 as device kernels, and the complete call
 * `icp_.compute(reading, reference, T_init)` (laser_slam/src/laser_track.cpp:496,
 * incremental_estimator.cpp:108) = reference filter, set_reference, reading filter, align, without the
 * clouds leaving the GPU.  Draws: the library's own stream with the std::srand/std::rand sequence of
 * glibc (csrc/lsgpu_rand.h); seed >= 0 reseeds it, seed < 0 continues it.  The device filters, the host
 * filters below and the oracle produce the same points, in the same order, with the same normals. */
typedef struct lsgpu_chain_config {
  float   reading_prob;     /* RandomSamplingDataPointsFilter.prob            yaml:2-3 (0.5); < 0: NO reading filter
                             * module (a yaml without readingDataPointsFilters): every point, no draw consumed */
  int     ssn_knn;          /* SamplingSurfaceNormalDataPointsFilter.knn      yaml:6-7 (10); 0: NO reference filter
                             * module -- the reference as given, no normals, no draw (point-to-point handles only) */
  float   ssn_ratio;        /* SamplingSurfaceNormalDataPointsFilter.ratio    yaml:6-7 (0.5)  */
  int     sn_knn;           /* SurfaceNormalDataPointsFilter.knn (3..32) as THE reference filter module; 0 (both presets, a
                             * zero-filled struct): absent.  Not together with ssn_knn > 0: LSGPU_BAD_CONFIG */
  int64_t seed;             /* >= 0: reseed before the reference filter; < 0: continue        */
} lsgpu_chain_config;
void lsgpu_chain_config_yaml(lsgpu_chain_config* c);     /* icp_default.yaml values           */
void lsgpu_chain_config_default(lsgpu_chain_config* c);  /* ICP::setDefault(): 0.75, 7, 0.5   */
/* What lsgpu_icp_compute accepts, without a handle or a device: LSGPU_OK, or LSGPU_BAD_CONFIG for ssn_knn / sn_knn outside
 * {0, 3..32}, both of them > 0, or neither with the point-to-plane minimizer (error_minimizer: LSGPU_MINIMIZER_*), which
 * needs the normals one of them provides. */
int lsgpu_chain_config_check(const lsgpu_chain_config* c, int error_minimizer);

/* SamplingSurfaceNormalDataPointsFilter on the device.  3 <= knn <= 32.  out_xyz1 (4 floats/pt) and
 * out_normals (3 floats/pt) need room for n points; host or device pointers. */
int lsgpu_icp_filter_reference(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float ratio,
                               int64_t seed, float* out_xyz1, float* out_normals, int64_t* n_out);
/* SurfaceNormalDataPointsFilter (keepNormals 1, epsilon 0, no maxDist) -- the contract, for the device and the host
 * version (lsgpu_filter_surface_normal) alike, which agree bit for bit:
 *   Every point is kept, in its place, and no rand() draw is consumed; 3 <= knn <= 32 and n >= knn, else LSGPU_BAD_ARG.
 *   Coordinates: everything below is taken on the cloud CENTRED ON ITS MEAN exactly as lsgpu_icp_set_reference centres
 *     it -- mean = (float)(sum in double / n) per coordinate, c = p - mean, one float subtraction per coordinate.
 *   The neighbourhood of point i is its knn nearest points of the same cloud, ITSELF INCLUDED (at distance 0; first
 *     unless an exact duplicate of it has a smaller index), exact search, d2 = fma(dz,dz, fma(dy,dy, dx*dx)) in float; neighbours in ascending d2, ties to the smaller index
 *     of the cloud as given -- the same rule picks between a knn-th and a (knn+1)-th point at the same distance.
 *   Normal: mean of the neighbourhood (float sum in that order / (float)knn), C = sum e e^T in float, rank test and
 *     eigenvector of the smallest eigenvalue as for a box of the sampling filter (csrc/lsgpu_box_normal.h, box_normal).
 *     A neighbourhood that fails the rank test (rank + 1 < 3: all its points on one line) gets the normal (0, 1, 0).
 * Device entry point: out_normals 3 floats per point; out_ids (nullable) knn indices per point, point major, into the
 * cloud as given, in that order (self first, but for a duplicate with a smaller index); out_d2 (nullable, only with out_ids) the matching squared distances.  Host or device
 * pointers.  The search runs on the structures lsgpu_icp_set_reference builds, so the call LEAVES THE CLOUD AS THE
 * HANDLE'S REFERENCE with these normals -- as lsgpu_icp_set_reference(h, xyz1, out_normals, n) would. */
int lsgpu_icp_filter_reference_normals(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float* out_normals,
                                       int32_t* out_ids, float* out_d2);
/* RandomSamplingDataPointsFilter on the device: keeps point i iff draw_i < prob, order preserved. */
int lsgpu_icp_filter_reading(lsgpu_icp* h, const float* xyz1, int64_t n, float prob, int64_t seed,
                             float* out_xyz1, int64_t* n_out);
/* ICP::compute.  Returns like lsgpu_icp_align (LSGPU_NO_CONVERGENCE also when a filter leaves no
 * point); stats->t_reserved[0] = milliseconds spent in the two filters + set_reference.
 * chain->sn_knn > 0: the reference filter is SurfaceNormalDataPointsFilter -- the whole reference, its normals computed
 * on the grid set_reference has just built; a reference with fewer than sn_knn points is LSGPU_BAD_ARG.  A point-to-point
 * handle reads no normals and skips the computation. */
int lsgpu_icp_compute(lsgpu_icp* h, const float* reading_xyz1, int64_t nq, const float* reference_xyz1,
                      int64_t nr, const float T_init[16], const lsgpu_chain_config* chain,
                      float T_out[16], lsgpu_icp_stats* stats);

/* ---- clouds kept in HBM between calls (persistent sub-maps) ------------------------
 * LaserTrack::localScanToSubMap (laser_slam/src/laser_track.cpp:466-519) rebuilds its sub-map at every scan
 * from the last `nscan_in_sub_map` scans: a 4x4 * 4xN transform and a concatenate per extra scan, all on the
 * host, then hands reading and sub-map to icp_.compute.  Here a scan is uploaded once into a numbered slot of
 * the handle; lsgpu_icp_compute_clouds assembles the sub-map on the device (out_i = T_i * cloud_i with the
 * arithmetic of lsgpu_transform_points, concatenated in the order given) and runs the whole ICP::compute on it.
 * Slots are small non-negative integers chosen by the caller; uploading to a used slot replaces its cloud. */
int lsgpu_cloud_upload(lsgpu_icp* h, int slot, const float* xyz1, int64_t n);
int lsgpu_cloud_release(lsgpu_icp* h, int slot);
int lsgpu_cloud_size(lsgpu_icp* h, int slot, int64_t* n);   /* n = -1: empty slot */
/* reading = cloud `reading_slot`; reference = concat_i ( T_i * cloud ref_slots[i] ), ref_T = 16 floats per
 * reference cloud, column major (NULL: all identity).  Otherwise exactly lsgpu_icp_compute. */
int lsgpu_icp_compute_clouds(lsgpu_icp* h, int reading_slot, const int* ref_slots, const float* ref_T,
                             int n_ref, const float T_init[16], const lsgpu_chain_config* chain,
                             float T_out[16], lsgpu_icp_stats* stats);
/* lsgpu_cloud_upload(h, reading_slot, reading_xyz1, nq) followed by lsgpu_icp_compute_clouds(h, reading_slot, ...), in one
 * call: the new scan (host memory) crosses PCIe WHILE the sub-map is assembled and filtered.  This is the call shape of
 * LaserTrack::processLaserScan -> localScanToSubMap (laser_slam/src/laser_track.cpp:112-119, 466-519): every scan is matched
 * exactly once, right after it arrived, against scans that are already resident; uploaded first and matched afterwards, a
 * 1 M-point scan's copy is 0.3 ms of idle device inside the reference's own timed region (scan_matching_times_,
 * laser_track.cpp:128, 208-209).  Same results, same draws, same return codes as the two calls one after the other; the
 * slot holds the scan on return whatever the registration's outcome.  `reading_slot` must not be one of `ref_slots`
 * (then, and for a device pointer or an empty cloud, the two calls are simply made one after the other). */
int lsgpu_icp_compute_clouds_upload(lsgpu_icp* h, int reading_slot, const float* reading_xyz1, int64_t nq,
                                    const int* ref_slots, const float* ref_T, int n_ref, const float T_init[16],
                                    const lsgpu_chain_config* chain, float T_out[16], lsgpu_icp_stats* stats);

/* ---- local-map maintenance on the device --------------------------------------------
 * What the ROS worker does to its local map between scans (laser_slam_ros/src/laser_slam_worker.cpp:415-488,
 * 522-540): cylindrical crop around the robot, voxel-grid down-sampling, rigid re-transform after a loop
 * closure (= lsgpu_transform_points).  Inputs / outputs: host or device pointers, 4 floats per point. */
/* applyCylindricalFilter (laser_slam_ros/include/laser_slam_ros/common.hpp:194-223): keeps the points with
 * (x-cx)^2 + (y-cy)^2 <= r^2 and |z-cz| <= height/2 (remove_point_inside: the points with >= in either test).
 * Order preserved.  out_xyz1 needs room for n points. */
int lsgpu_filter_cylinder(lsgpu_icp* h, const float* xyz1, int64_t n, const float center[3], double radius_m,
                          double height_m, int remove_point_inside, float* out_xyz1, int64_t* n_out);
/* pcl::VoxelGrid<PointXYZ> (laser_slam_worker.cpp:70-72, 439-440): one centroid (float sums in input order,
 * divided by the count) per voxel with >= min_points points, voxels in ascending index order.  LSGPU_BAD_ARG if
 * the voxel index would overflow an int (PCL refuses such leaf sizes as well). */
int lsgpu_filter_voxel_grid(lsgpu_icp* h, const float* xyz1, int64_t n, const float leaf[3], int min_points,
                            float* out_xyz1, int64_t* n_out);

/* ---- the input filter chain -------------------------------------------------
 * LaserTrack loads a libpointmatcher DataPointsFilters chain from `icp_input_filters_file` (laser_slam/src/
 * laser_track.cpp:24-30, LOG(FATAL) if the file cannot be opened) and applies it to every incoming scan before the
 * scan is stored or matched (laser_track.cpp:81, :146: input_filters_.apply(scan.scan)).  The filters below run on the
 * device, one after the other, each on the output of the previous one, order of the surviving points preserved:
 *   MaxDistDataPointsFilter      dim -1: keep |p| <  |maxDist|        dim 0..2: keep  p[dim]  <  maxDist (SIGNED, as upstream)
 *   MinDistDataPointsFilter      dim -1: keep |p| >  |minDist|        dim 0..2: keep |p[dim]| >  minDist
 *   BoundingBoxDataPointsFilter  inside = xMin < x < xMax && ...;     keeps inside (removeInside 0) or outside (1)
 *   FixStepSamplingDataPointsFilter  keeps points phase, phase + step, ...; phase = rand() % step; afterwards
 *                                step *= stepMult, clamped at endStep (the step persists from scan to scan: `state`)
 *   RandomSamplingDataPointsFilter   keeps point i iff draw_i < prob
 *   RemoveNaNDataPointsFilter        drops the points with a NaN among their four feature rows x, y, z, pad (Inf stays)
 *   VoxelGridDataPointsFilter        one point per occupied voxel of a grid anchored at the cloud's own minimum (below)
 *   OctreeGridDataPointsFilter       one point per leaf of an octree over the cloud, in depth-first leaf order (below)
 * (MaxPointCountDataPointsFilter is NOT offered: which points it keeps depends on the libpointmatcher version --
 *  std::random_shuffle in the 1.2 line, sequential selection sampling later -- and on the C++ library's shuffle; it
 *  cannot be restated from the reference, which configures none.  Unknown module names are configuration errors.)
 * |p| = sqrt(fma(z,z,fma(y,y,x*x))) in float.  Draws: the library's glibc-sequence stream (see lsgpu_icp_compute);
 * seed >= 0 reseeds it before the first filter.  LSGPU_NO_CONVERGENCE if a filter is handed an empty cloud
 * (PointMatcher::ConvergenceError "no points to filter" upstream); an empty chain copies the cloud.
 *
 * VoxelGridDataPointsFilter (libpointmatcher's module; NOT pcl::VoxelGrid of lsgpu_filter_voxel_grid, whose grid is anchored at
 * integer multiples of the leaf and whose output is in voxel-index order).  Restated from knowledge of upstream's
 * VoxelGridDataPointsFilter::inPlaceFilter, parity unpinned (DESIGN.md §5 choices 30-34).  lsgpu_point_filter: v[0..2] =
 * vSizeX / vSizeY / vSizeZ (default 1; finite and > 0), flag = useCentroid (default 1), dim = averageExistingDescriptors
 * (default 1); the last two take 0 or 1 only.  A bad parameter is LSGPU_BAD_CONFIG before anything runs.
 *   Arithmetic: float throughout, one rounding per operation (`/` is the correctly rounded division: the library is built
 *     without fast-math and with -ffp-contract=off, csrc/Makefile).
 *   Bounds, per axis a: minB = min_a / vSize_a, maxB = max_a / vSize_a (min / max over the cloud handed to the module),
 *     numDiv_a = (uint)((1.0f + maxB) - minB), numVox = numDivX numDivY numDivZ.  A numDiv of 0 (1 + maxB rounds to maxB
 *     once |maxB| >= 2^24) counts as 1.  numVox > 2^31 - 1: LSGPU_BAD_CONFIG "too many voxels" (InvalidParameter upstream).
 *   Voxel of a point: i = (uint)floorf(x / vSizeX - minBX), j, k likewise; idx = i + j numDivX + k numDivX numDivY.
 *     DEVIATION: i, j, k are clamped to numDiv - 1 -- upstream indexes out of range in the rounding corner where
 *     maxB - minB rounds up to an integer.
 *   The first point of a voxel is the one with the smallest input index in it.
 *   useCentroid 1: per coordinate, s starts as the first point's, every further point of the voxel is added in ascending input
 *     index (s += v), the result is s / (float)count.  useCentroid 0: the voxel's centre vSize_a (minB_a + (float)i_a + 0.5f),
 *     evaluated in that order.  The 4th component of the output point is the first point's (the facades' tag travels there).
 *   Output: one point per occupied voxel, in ascending order of the voxels' FIRST POINTS (upstream's sorted pointsToKeep),
 *     not in voxel-index order.  No draw is consumed.
 *   A NaN or +-inf coordinate in the cloud handed to the module: LSGPU_BAD_ARG (put RemoveNaNDataPointsFilter in front).
 *   Descriptors: the library sees none.  The C++ facade picks the first point's normal through the tag
 *     (averageExistingDescriptors 0); with averageExistingDescriptors 1 on a cloud that carries normals its apply() throws
 *     ConfigError -- averaging descriptors is not implemented.  Without descriptors both values are accepted.
 *   lsgpu_filter_voxel_grid_points is the host twin, bit for bit.
 *
 * OctreeGridDataPointsFilter (libpointmatcher's module, the 3-D case): one point per leaf of an octree over the cloud whose
 * leaves stop at maxPointByNode points or maxSizeByNode metres.  Restated from knowledge of upstream's
 * OctreeGridDataPointsFilter::inPlaceFilter and Octree_::build, parity unpinned (DESIGN.md §5 choices 49-54).
 * lsgpu_point_filter: v[0] = maxSizeByNode (default 0; finite, >= 0), v[1] = maxPointByNode (default 1; an integer in
 * [1, 2^24], carried as a float), dim = samplingMethod (default 0; 0 FirstPts, 1 RandomPts, 2 Centroid, 3 Medoid), flag =
 * buildParallel (default 1; 0 or 1, accepted and without effect).  Anything else is LSGPU_BAD_CONFIG, with the module and
 * the parameter named, before anything runs.
 *   Arithmetic: float throughout, one rounding per operation, as above.
 *   Root box, per axis a: ext_a = max_a - min_a over the cloud handed to the module, center_a = min_a + ext_a 0.5f;
 *     radius = max_a(ext_a) 0.5f.
 *   A node is a leaf if 2 radius <= maxSizeByNode, or it holds at most maxPointByNode points, or it is at depth 21 (the
 *     root is at depth 0).  DEVIATION: the depth cap -- upstream goes on halving until the radius underflows.  The cap
 *     matters only when more than maxPointByNode points lie within 2^-21 of the root's extent of each other (exact
 *     duplicates, say): they then share one leaf instead of a chain of ~130 more levels.
 *   Splitting: otherwise the node's points go to octant (x > cx) | (y > cy) << 1 | (z > cz) << 2.  Child o has radius' =
 *     radius 0.5f and center'_a = center_a + radius' if bit a of o is set, center_a - radius' if not.  Inside a node the
 *     points stay in ascending input index.
 *   Leaf order: the non-empty leaves are visited depth first, octants 0..7.  Output point k comes from the k-th visited leaf
 *     (what upstream's swap-and-lookup bookkeeping intends):
 *       FirstPts   the leaf's point with the smallest input index
 *       RandomPts  its point number (uint)((float)(count - 1) draw) in that order; ONE draw of the library's stream per
 *                  non-empty leaf, in visiting order -- no other method draws
 *       Centroid   per coordinate, s starts as the first point's, every further point is added in ascending input index,
 *                  the result is s / (float)count; the 4th component is the first point's
 *       Medoid     the point with the smallest sqrtf(dx dx + dy dy + dz dz) to that centroid, the sum left to right, strict
 *                  <: the earliest wins a tie
 *     The methods that return an input point return all four components of it (the facades' tag travels in the 4th).
 *   A NaN or +-inf coordinate in the cloud handed to the module: LSGPU_BAD_ARG (put RemoveNaNDataPointsFilter in front).
 *   Descriptors: the library sees none.  The C++ facade picks the chosen point's normal through the tag; Centroid on a cloud
 *     that carries normals makes its apply() throw ConfigError -- averaging descriptors is not implemented.
 *   The 2-D quadtree is not offered; the module stands in the input filter chain only, not in the filter sections of the ICP
 *   chain.  lsgpu_filter_octree_grid_points is the host twin, bit for bit. */
enum {
  LSGPU_FILTER_MAX_DIST = 1,
  LSGPU_FILTER_MIN_DIST = 2,
  LSGPU_FILTER_BOUNDING_BOX = 3,
  LSGPU_FILTER_FIX_STEP_SAMPLING = 4,
  LSGPU_FILTER_RANDOM_SAMPLING = 5,
  LSGPU_FILTER_REMOVE_NAN = 6,
  LSGPU_FILTER_VOXEL_GRID = 7,
  LSGPU_FILTER_OCTREE_GRID = 8
};
typedef struct lsgpu_point_filter {
  int    type;     /* LSGPU_FILTER_*                                                                          */
  int    dim;      /* Max/MinDist: -1 radial, 0..2 one axis   VoxelGrid: averageExistingDescriptors           */
                   /* OctreeGrid: samplingMethod                                                               */
  int    flag;     /* BoundingBox: removeInside               VoxelGrid: useCentroid                          */
                   /* OctreeGrid: buildParallel                                                                */
  int    pad_;
  float  v[6];     /* MaxDist {maxDist}  MinDist {minDist}  BoundingBox {xMin,xMax,yMin,yMax,zMin,zMax}        */
                   /* FixStepSampling {startStep,endStep,stepMult}  RandomSampling {prob}                      */
                   /* VoxelGrid {vSizeX,vSizeY,vSizeZ}  OctreeGrid {maxSizeByNode,maxPointByNode}              */
  double state;    /* FixStepSampling: current step (0: start at startStep); updated by every apply            */
} lsgpu_point_filter;
int lsgpu_apply_point_filters(lsgpu_icp* h, lsgpu_point_filter* filters, int n_filters, const float* xyz1,
                              int64_t n, int64_t seed, float* out_xyz1, int64_t* n_out);

/* ---- the ROS message surface of the scan path ----------------------------------
 * LaserSlamWorker::scanCallback turns the incoming sensor_msgs/PointCloud2 into DataPoints with
 * PointMatcher_ros::rosMsgToPointMatcherCloud<float> (laser_slam_ros/src/laser_slam_worker.cpp:125) and publishes
 * clouds through lpmToPcl / pcl::toROSMsg (laser_slam_ros/include/laser_slam_ros/common.hpp:159-191).  Both are
 * pure layout changes and run on the device so that a scan crosses PCIe once, as the message's byte block.
 *   from: `data` = the message's data block (n_points records of point_step bytes, host or device memory), the
 *         FLOAT32 fields x, y, z at byte offsets off_x/y/z inside a record (any alignment), optionally byte-swapped
 *         (is_bigendian); out = x,y,z,1 per point.  drop_non_finite (= !is_dense): records with a NaN / Inf
 *         coordinate are removed, order preserved.
 *   to  : x,y,z,1 -> the data block of a PointCloud2 / pcl::PointCloud<pcl::PointXYZ> with fields x@0 y@4 z@8,
 *         point_step 16 (what pcl::toROSMsg emits for PointXYZ; the 4th float of a record is padding, written 1). */
int lsgpu_cloud_from_pointcloud2(lsgpu_icp* h, const unsigned char* data, int64_t n_points, int point_step, int off_x,
                                 int off_y, int off_z, int is_bigendian, int drop_non_finite, float* out_xyz1,
                                 int64_t* n_out);
int lsgpu_cloud_to_pointxyz(lsgpu_icp* h, const float* xyz1, int64_t n, unsigned char* out_data /* 16 n bytes */);

/* ---- host-side versions of the two filters (same output as the device filters) and O(1) helpers ---- */

/* RandomSamplingDataPointsFilter (yaml:1-3): keep i iff draw_i < prob; seed as above. */
int64_t lsgpu_filter_random_sampling(int64_t n, float prob, int64_t seed, int64_t* keep_idx);
/* SamplingSurfaceNormalDataPointsFilter (yaml:5-7), samplingMethod 0, keepNormals 1. */
int64_t lsgpu_filter_sampling_surface_normal(const float* xyz1, int64_t n, int knn, float ratio,
                                             int64_t seed, float* out_xyz1, float* out_normals);
/* SurfaceNormalDataPointsFilter on the host (a checker: sort-based exact search): the contract and the outputs of
 * lsgpu_icp_filter_reference_normals, bit for bit.  Returns LSGPU_OK or LSGPU_BAD_ARG. */
int lsgpu_filter_surface_normal(const float* xyz1, int64_t n, int knn, float* out_normals, int32_t* out_ids,
                                float* out_d2);
/* VoxelGridDataPointsFilter of the input filter chain on the host (no GPU, no handle): upstream's sequential loop with the
 * contract and the float arithmetic above, bit for bit the output of lsgpu_apply_point_filters with this one module.
 * out_xyz1 needs room for n points.  Returns the number of output points, or -LSGPU_BAD_CONFIG (a bad vsize / use_centroid,
 * too many voxels), -LSGPU_BAD_ARG (a NULL pointer, a NaN or infinite coordinate), -LSGPU_NO_CONVERGENCE (n <= 0). */
int64_t lsgpu_filter_voxel_grid_points(const float* xyz1, int64_t n, const float vsize[3], int use_centroid,
                                       float* out_xyz1);
/* OctreeGridDataPointsFilter of the input filter chain on the host (no GPU, no handle): the sequential recursion itself, with
 * the contract and the float arithmetic above, bit for bit the output of lsgpu_apply_point_filters with this one module.
 * seed >= 0 reseeds the library's draw stream first; RandomPts (sampling_method 1) then takes one draw per non-empty leaf.
 * out_xyz1 needs room for n points.  Returns the number of output points, or -LSGPU_BAD_CONFIG (a bad max_size_by_node /
 * max_point_by_node / sampling_method), -LSGPU_BAD_ARG (a NULL pointer, a NaN or infinite coordinate),
 * -LSGPU_NO_CONVERGENCE (n <= 0). */
int64_t lsgpu_filter_octree_grid_points(const float* xyz1, int64_t n, float max_size_by_node, int max_point_by_node,
                                        int sampling_method, int64_t seed, float* out_xyz1);
/* RigidTransformation::checkParameters / correctParameters (common.hpp:136-149). */
int  lsgpu_check_rigid(const float T[16]);
void lsgpu_correct_rigid(const float T[16], float out[16]);
/* The rotation metric of DifferentialTransformationChecker (yaml:24-27) between two 4x4 transforms (column major):
 * Quaternion(R_a).angularDistance(Quaternion(R_b)) = 2 atan2(|vec|, |w|) of q_a * conj(q_b), in float -- the same code
 * the device-side checker runs (csrc/lsgpu_host_math.h). */
float lsgpu_rotation_distance(const float Ta[16], const float Tb[16]);

/* ---- RobustOutlierFilter: M-estimator weights with a MAD scale (DESIGN.md §3 "RobustOutlierFilter", §5 choices 18-23) ----
 * The one outlier filter whose weights are real numbers.  Per iteration, over the matches every other outlier filter sees:
 *   scale     none: 1.  mad: over the m valid (finite) squared match distances d2, med = sorted(d2)[m / 2],
 *             mad = sorted(|d2 - med|)[m / 2] (float), scale = sqrtf(mad); recomputed in iteration it (1-based, restarted by
 *             every align) iff nb_iteration_for_scale == 0 || it <= nb_iteration_for_scale, else the last scale is kept.
 *             Always the matcher's point-to-point d2.  No valid match or scale == 0: LSGPU_NO_CONVERGENCE, T_out = T_init.
 *   distance  point2point: e = d2.  point2plane: e = r r, r = n . (p - q) as the point-to-plane pass computes it (float).
 *   weight    e2 = e / (scale scale), k = tuning, k2 = k k, float, one operation per rounding:
 *             cauchy 1 / (1 + e2 / k2)   huber e2 < k2 ? 1 : k / sqrtf(e2)   tukey e2 < k2 ? (1 - e2 / k2)^2 : 0
 *             gm k2 / (k + e2)^2   sc e2 > k ? 4 k2 / (k + e2)^2 : 1   L1 1 / sqrtf(e2);
 *             approximation finite: w = 0 where e2 >= approximation^2.  A non-finite weight: LSGPU_NO_CONVERGENCE.
 *   The weights of all outlier filters multiply; a pair with weight 0 or an invalid match is not used; n_used counts the pairs
 *   with w > 0; limit stays the binary filters' effective upper limit (+inf with none).  Point-to-plane: A = sum w J J^T,
 *   b = -sum w J r.  Point-to-point: sum w p, sum w q, sum w q p^T; slot 27 = sum w, slot 28 = sum w e^2 -- in the sums of
 *   lsgpu_normal_eq / lsgpu_point_to_point as well (their scale: the MAD of the d2 they are given, or 1).
 *   With matcher_knn = k >= 2 every pair is weighted on its own.  A handle with the filter takes the chain plan
 *   (csrc/lsgpu_policy.h); lsgpu_icp_comm_init refuses it.  welsch / student and the berg / std scale estimators are
 *   LSGPU_BAD_CONFIG (exp / pow cannot be made bit-identical between host and device). */
enum { LSGPU_ROBUST_CAUCHY = 0, LSGPU_ROBUST_HUBER = 1, LSGPU_ROBUST_TUKEY = 2, LSGPU_ROBUST_GM = 3, LSGPU_ROBUST_SC = 4,
       LSGPU_ROBUST_L1 = 5, LSGPU_ROBUST_WELSCH = 6 /* refused */, LSGPU_ROBUST_STUDENT = 7 /* refused */ };
enum { LSGPU_ROBUST_SCALE_NONE = 0, LSGPU_ROBUST_SCALE_MAD = 1, LSGPU_ROBUST_SCALE_BERG = 2 /* refused */,
       LSGPU_ROBUST_SCALE_STD = 3 /* refused */ };
enum { LSGPU_ROBUST_DIST_POINT2POINT = 0, LSGPU_ROBUST_DIST_POINT2PLANE = 1 };
typedef struct lsgpu_robust_config {
  int   robust_fct;              /* LSGPU_ROBUST_*            robustFct            (cauchy)      */
  float tuning;                  /*                           tuning               (1.0)         */
  int   scale_estimator;         /* LSGPU_ROBUST_SCALE_*      scaleEstimator       (mad)         */
  int   nb_iteration_for_scale;  /*                           nbIterationForScale  (0: always)   */
  int   distance_type;           /* LSGPU_ROBUST_DIST_*       distanceType         (point2point) */
  float approximation;           /*                           approximation        (+inf: none)  */
  int   reserved[2];             /* 0 */
} lsgpu_robust_config;
void lsgpu_robust_config_default(lsgpu_robust_config* c);   /* the module's defaults */
/* What lsgpu_icp_set_robust_filter accepts, without a handle or a device: LSGPU_OK, or LSGPU_BAD_CONFIG for a refused or
 * unknown value, a negative or NaN tuning / approximation, a negative nb_iteration_for_scale, or point2plane on a
 * point-to-point handle (error_minimizer: LSGPU_MINIMIZER_*) whose reference has no normals (have_normals 0). */
int lsgpu_robust_config_check(const lsgpu_robust_config* c, int error_minimizer, int have_normals);
/* Gives the handle the filter (cfg is copied), NULL removes it.  Bad values: LSGPU_BAD_CONFIG before the device is touched
 * (the handle keeps what it had).  point2plane on a point-to-point handle is checked again by align, which knows whether
 * set_reference was given normals. */
int lsgpu_icp_set_robust_filter(lsgpu_icp* h, const lsgpu_robust_config* cfg);
/* Host twins (no GPU, no handle), bit-identical with the device loop.  lsgpu_robust_scale: median and MAD scale of the finite
 * entries of d2 (+inf = invalid match); LSGPU_NO_CONVERGENCE if there is none.  lsgpu_robust_weights: w_out[i] of e[i]
 * (d2, or r r for point2plane) under cfg's function, tuning and approximation with the given scale. */
int lsgpu_robust_scale(const float* d2, int64_t n, float* median, float* scale);
int lsgpu_robust_weights(const lsgpu_robust_config* cfg, float scale, const float* e, int64_t n, float* w_out);
/* One record per iteration of the last align of a handle with the filter; returns the number written. */
typedef struct lsgpu_robust_trace {
  float  median;       /* of the valid d2 when the scale was last computed (0 with none)       */
  float  scale;        /* the scale the iteration's weights used                                */
  double w_sum;        /* sum of the weights of the used pairs (slot 27)                        */
  int    recomputed;   /* 1: the scale was computed in this iteration                           */
  int    reserved;
} lsgpu_robust_trace;
int lsgpu_icp_get_robust_trace(lsgpu_icp* h, lsgpu_robust_trace* out, int cap);
/* The point-to-plane step from the 27 sums of lsgpu_normal_eq (21 upper-tri of A, 6 of b): dT (4x4 float, column major).
 * Host only; the same function the device loop runs, bit for bit -- the sibling of lsgpu_point_to_point_solve.
 * LSGPU_NO_CONVERGENCE if A is not positive definite. */
int lsgpu_point_to_plane_solve(const double sums[27], float dT[16]);

/* ---- SurfaceNormalOutlierFilter, reading normals and oriented normals (DESIGN.md §3 "SurfaceNormalOutlierFilter", §5 choices 24-29) ----
 * SurfaceNormalOutlierFilter (maxAngle): eps = (float)cos((double)maxAngle), taken once when the filter is given to the handle.
 *   Per iteration, for reading point x and each of its k matches: an invalid match has weight 0; else
 *   nr = normalized(R_iter n0[x]), n0 = R_init n_reading[x] the reading normal as step 5 of ICP::compute moves it with the
 *   reading (once per alignment; R_iter is the rotation of the iteration's T_iter and is applied to n0, never to the last
 *   iteration's result), both rotations with the fma chain of lsgpu_rotate_descriptors; nf = normalized(n_reference[id]);
 *   v = fma(nr.z, nf.z, fma(nr.y, nf.y, nr.x nf.x)); weight 0 iff v < eps (a NaN v keeps the pair).
 *   normalized(a) = a / sqrtf(fma(az, az, fma(ay, ay, ax ax))), a vector of length 0 stays as it is.
 *   The weight multiplies those of the other outlier filters: the trim / median order statistics still see every valid
 *   distance, n_used counts the pairs of weight > 0, limit keeps its meaning, nothing kept is LSGPU_NO_CONVERGENCE.
 *   Without reading normals (plain lsgpu_icp_align) or without reference normals the filter is inert.  A handle with the
 *   filter takes the chain plan; lsgpu_icp_comm_init refuses it.  lsgpu_normal_eq / lsgpu_point_to_point are handed no
 *   reading normals and do not apply the test.
 * Orientation (ObservationDirectionDataPointsFilter {x, y, z} directly followed by OrientNormalsDataPointsFilter
 *   {towardCenter}): for every point p of the cloud in the frame it was given in, o = sensor - p (three float subtractions),
 *   s = fma(o.z, n.z, fma(o.y, n.y, o.x n.x)); n is negated if s < 0 (towardCenter 1) or s > 0 (towardCenter 0).
 * Reading normals (reading_sn_knn): the contract of lsgpu_icp_filter_reference_normals on the reading's KEPT points (after
 *   RandomSamplingDataPointsFilter); fewer kept points than knn: LSGPU_BAD_ARG.  lsgpu_icp_compute then runs on one stream
 *   (the reading's side cannot overlap the reference's grid build: both use the handle's grid). */
typedef struct lsgpu_normals_config {
  float max_angle;              /* SurfaceNormalOutlierFilter maxAngle [rad], 0 .. 3.1416 (1.57); < 0: no such filter      */
  int   reading_sn_knn;         /* SurfaceNormalDataPointsFilter on the reading: knn 3..32; 0: absent                      */
  int   reading_orient;         /* orientation pair on the reading: 0 off, 1 towardCenter, 2 away                          */
  int   reference_orient;       /* ... on the reference                                                                    */
  float reading_sensor[3];      /* ObservationDirectionDataPointsFilter x, y, z of the reading section                     */
  float reference_sensor[3];    /* ... of the reference section                                                            */
  int   reading_normals_given;  /* 1: the caller hands the reading normals to lsgpu_icp_align_normals (kernel-level use)   */
  int   reserved[1];            /* 0 */
} lsgpu_normals_config;
void lsgpu_normals_config_default(lsgpu_normals_config* c);   /* no filter, no reading normals, no orientation */
/* Without a handle or a device: LSGPU_OK, or LSGPU_BAD_CONFIG for a value out of range, an orientation without normals in
 * front of it, the outlier filter without reading normals or without reference normals (have_reference_normals 0), or
 * reading normals that no module reads (max_angle < 0). */
int lsgpu_normals_config_check(const lsgpu_normals_config* c, int error_minimizer, int have_reference_normals);
/* Gives the handle the configuration (copied), NULL removes it.  Bad values: LSGPU_BAD_CONFIG before the device is touched. */
int lsgpu_icp_set_normals(lsgpu_icp* h, const lsgpu_normals_config* cfg);
/* SurfaceNormalDataPointsFilter on a reading, then (orient 1 / 2) the orientation towards / away from sensor[3] (nullable
 * with orient 0): out_normals 3 floats per point, in the cloud's order.  The search runs on a grid of its own: the
 * handle's reference is what it was. */
int lsgpu_icp_reading_normals(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, int orient, const float sensor[3],
                              float* out_normals);
/* lsgpu_icp_align with the reading's normals (3 floats per point, the reading's order; NULL: lsgpu_icp_align). */
int lsgpu_icp_align_normals(lsgpu_icp* h, const float* reading_xyz1, int64_t nq, const float* reading_normals,
                            const float T_init[16], float T_out[16], lsgpu_icp_stats* stats);
/* The reference normals the handle holds, in the order the reference was given to set_reference (3 floats per point; after
 * lsgpu_icp_compute: the filtered reference's).  LSGPU_BAD_ARG without normals. */
int lsgpu_icp_get_reference_normals(lsgpu_icp* h, float* out_normals, int64_t cap_points);
/* Host twins (no GPU, no handle), bit-identical with the device.  lsgpu_orient_normals flips `normals` in place (mode 1 / 2).
 * lsgpu_normal_angle_weights: w[i k + j] of reading point i's j-th match ids[i k + j] (< 0: invalid, weight 0) under T
 * (4x4 column major: its rotation is applied to reading_normals, which are n0 above). */
int lsgpu_orient_normals(const float* xyz1, int64_t n, const float sensor[3], int mode, float* normals);
int lsgpu_normal_angle_weights(const float T[16], const float* reading_normals, int64_t nq, const float* reference_normals,
                               const int32_t* ids, int k, float max_angle, float* w);
/* One record per iteration of the last align that applied the filter; returns the number written. */
typedef struct lsgpu_normal_angle_trace {
  int64_t rejected;   /* pairs the angle test alone rejected: valid, kept by every binary distance filter, v < eps */
  float   eps;
  int     reserved;
} lsgpu_normal_angle_trace;
int lsgpu_icp_get_normal_angle_trace(lsgpu_icp* h, lsgpu_normal_angle_trace* out, int cap);

/* ---- the module chain of a YAML document: PointMatcher::ICP::loadFromYaml (laser_slam/src/laser_track.cpp:17) ----
 * One rule set for every front end (csrc/lsgpu_chain_loader.cpp; DESIGN.md §3 "The chain loader").  A front end parses the
 * YAML syntax and hands over the modules in document order: the top-level section, the module's name and its parameters, every
 * value as the scalar's TEXT ("0.75", ".inf", "huber").  The library decides the rest: which modules the device path has, their
 * parameters, defaults and ranges, what may be given once, the order inside the two filter sections, and what the loop cannot
 * run without.  Modules of the sections `inspector` and `logger` are skipped; any other unknown section or module is refused.
 * Host only: no handle, no device. */
typedef struct lsgpu_yaml_param  { const char* key; const char* value; } lsgpu_yaml_param;
typedef struct lsgpu_yaml_module {
  const char* section;              /* "readingDataPointsFilters", "matcher", ...                                  */
  const char* name;                 /* "RandomSamplingDataPointsFilter", ...                                       */
  const lsgpu_yaml_param* params;   /* n_params of them (NULL with 0)                                              */
  int n_params;
  int reserved;                     /* 0 */
} lsgpu_yaml_module;
typedef struct lsgpu_loaded_chain {
  lsgpu_icp_config     icp;         /* trim ratio (1: no TrimmedDist), checkers (no Differential: -1, -1, 1), minimizer,
                                     * matcher knn / maxDist, Max- / Min- / MedianDist thresholds; the rest as _config_default */
  lsgpu_chain_config   chain;       /* reading_prob (< 0: no reading filter), ssn_knn, ssn_ratio, sn_knn; seed -1  */
  lsgpu_robust_config  robust;      /* RobustOutlierFilter (the module's defaults with has_robust 0)               */
  int has_robust;
  lsgpu_normals_config normals;     /* SurfaceNormalOutlierFilter, reading normals, orientation pairs              */
  int has_normals;                  /* 0: none of these modules (normals holds lsgpu_normals_config_default)       */
  int reserved[6];                  /* [0] = 1: errorMinimizer PointToPlaneWithCovErrorMinimizer (icp.error_minimizer stays
                                     * LSGPU_MINIMIZER_POINT_TO_PLANE), [1] = the IEEE-754 bits of (float)sensorStdDev then, else 0;
                                     * read them with lsgpu_loaded_chain_covariance.  [2], [3] = the number of cut modules in
                                     * the reading / reference section (the modules: lsgpu_chain_load_cuts).  [4] = 1: MaxDensityDataPointsFilter
                                     * behind the reference's SurfaceNormalDataPointsFilter, [5] = the IEEE-754 bits of (float)maxDensity
                                     * then, else 0; read them with lsgpu_loaded_chain_max_density */
} lsgpu_loaded_chain;
/* LSGPU_OK and *out (every byte of it, padding 0), or LSGPU_BAD_CONFIG with the reason -- the module's name in it, or the
 * section's for an unknown section -- written to why[0 .. why_cap), truncated if need be and always NUL-terminated; *out is
 * then left as it was.  why may be NULL.  NULL pointers inside mods, or a NULL out: LSGPU_BAD_ARG. */
int lsgpu_chain_load(const lsgpu_yaml_module* mods, int n_mods, lsgpu_loaded_chain* out, char* why, int why_cap);
/* The reason lsgpu_robust_config_check / lsgpu_normals_config_check refuse a configuration (a static string, the module's
 * name in it), or NULL where they return LSGPU_OK: what ICP::loadFromYaml (laser_track.cpp:17) reports for such a module. */
const char* lsgpu_robust_config_why(const lsgpu_robust_config* c, int error_minimizer, int have_normals);
const char* lsgpu_normals_config_why(const lsgpu_normals_config* c, int error_minimizer, int have_reference_normals);

/* ---- PointToPlaneWithCovErrorMinimizer: the covariance of an alignment (DESIGN.md §3 "PointToPlaneWithCovErrorMinimizer", §5 choice 35) ----
 * The module solves the step of PointToPlaneErrorMinimizer -- T_out, the statistics and the trace of a handle do not change
 * with it -- and estimates the 6x6 covariance of the result (Censi's closed form; upstream: errorMinimizer->getCovariance()).
 * Everything in the reference-mean frame, as lsgpu_normal_eq.  The pairs are those of the LAST EXECUTED iteration at the
 * pose it matched at: p = the reading point at T_iter before that iteration's update, q = its match, n = the match's normal;
 * a pair counts iff that iteration gave it a non-zero weight (a valid match, lo2 <= d2 <= limit with the iteration's effective
 * upper limit and MinDistOutlierFilter's lo2).  dT = that iteration's step (lsgpu_point_to_plane_solve).  In double on the host:
 *   beta = -asin(dT(2,0)), alpha = atan2(dT(2,1), dT(2,2)), gamma = atan2(dT(1,0) / cos beta, dT(0,0) / cos beta),
 *   w = (alpha, beta, gamma), t = dT(0..2, 3), each rounded to float.  Per pair, float, one rounding per operation, sums of
 *   three terms left to right ((x + y) + z):
 *   r_p = sqrtf(p.p), u = p / r_p, r_q = sqrtf(q.q), v = q / r_q, m = u x n, c = w x p, g = w x u,
 *   E = n . (((p + c) + t) - q), N_rd = n . (u + g), N_rf = -(n . v),
 *   h = [n ; r_p m]   a = [n N_rd ; m (E + r_p N_rd)]   b = [n N_rf ; (r_q m) N_rf]      (translation first, then rotation)
 *   H = sum h h^T, M = sum (a a^T + b b^T): the products and the sums in double.  cov = sensorStdDev^2 H^-1 M H^-1 in double.
 * The weights of the outlier filters are not applied (upstream ignores them here).  r_p = 0 or r_q = 0 (a point exactly on the
 * reference mean) divides by zero as upstream does: the sums become non-finite, which counts as singular.
 * Scope: knn 1, any subset of Trimmed- / Max- / Min- / MedianDistOutlierFilter, KDTreeMatcher maxDist.  A handle with
 * matcher_knn >= 2, RobustOutlierFilter, SurfaceNormalOutlierFilter, the point-to-point minimizer or a communicator refuses
 * lsgpu_icp_set_covariance (LSGPU_BAD_CONFIG, the module named in lsgpu_last_error), and a handle with the covariance refuses
 * those (lsgpu_icp_set_robust_filter, lsgpu_icp_set_normals with max_angle >= 0, lsgpu_icp_comm_init).
 * Cost: one exact search at the last iteration's pose and one pass over its pairs after the loop, only on handles that asked. */
typedef struct lsgpu_covariance_config {
  float sensor_std_dev;   /* sensorStdDev [m] (0.01): finite and >= 0 */
  int   reserved[3];      /* 0 */
} lsgpu_covariance_config;
void lsgpu_covariance_config_default(lsgpu_covariance_config* c);
/* Switches the covariance on (cfg is copied), NULL switches it off.  Bad values and the refused combinations above:
 * LSGPU_BAD_CONFIG before the device is touched (the handle keeps what it had). */
int lsgpu_icp_set_covariance(lsgpu_icp* h, const lsgpu_covariance_config* cfg);
typedef struct lsgpu_icp_quality {
  double  covariance[36];   /* row major, symmetric; order x y z (translation), then alpha beta gamma (rotation about x, y, z) */
  double  residual;         /* sum (n . (p - q))^2 over the pairs                                                          */
  int64_t n_pairs;          /* == lsgpu_icp_stats.final_n_used                                                             */
  float   used_ratio;       /* n_pairs / nq: getWeightedPointUsedRatio of a binary chain                                   */
  int     reserved[3];      /* 0 */
} lsgpu_icp_quality;
/* The quality record of the handle's LAST alignment (lsgpu_icp_align, _align_normals, _compute, _compute_clouds,
 * _compute_clouds_upload; after lsgpu_icp_align_batch: of the last pair each handle ran).  LSGPU_BAD_CONFIG if the covariance
 * is not switched on (the reason in lsgpu_last_error); LSGPU_NO_CONVERGENCE if there was no alignment yet, the last one did not
 * return LSGPU_OK, or H is singular; *out is written only with LSGPU_OK. */
int lsgpu_icp_get_quality(lsgpu_icp* h, lsgpu_icp_quality* out);
/* Kernel-level entry, the inputs of lsgpu_normal_eq plus the step: out[0..20] = upper triangle of H (row major, a <= c),
 * [21..41] = of M, [42] = the pair count, [43] = sum (n . (p - q))^2.  A pair counts iff its id is valid, d2 <= limit and
 * d2 >= the handle's MinDistOutlierFilter threshold squared.  dT NULL: the identity.  Reproducible run to run. */
int lsgpu_point_to_plane_cov(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16], const int32_t* ids,
                             const float* d2, float limit, const float dT[16], double out[44]);
/* cov (row major 6x6, one triangle computed and mirrored) from those 44 sums.  Host only (no GPU, no handle); the function the
 * library itself calls after the loop, bit for bit.  LSGPU_NO_CONVERGENCE, cov untouched: a pair count <= 0, a non-finite sum,
 * or a singular H -- a Cholesky pivot of H no greater than 1e-6 times its own diagonal entry (the accuracy of the float
 * per-pair terms: below it the data do not determine the direction).  LSGPU_BAD_CONFIG: sensor_std_dev negative or non-finite. */
int lsgpu_point_to_plane_cov_solve(const double sums[44], float sensor_std_dev, double cov[36]);
/* The covariance slots of a loaded chain: 1 and *sensor_std_dev (nullable) if the document names
 * PointToPlaneWithCovErrorMinimizer, else 0 and *sensor_std_dev untouched.  Host only.  (An exported function, not an inline one:
 * every function this header names is a symbol of the library, which is what the FFI front ends bind.) */
int lsgpu_loaded_chain_covariance(const lsgpu_loaded_chain* c, float* sensor_std_dev);

/* ---- cut modules in the ICP chain (DESIGN.md §3 "Cut modules in the ICP chain") ----------------------------------------
 * A cut module is one of the four stateless per-point predicates of the input filter chain above: MaxDist- (type 1), MinDist-
 * (2), BoundingBox- (3) and RemoveNaNDataPointsFilter (6), as lsgpu_point_filter records with the semantics stated there
 * (`state` and `pad_` are not read).  In readingDataPointsFilters / referenceDataPointsFilters of an ICP chain they run INSIDE
 * lsgpu_icp_compute / _compute_clouds / _compute_clouds_upload:
 *   Reference section: up to LSGPU_CHAIN_CUT_MAX modules, any order, in front of the normals module (ssn_knn / sn_knn; none on a
 *     point-to-point chain).  Applied to the reference as handed to compute (the assembled sub-map of _compute_clouds), before
 *     the sampling filter and before centring.  sn_knn larger than the surviving count: LSGPU_BAD_ARG.
 *   Reading section: up to LSGPU_CHAIN_CUT_MAX modules, any order, reading[0 .. reading_sampling_at) in front of
 *     RandomSamplingDataPointsFilter (chain.reading_prob >= 0) and the rest behind it; all of them in front of the reading's
 *     normals.  Applied to the reading in its own frame, before T_init; an uploaded slot is never modified.
 *   Order of the surviving points is preserved; a cut module consumes no draw; RandomSampling draws once per point that reaches
 *     it -- once per survivor of the modules in front of it, the draw's index the point's rank among them.  After the call the
 *     library's draw stream stands where the sequential chain (lsgpu_apply_point_filters per section, reference first) leaves it.
 *   A section that leaves no point: LSGPU_NO_CONVERGENCE ("... filter left no point").
 * Each section is ONE fused pass whatever it holds (csrc/lsgpu_chain_cut.hip.h); a handle without cut modules enqueues what it
 * always did.  The split-scan mode (lsgpu_icp_comm_init) refuses a handle with cut modules, and the other way round. */
#define LSGPU_CHAIN_CUT_MAX 8
typedef struct lsgpu_chain_cuts {
  int n_reading, n_reference;   /* 0 .. LSGPU_CHAIN_CUT_MAX each                                                                 */
  int reading_sampling_at;      /* reading modules in front of RandomSampling, 0 .. n_reading; ignored without RandomSampling   */
  int reserved;                 /* 0 */
  lsgpu_point_filter reading[LSGPU_CHAIN_CUT_MAX], reference[LSGPU_CHAIN_CUT_MAX];
} lsgpu_chain_cuts;
/* Gives the handle the cut modules (copied); NULL or two zero counts switch them off.  LSGPU_BAD_CONFIG, the module named in
 * lsgpu_last_error and the handle left as it was: a type other than 1, 2, 3, 6, a dim outside -1..2 (Max- / MinDist), a count out of
 * range, a handle with a communicator.  reading_sampling_at is clamped to 0 .. n_reading. */
int lsgpu_icp_set_chain_cuts(lsgpu_icp* h, const lsgpu_chain_cuts* cuts);
/* The fused pass of one section alone (kernel-level entry).  side 0: cuts->reading with RandomSampling of probability prob at
 * position cuts->reading_sampling_at (prob < 0: no RandomSampling); side 1: cuts->reference, prob ignored.  The handle's own
 * cut modules are not read.  seed as lsgpu_apply_point_filters; xyz1 / out_xyz1 host or device pointers, out_xyz1 with room
 * for n points.  CONTRACT: the output points and the draws consumed equal lsgpu_apply_point_filters with the same modules in
 * the same order (RandomSampling as a type 5 module at its position), except that a section emptied by a module that is not
 * its last returns LSGPU_OK with *n_out = 0 where the sequential chain reports LSGPU_NO_CONVERGENCE.  n == 0 with a module:
 * LSGPU_NO_CONVERGENCE, as there. */
int lsgpu_icp_filter_section(lsgpu_icp* h, const lsgpu_chain_cuts* cuts, int side, float prob, const float* xyz1, int64_t n,
                             int64_t seed, float* out_xyz1, int64_t* n_out);
/* The cut modules of a YAML document: the rules, the refusals and the texts of lsgpu_chain_load (which writes their counts to
 * lsgpu_loaded_chain.reserved[2], [3]: reading, reference), the modules themselves in *out (every byte, padding 0).
 * Parameters and defaults: MaxDist {dim -1, maxDist 1}, MinDist {dim -1, minDist 1}, BoundingBox {xMin -1, xMax 1, yMin -1,
 * yMax 1, zMin -1, zMax 1, removeInside 1}, RemoveNaN {} -- those of the input filter chain's front ends.  dim an integer in
 * -1..2, removeInside 0 or 1, the limits numbers (inf allowed).  Host only. */
int lsgpu_chain_load_cuts(const lsgpu_yaml_module* mods, int n_mods, lsgpu_chain_cuts* out, char* why, int why_cap);

/* ---- MaxDensityDataPointsFilter behind SurfaceNormalDataPointsFilter keepDensities 1 (DESIGN.md §3 "Thinning the dense near
 * range", §5 choices 36-40) ----------------------------------------------------------------------------------------------
 * The reference section  SurfaceNormalDataPointsFilter {knn, keepDensities 1}, MaxDensityDataPointsFilter {maxDensity}  [,
 * ObservationDirectionDataPointsFilter, OrientNormalsDataPointsFilter]: normals and densities on the whole cloud, then the dense
 * near range is thinned.  Restated from knowledge of upstream, parity unpinned.
 *   Density of point i: the knn neighbourhood of lsgpu_icp_filter_reference_normals, in its order, on the centred cloud;
 *     mean = box_normal's mean, bit for bit; e_j = p_j - mean; r = sqrtf(max_j ((ex ex + ey ey) + ez ez));
 *     volume = (float)(4/3 pi) * ((r r) r); density = (float)knn / volume.  Float, one rounding per operation, no pow
 *     (csrc/lsgpu_density.h, shared by host and device).  r == 0 (knn identical points): +inf.
 *   MaxDensityDataPointsFilter {maxDensity: default 10, in (0, inf]}, over the cloud in the order given: last = the largest
 *     non-NaN density; sat = 0 if every point's density equals last, else 1 (upstream's integer division 1 - nbSaturated / n).
 *     A point with density > maxDensity takes ONE draw, (float)rand() / (float)RAND_MAX, and is kept iff draw < accept,
 *     accept = maxDensity / density (a float division), multiplied by (float)sat if density == last.  Every other point -- a
 *     NaN density included -- is kept and takes no draw.  Order preserved.  A +inf density: accept 0, dropped, its draw
 *     consumed.  The draw of a dense point is indexed by its rank among the dense points; afterwards the library's draw stream
 *     stands n_dense draws further on, and the reading section's draws start there.
 *   In lsgpu_icp_compute (a handle with lsgpu_icp_set_max_density, chain->sn_knn > 0): the reference's cut modules, the grid of
 *     the whole surviving cloud, normals + densities on it, the thinning pass; the thinned cloud and its normals then go on as
 *     SamplingSurfaceNormalDataPointsFilter's output does (orientation, centring on the THINNED cloud's mean, grid, loop).  The
 *     reading's filter runs behind the count of dense points, on one stream.  Nothing kept: LSGPU_NO_CONVERGENCE ("compute: the
 *     reference filter left no point").  A point-to-point handle runs the densities and the thinning too.  chain->sn_knn == 0
 *     on such a handle: LSGPU_BAD_CONFIG.  A handle without the module enqueues what it always did.
 *   Not together with the split-scan mode (lsgpu_icp_comm_init) or PointToPlaneWithCovErrorMinimizer (lsgpu_icp_set_covariance):
 *     LSGPU_BAD_CONFIG, the module named in lsgpu_last_error, whichever of the two calls comes second.
 *   Loader: the module may stand only in referenceDataPointsFilters, directly behind SurfaceNormalDataPointsFilter with
 *     keepDensities 1 and in front of the orientation pair, once.  keepDensities 1 with no MaxDensityDataPointsFilter behind it
 *     stays refused (nothing would read the densities), as it is on the reading side. */
typedef struct lsgpu_max_density_config {
  float max_density;   /* maxDensity [points / m^3] (10): > 0, +inf allowed, not NaN */
  int   reserved[3];   /* 0 */
} lsgpu_max_density_config;
void lsgpu_max_density_config_default(lsgpu_max_density_config* c);
/* Without a handle or a device: LSGPU_OK / NULL, or LSGPU_BAD_CONFIG / the reason (a static string, the module's name in it)
 * for a maxDensity that is not > 0, or sn_knn <= 0: no SurfaceNormalDataPointsFilter in front of the module. */
int lsgpu_max_density_config_check(const lsgpu_max_density_config* c, int sn_knn);
const char* lsgpu_max_density_config_why(const lsgpu_max_density_config* c, int sn_knn);
/* Gives the handle the module (cfg is copied), NULL removes it.  A bad maxDensity and the refused combinations above:
 * LSGPU_BAD_CONFIG before the device is touched (the handle keeps what it had). */
int lsgpu_icp_set_max_density(lsgpu_icp* h, const lsgpu_max_density_config* cfg);
/* lsgpu_icp_filter_reference_normals with the densities: out_densities (nullable) one float per point, in the cloud's order.
 * Without out_densities it is that function: the same launches, the same outputs. */
int lsgpu_icp_filter_reference_normals_densities(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float* out_normals,
                                                 int32_t* out_ids, float* out_d2, float* out_densities);
/* The two modules on a cloud (kernel-level entry): out_xyz1 (4 floats / point) and out_normals (3 floats / point) need room for n
 * points, out_xyz1 must not be xyz1; out_densities (nullable): one float per INPUT point; *n_out points kept, *n_dense draws
 * consumed.  seed as lsgpu_icp_filter_reading.  Host or device pointers.  LSGPU_NO_CONVERGENCE if nothing is kept (the draws are
 * consumed).  The call leaves the WHOLE cloud as the handle's reference, as lsgpu_icp_filter_reference_normals does. */
int lsgpu_icp_filter_reference_max_density(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float max_density, int64_t seed,
                                           float* out_xyz1, float* out_normals, float* out_densities, int64_t* n_out,
                                           int64_t* n_dense);
/* Host twins (no GPU, no handle), bit-identical with the device: lsgpu_filter_surface_normal with the densities beside the
 * normals, and the two modules with the outputs of lsgpu_icp_filter_reference_max_density (host pointers). */
int lsgpu_filter_surface_normal_densities(const float* xyz1, int64_t n, int knn, float* out_normals, int32_t* out_ids,
                                          float* out_d2, float* out_densities);
int lsgpu_filter_max_density(const float* xyz1, int64_t n, int knn, float max_density, int64_t seed, float* out_xyz1,
                             float* out_normals, float* out_densities, int64_t* n_out, int64_t* n_dense);
/* The module's slots of a loaded chain: 1 and *max_density (nullable) if the document names MaxDensityDataPointsFilter, else 0
 * and *max_density untouched.  Host only. */
int lsgpu_loaded_chain_max_density(const lsgpu_loaded_chain* c, float* max_density);

/* ---- ShadowDataPointsFilter behind the module that produces the normals, either section (DESIGN.md §3
 * "ShadowDataPointsFilter", §5 choices 41-44) -----------------------------------------------------------------------------
 * Drops the points whose normal is nearly perpendicular to the ray that observed them: grazing returns and the mixed pixels at
 * depth edges.  Restated from knowledge of upstream's ShadowDataPointsFilter::inPlaceFilter, parity unpinned.
 *   Per point p (as given to the section -- not centred, the 4th component not read) with normal n, in float, one rounding per
 *     operation, no fma, sums of three terms left to right:  ln = sqrtf((nx nx + ny ny) + nz nz), lp = sqrtf((px px + py py) + pz pz),
 *     u = n / ln, v = p / lp (three divisions each), value = fabsf((ux vx + uy vy) + uz vz); kept iff value > eps
 *     (csrc/lsgpu_shadow.h, shared by host and device).  A zero normal, a point at the origin or a NaN anywhere: value 0 or NaN,
 *     dropped.  eps: default 0.1, finite, in [0, 3.1416].  Order of the survivors preserved, no draw consumed.
 *   In lsgpu_icp_compute / _compute_clouds / _compute_clouds_upload (a handle with lsgpu_icp_set_shadow):
 *     reference, chain->ssn_knn > 0: the pass runs on the sampling filter's points and normals;
 *     reference, chain->sn_knn > 0: the grid of the whole (cut) reference, the normals on it, the pass -- the kept cloud and its
 *       normals then go on as the sampling filter's output does (orientation, centring on the KEPT cloud's mean, grid, loop); a
 *       point-to-point handle computes the normals for the module too;
 *     reference, with lsgpu_icp_set_max_density: the pass runs on the thinning's output, the thinning's draws are untouched;
 *     reference, neither ssn_knn nor sn_knn: LSGPU_BAD_CONFIG (no normals);
 *     reading: behind its SurfaceNormalDataPointsFilter (lsgpu_normals_config.reading_sn_knn) and its orientation; the
 *       loop and SurfaceNormalOutlierFilter see the kept points and their normals.
 *     A section left with no point: LSGPU_NO_CONVERGENCE ("compute: the reference / reading filter left no point").  A handle
 *     without the module enqueues what it always did.
 *   Not together with the split-scan mode (lsgpu_icp_comm_init) or PointToPlaneWithCovErrorMinimizer (lsgpu_icp_set_covariance: its
 *     first version does not cover a reference thinned behind the normals): LSGPU_BAD_CONFIG, the module named in
 *     lsgpu_last_error, whichever of the two calls comes second.  reading_eps >= 0 on a handle whose lsgpu_normals_config has no
 *     reading_sn_knn, and lsgpu_icp_set_normals taking the reading's normals away while reading_eps >= 0: refused likewise.
 *   Loader: ShadowDataPointsFilter {eps}, once per section, anywhere behind the section's normals module (and behind
 *     MaxDensityDataPointsFilter where there is one) but not between ObservationDirection- and OrientNormalsDataPointsFilter.
 *     On the reading only with SurfaceNormalOutlierFilter in the chain (reading normals that no outlier filter reads stay
 *     refused).  lsgpu_loaded_chain has no free slot left, so the module travels by its own entry, lsgpu_chain_load_shadow: a
 *     front end that loads a document MUST call it beside lsgpu_chain_load and give the result to lsgpu_icp_set_shadow (both
 *     facades of this repository and the shim do), or a chain with the module runs without it. */
typedef struct lsgpu_shadow_config {
  float reading_eps, reference_eps;   /* eps of the section's module; < 0: no module on that side */
  int   reserved[2];                  /* 0 */
} lsgpu_shadow_config;
void lsgpu_shadow_config_default(lsgpu_shadow_config* c);   /* both -1: no module */
/* Without a handle or a device: LSGPU_OK / NULL, or LSGPU_BAD_CONFIG / the reason (a static string, the module's name in it) for
 * an eps that is NaN, infinite or above 3.1416, or a reserved field that is not 0. */
int lsgpu_shadow_config_check(const lsgpu_shadow_config* c);
const char* lsgpu_shadow_config_why(const lsgpu_shadow_config* c);
/* Gives the handle the module (cfg is copied); NULL, or both eps < 0, removes it.  A bad eps and the refused combinations above:
 * LSGPU_BAD_CONFIG before the device is touched (the handle keeps what it had). */
int lsgpu_icp_set_shadow(lsgpu_icp* h, const lsgpu_shadow_config* cfg);
/* The pass on a cloud with its normals (kernel-level entry): xyz1 4 floats / point, normals 3 floats / point, host or device
 * pointers; out_xyz1 / out_normals need room for n points and must not be the inputs.  *n_out points kept.  The handle's own
 * module is not read.  LSGPU_NO_CONVERGENCE if nothing is kept ("... the filter left no point"). */
int lsgpu_icp_filter_shadow(lsgpu_icp* h, const float* xyz1, const float* normals, int64_t n, float eps, float* out_xyz1,
                            float* out_normals, int64_t* n_out);
/* Host twin (no GPU, no handle), bit-identical with the device pass; host pointers. */
int lsgpu_filter_shadow(const float* xyz1, const float* normals, int64_t n, float eps, float* out_xyz1, float* out_normals,
                        int64_t* n_out);
/* The ShadowDataPointsFilter modules of a YAML document: the walk, the rules, the refusals and the texts of lsgpu_chain_load,
 * the two eps in *out (every byte; -1 for a section without the module).  Host only. */
int lsgpu_chain_load_shadow(const lsgpu_yaml_module* mods, int n_mods, lsgpu_shadow_config* out, char* why, int why_cap);

/* ---- PointToPlaneErrorMinimizer force4DOF / force2D and BoundTransformationChecker (DESIGN.md §3 "Constrained steps and the
 * bound checker") ------------------------------------------------------------------------------------------------------------
 * What a ground vehicle's ICP file adds to icp_.compute (laser_slam/src/laser_track.cpp:496-499 catches the ConvergenceError
 * the checker throws and falls back to the odometry).  Restated from knowledge of upstream's
 * PointToPlaneErrorMinimizer::compute_in_place and BoundTransformationChecker::check, parity unpinned.
 *   The constrained steps (dof): per kept pair, in the loop's reference-mean frame, f = [p x n; n] and e = n . (p - q) as in the
 *     6-DOF step; the 6x6 sums A = sum w f f^T, b = -sum w f e are formed as always.
 *     LSGPU_MOTION_DOF_4 (force4DOF; unknowns yaw, tx, ty, tz): rows and columns {2, 3, 4, 5} of A and b are solved.
 *     LSGPU_MOTION_DOF_3 (force2D; unknowns yaw, tx, ty): rows and columns {2, 3, 4}; b is formed with the planar residual
 *       e2 = n.x (p.x - q.x) + n.y (p.y - q.y) (the z row of both clouds and of the normals dropped, the normals not
 *       renormalised).  A and slot 28 (sum e^2) keep the three-dimensional terms; matching, distances, the trim limit and every
 *       outlier filter stay three-dimensional.
 *     Solve: the float LLT of the 6-DOF step on the sub-system; a failed pivot is LSGPU_NO_CONVERGENCE ("normal matrix not
 *       positive definite").  dT: the rotation by yaw about the z axis through the reference mean -- sine and cosine of |yaw|
 *       evaluated in double and rounded, third row and column exactly 0, 0, 1 -- and the translation (tz = 0 under force2D);
 *       T_iter <- dT T_iter.  Checkers, trace layout and caps unchanged: lsgpu_iter_trace.A / .b hold the full sums (b with e2
 *       under force2D), .x = {0, 0, yaw, tx, ty, tz} with the fixed unknowns exactly 0.  lsgpu_normal_eq on such a handle
 *       returns the sums of its mode.
 *     First version: KDTreeMatcher knn 1 (with or without maxDist) and any of Trimmed-, Max-, Min-, MedianDistOutlierFilter.
 *       Not together with knn >= 2, RobustOutlierFilter, SurfaceNormalOutlierFilter, PointToPlaneWithCovErrorMinimizer,
 *       PointToPointErrorMinimizer or the split-scan mode: LSGPU_BAD_CONFIG before the device is touched, the module named in
 *       lsgpu_last_error, whichever call comes second.
 *   BoundTransformationChecker (bound 1; max_rotation_norm, max_translation_norm finite and >= 0): the checker is initialised
 *     with the loop's first T_iter; an iteration whose T_iter has angularDistance(q_iter, q_0) > max_rotation_norm or
 *     |t_iter - t_0| > max_translation_norm is a ConvergenceError.  The bound is evaluated on the host AFTER the loop, from the
 *     history the loop's checkers keep (one quaternion and translation per iteration, copied with the loop state): the first
 *     entry out of bounds makes the call return LSGPU_NO_CONVERGENCE with T_out = T_init and lsgpu_last_error
 *     "BoundTransformationChecker: limit out of bounds: rot <value>/<limit> tr <value>/<limit>".  A loop that failed by itself
 *     in a later iteration: the bound's message wins; in an earlier one: the loop's stands.  When
 *     CounterTransformationChecker ends the loop its last T_iter is in no history; bound_before_counter 1 (the document lists
 *     the bound in front of the counter) checks it too, 0 does not (upstream's MaxNumIterationsReached leaves the checker
 *     loop).  Works with either minimizer; not in the split-scan mode.  A handle without it enqueues and copies what it did. */
#define LSGPU_MOTION_DOF_6 0   /* the free step */
#define LSGPU_MOTION_DOF_3 3   /* force2D  */
#define LSGPU_MOTION_DOF_4 4   /* force4DOF */
typedef struct lsgpu_motion_config {
  int   dof;                    /* LSGPU_MOTION_DOF_* */
  int   bound;                  /* 1: BoundTransformationChecker */
  float max_rotation_norm, max_translation_norm;   /* rad, m; read if bound */
  int   bound_before_counter;   /* 1: listed in front of CounterTransformationChecker */
  int   reserved[3];            /* 0 */
} lsgpu_motion_config;
void lsgpu_motion_config_default(lsgpu_motion_config* c);   /* dof 0, no bound, both limits 1 (the module's defaults), behind the counter */
/* Without a handle or a device: LSGPU_OK / NULL, or LSGPU_BAD_CONFIG / the reason (a static string, the module's name in it). */
int lsgpu_motion_config_check(const lsgpu_motion_config* c);
const char* lsgpu_motion_config_why(const lsgpu_motion_config* c);
/* Gives the handle the two modules (cfg is copied); NULL, or dof 0 without bound, removes them.  Bad values and the refused
 * combinations above: LSGPU_BAD_CONFIG before the device is touched (the handle keeps what it had). */
int lsgpu_icp_set_motion(lsgpu_icp* h, const lsgpu_motion_config* cfg);
/* The step of a handle's mode from the 27 sums of lsgpu_normal_eq: dof LSGPU_MOTION_DOF_6 is lsgpu_point_to_plane_solve, _4 and
 * _3 the constrained steps above (dof 3 expects b formed with e2, as a force2D handle's lsgpu_normal_eq returns it).  Host only,
 * bit for bit what the device lane computes.  LSGPU_NO_CONVERGENCE (dT the identity) if the system solved is not positive
 * definite; any other dof: LSGPU_BAD_ARG. */
int lsgpu_point_to_plane_solve_dof(const double sums[27], int dof, float dT[16]);
/* T_iters: n column-major 4x4 transforms, entry 0 the one the checker was initialised with.  The first index >= 1 whose
 * rotation (angularDistance of the Eigen quaternions) or translation differs from entry 0 by MORE than its limit, -1 if there
 * is none (or n < 2, or a NULL T_iters).  Host only; the arithmetic the library applies to the loop's history. */
int lsgpu_bound_first_violation(const float* T_iters, int n, float max_rot, float max_trans);
/* The force2D / force4DOF parameters and the BoundTransformationChecker of a YAML document: the walk, the rules, the refusals and
 * the texts of lsgpu_chain_load, the result in *out (every byte; lsgpu_motion_config_default for a document with neither).  Host
 * only.  As with lsgpu_chain_load_shadow, a front end that loads a document MUST call it beside lsgpu_chain_load and give the
 * result to lsgpu_icp_set_motion. */
int lsgpu_chain_load_motion(const lsgpu_yaml_module* mods, int n_mods, lsgpu_motion_config* out, char* why, int why_cap);

/* ---- CovarianceSamplingDataPointsFilter: geometrically stable sampling of a cloud with normals (DESIGN.md §3
 * "CovarianceSamplingDataPointsFilter", §5 choices 55-62) ---------------------------------------------------------------------
 * Gelfand's sampling: of the point-to-plane constraints [(p - c) x n ; n] of a cloud it keeps the nbSample points that constrain
 * the six eigen-directions of their 6x6 covariance equally -- in a corridor the few points that stop the scan sliding along
 * it, where RandomSampling keeps what is plentiful.  Restated from knowledge of upstream's
 * CovarianceSamplingDataPointsFilter::inPlaceFilter, parity unpinned.
 *   Parameters: nbSample (default 5000, an integer in [1, 2^31 - 16]); torqueNorm (default 1; 0: L = 1, 1: L = Lavg, 2: L = Lmax).
 *     Anything else: LSGPU_BAD_CONFIG, the module and the parameter named.
 *   Input: n points xyz1 with normals (3 floats each), as given -- not centred, the 4th component carried and not read.
 *   nbSample >= n: the cloud passes unchanged (ids 0 .. n - 1), nothing is computed (sums_out: zeros, n in its last slot).
 *   Otherwise, in float, one rounding per operation, no fma, sums left to right, unless marked double:
 *   1. S_a = sum p_a in double, c_a = (float)(S_a / (double)n); min_a, max_a per axis; d = p - c.
 *   2. Lnorm.  torqueNorm 0: 1.  1: (float)(sum (double)sqrtf((dx dx + dy dy) + dz dz) / (double)n).  2: e * 0.5f with e the
 *      largest of the three float differences max_a - min_a.  An Lnorm that is 0 or not finite: LSGPU_BAD_ARG (upstream
 *      divides by it).
 *   3. invL = 1.f / Lnorm; m = d x n, each component two products and one subtraction (mx = dy nz - dz ny, my = dz nx - dx nz,
 *      mz = dx ny - dy nx); v = (invL mx, invL my, invL mz, nx, ny, nz).
 *   4. C_ab = sum (double)v_a (double)v_b for a <= b: 21 sums, the products exact in double.  A sum of step 1, 2 or 4 that is
 *      not finite -- a NaN or an infinite point or normal -- is LSGPU_BAD_ARG, the outputs untouched.
 *   5. Eigenvectors: cyclic Jacobi on the symmetric C in double (lsgpu_cov_sampling_eigen; one host function, which the
 *      device path and the host twin both call).  A = C, V = I.  A sweep starts with off = the sum, row major, of a_pq^2 over
 *      p < q: off == 0 ends the iteration, as do 30 sweeps.  The sweep visits (p, q), p < q, row major, and skips a pair with
 *      a_pq == 0; else theta = (a_qq - a_pp) / (2 a_pq), t = s / (|theta| + sqrt(theta theta + 1)) with s = -1 if theta < 0
 *      and +1 otherwise, cs = 1 / sqrt(t t + 1), sn = t cs; then for every row k (a_kp, a_kq) <- (cs a_kp - sn a_kq,
 *      sn a_kp + cs a_kq), then for every column k (a_pk, a_qk) <- (cs a_pk - sn a_qk, sn a_pk + cs a_qk), then a_pq = a_qp = 0,
 *      then for every row k (v_kp, v_kq) <- (cs v_kp - sn v_kq, sn v_kp + cs v_kq).  Eigenpairs (a_jj, column j of V) in
 *      ascending order of the eigenvalue, ties by the original column; X_k = the k-th vector rounded to float.  Signs do not
 *      matter below.  (Upstream's general EigenSolver leaves the order unspecified; ascending -- the least constrained
 *      direction served first -- is this library's choice.)
 *   6. s_k = ((((v0 X0k + v1 X1k) + v2 X2k) + v3 X3k) + v4 X4k) + v5 X5k, mag_k(i) = fabsf(s_k).
 *   7. List k: the point indices by decreasing mag_k, ties by ascending index (upstream's std::list::sort is stable).  The
 *      order is that of the magnitudes' bit patterns as unsigned integers, which for the non-negative floats is their order.
 *   8. Walk: t[0..5] = 0 in float; nbSample times: k = 0, for i = 0..5: if (t[k] > t[i]) k = i (the first index of the
 *      minimum); pop list k from the front while its head is already chosen; the head is chosen and popped;
 *      t[j] += mag_j(id) * mag_j(id) for j = 0..5.
 *   9. Output: the chosen points and normals, all four and three components, in the order they were chosen (what upstream's
 *      swap-and-lookup bookkeeping intends).  No draw is consumed.
 *   Heads of nbSample entries suffice: every entry popped from list k is a chosen point and chosen points are distinct, so at
 *   most nbSample entries of a list are ever popped and the last head is read at position nbSample - 1 at most.  The device
 *   path therefore sends the first nbSample entries of each sorted list -- index and the six magnitudes, 28 bytes -- to the
 *   host in one download; the walk runs there, the picks go back, one kernel gathers.  Device path: three passes of double
 *   sums without atomics (reproducible run to run), six full stable radix sorts of n pairs (a top-nbSample selection in front of a
 *   small sort is the follow-up).
 *   sums[32], in order: S (3), min (3), max (3), sum of lengths (1; 0 unless torqueNorm 1), C upper triangle row major (21), n.
 *   In lsgpu_icp_compute / _compute_clouds / _compute_clouds_upload (a handle with lsgpu_icp_set_cov_sampling) the module is
 *   the section's last thinning step behind the normals:
 *     reference, chain->ssn_knn > 0: on the sampling filter's points and normals;
 *     reference, chain->sn_knn > 0: the grid of the whole (cut) reference, the normals on it, copied out in the cloud's order, the
 *       module -- by the route ShadowDataPointsFilter takes; a point-to-point handle computes the normals for the module too;
 *     reference, behind MaxDensityDataPointsFilter and ShadowDataPointsFilter where the handle has them: on their output;
 *     the kept cloud and its normals go on as the sampling filter's output does (orientation, centring on the KEPT cloud's
 *       mean, grid, loop);
 *     reference, neither ssn_knn nor sn_knn: LSGPU_BAD_CONFIG (no normals);
 *     reading: behind its SurfaceNormalDataPointsFilter (lsgpu_normals_config.reading_sn_knn), its orientation and its Shadow
 *       pass; the loop and SurfaceNormalOutlierFilter see the kept points and their normals.
 *     A section with no more than nbSample points passes unchanged (behind SurfaceNormalDataPointsFilter alone the handle then
 *     does what one without the module does).  A degenerate section (Lnorm 0, a value that is not finite) or one of more than
 *     (2^31 - 16) / 6 points: LSGPU_BAD_ARG, the handle holds no reference and stays usable.  No draw is consumed, the draw stream of a compute is untouched; the side stream
 *     stays on (the module runs on the main stream, in front of the reading's side).  A handle without the module enqueues
 *     what it always did.
 *   Not together with the split-scan mode (lsgpu_icp_comm_init) or PointToPlaneWithCovErrorMinimizer (lsgpu_icp_set_covariance):
 *     LSGPU_BAD_CONFIG, the module named in lsgpu_last_error, whichever of the two calls comes second.  reading_nb_sample > 0 on
 *     a handle whose lsgpu_normals_config has no reading_sn_knn, and lsgpu_icp_set_normals taking the reading's normals away
 *     while reading_nb_sample > 0: refused likewise.
 *   Loader: CovarianceSamplingDataPointsFilter {nbSample, torqueNorm}, once per section, behind the section's normals module
 *     and behind its MaxDensity- and ShadowDataPointsFilter (either of them behind the module is refused), not between
 *     ObservationDirection- and OrientNormalsDataPointsFilter (the pair may follow: the module does not read the normals'
 *     signs).  On the reading only with SurfaceNormalOutlierFilter in the chain.  Not with PointToPlaneWithCovErrorMinimizer.
 *     The module travels by its own entry, lsgpu_chain_load_cov_sampling: a front end that loads a document MUST call it beside
 *     lsgpu_chain_load and give the result to lsgpu_icp_set_cov_sampling (both facades of this repository and the shim do), or
 *     a chain with the module runs without it.  In the input filter chain (lsgpu_apply_point_filters) the name stays unknown. */
typedef struct lsgpu_cov_sampling_config {
  int reading_nb_sample, reference_nb_sample;       /* nbSample of the section's module; 0: no module on that side */
  int reading_torque_norm, reference_torque_norm;   /* torqueNorm: 0, 1 or 2 */
  int reserved[4];                                  /* 0 */
} lsgpu_cov_sampling_config;
void lsgpu_cov_sampling_config_default(lsgpu_cov_sampling_config* c);   /* no module on either side, torqueNorm 1 */
/* Without a handle or a device: LSGPU_OK / NULL, or LSGPU_BAD_CONFIG / the reason (a static string, the module's and the
 * parameter's name in it). */
int lsgpu_cov_sampling_config_check(const lsgpu_cov_sampling_config* c);
const char* lsgpu_cov_sampling_config_why(const lsgpu_cov_sampling_config* c);
/* Gives the handle the module (cfg is copied); NULL, or both nb_sample 0, removes it.  Bad values and the refused combinations
 * above: LSGPU_BAD_CONFIG before the device is touched (the handle keeps what it had). */
int lsgpu_icp_set_cov_sampling(lsgpu_icp* h, const lsgpu_cov_sampling_config* cfg);
/* The CovarianceSamplingDataPointsFilter modules of a YAML document: the walk, the rules, the refusals and the texts of
 * lsgpu_chain_load, the parameters in *out (every byte; lsgpu_cov_sampling_config_default for a document without the module).
 * Host only. */
int lsgpu_chain_load_cov_sampling(const lsgpu_yaml_module* mods, int n_mods, lsgpu_cov_sampling_config* out, char* why, int why_cap);
/* The module on a cloud with its normals (kernel-level entry): xyz1 4 floats / point, normals 3 floats / point, host or device
 * pointers; out_xyz1 / out_normals / out_ids (nullable) need room for min(nb_sample, n) points and must not be the inputs.
 * n <= (2^31 - 16) / 6.  *n_out = min(nb_sample, n); sums_out (nullable, host): the sums the device formed.
 * LSGPU_NO_CONVERGENCE for n == 0. */
int lsgpu_icp_filter_cov_sampling(lsgpu_icp* h, const float* xyz1, const float* normals, int64_t n, int nb_sample, int torque_norm,
                                  float* out_xyz1, float* out_normals, int32_t* out_ids, int64_t* n_out, double sums_out[32]);
/* Wall time in ms of the phases of the handle's last lsgpu_icp_filter_cov_sampling that got past the early exit: sums (three
 * waits and the Jacobi), projections + sorts + heads download, the host walk, picks upload + gather (enqueue). */
int lsgpu_icp_cov_sampling_phase_ms(lsgpu_icp* h, double ms[4]);
/* Host twin (no GPU, no handle); host pointers.  sums_in == NULL: the sums are added sequentially in double, in index order.
 * sums_in given (32 doubles in sums_out's layout): those are used and no sum is formed -- a tree-shaped device sum and a
 * sequential one differ in the last bits of a double; fed the device's sums_out the twin is bit-identical with the device
 * path in everything behind the sums. */
int lsgpu_filter_cov_sampling(const float* xyz1, const float* normals, int64_t n, int nb_sample, int torque_norm, const double* sums_in,
                              float* out_xyz1, float* out_normals, int32_t* out_ids, int64_t* n_out, double sums_out[32]);
/* Step 5 on the upper triangle C21 (row major) of a symmetric 6x6 matrix: X[6 a + k] = component a of the k-th eigenvector as
 * float, values (nullable) the eigenvalues, ascending.  Host only.  LSGPU_BAD_ARG for a NULL or an entry that is not finite. */
int lsgpu_cov_sampling_eigen(const double C21[21], float X[36], double values[6]);

/* ---- carried normals: a cloud brings its normals along (DESIGN.md §3 "Carried normals", §5 choices) --------------------------
 * LaserTrack applies its input filters once to every scan, stores the result, rebuilds the sub-map with
 * RigidTransformation::compute + concatenate and hands both clouds to ICP::compute.  With SurfaceNormalDataPointsFilter in the
 * input filters the normals are computed once per scan and travel as a descriptor; the ICP chain then needs no normals
 * module.  The rules:
 *  1. A cloud may carry normals, 3 floats per point beside the points.  A sub-map concat_i(T_i cloud_i) carries normals iff
 *     EVERY member does (concatenate keeps what both sides have).  Points move with the arithmetic of lsgpu_transform_points,
 *     normals with that of lsgpu_rotate_descriptors; a member whose transform is exactly the identity is copied bit for bit
 *     (Inf and NaN survive).
 *  2. A normals module in a section overwrites what the section's cloud carries: with ssn_knn / sn_knn > 0 (reference) or
 *     reading_sn_knn > 0 (reading) the carried normals of that side are never read, and every result is bit-identical to the
 *     call on clouds without normals.
 *  3. Carried normals nobody reads do not travel (no upload, no compaction, no sort).  The reference's are read iff the
 *     minimizer is not point-to-point, or RobustOutlierFilter takes the point-to-plane distance, or SurfaceNormalOutlierFilter
 *     is set; the reading's iff SurfaceNormalOutlierFilter is set (max_angle >= 0).
 *  4. RandomSamplingDataPointsFilter and the cut modules (lsgpu_icp_set_chain_cuts) keep a point's normal with the point.
 *     Order, predicates, draws and the number of draws consumed are those of the section on a cloud without normals;
 *     RemoveNaN looks at the four feature rows only.
 *  5. Readers.  Reference: the point-to-plane minimizers, RobustOutlierFilter point2plane, SurfaceNormalOutlierFilter and the
 *     reference's ObservationDirection + OrientNormals pair (reference_orient).  Reading: SurfaceNormalOutlierFilter.  Behind
 *     the sections the loop sees what lsgpu_icp_set_reference(ref, ref_normals) + lsgpu_icp_align_normals(reading,
 *     reading_normals) on the sections' outputs see.
 *  6. A reference without normals that somebody reads, in a chain without a reference module, is LSGPU_BAD_CONFIG as ever;
 *     where some slots of a sub-map carry normals and one does not, the error names that slot.  SurfaceNormalOutlierFilter
 *     with reading_normals_given 1 and a reading that carries none is inert (upstream skips it with a warning).
 * Refused in this version: MaxDensity-, Shadow- and CovarianceSamplingDataPointsFilter on carried normals (they need the
 * section's own normals module: the texts of lsgpu_icp_compute apply), the reading's orientation pair on carried normals
 * (lsgpu_normals_config_check's text), and carried normals on a split-scan handle (lsgpu_icp_set_reference takes them there).
 *
 * lsgpu_cloud_upload_normals: lsgpu_cloud_upload plus the cloud's normals (host or device); normals NULL is lsgpu_cloud_upload,
 * which drops what the slot carried.  lsgpu_cloud_release frees both. */
int lsgpu_cloud_upload_normals(lsgpu_icp* h, int slot, const float* xyz1, const float* normals, int64_t n);
int lsgpu_cloud_has_normals(lsgpu_icp* h, int slot, int* has);   /* 1: the slot holds a cloud that carries normals */
/* lsgpu_icp_compute on clouds that carry normals; host or device pointers, either normals pointer may be NULL.  Both NULL:
 * lsgpu_icp_compute, bit for bit.  The caller's normals are only read. */
int lsgpu_icp_compute_normals(lsgpu_icp* h, const float* reading_xyz1, const float* reading_normals, int64_t nq,
                              const float* reference_xyz1, const float* reference_normals, int64_t nr, const float T_init[16],
                              const lsgpu_chain_config* chain, float T_out[16], lsgpu_icp_stats* stats);
/* lsgpu_icp_compute_clouds and lsgpu_icp_compute_clouds_upload use what the slots carry (rule 1); the latter stores points only,
 * so its reading slot carries none afterwards.  This entry stores the reading with its normals and computes.  In this version
 * the upload and the compute run one after the other: no overlap of the copy with the sub-map's assembly. */
int lsgpu_icp_compute_clouds_upload_normals(lsgpu_icp* h, int reading_slot, const float* reading_xyz1, const float* reading_normals,
                                            int64_t nq, const int* ref_slots, const float* ref_T, int n_ref, const float T_init[16],
                                            const lsgpu_chain_config* chain, float T_out[16], lsgpu_icp_stats* stats);
/* lsgpu_chain_load for a caller whose clouds carry normals: `carried` is a set of the two bits below.  The same walk, rules
 * and texts; a carried reference counts as normals for whoever reads the reference's (no reference module needed, and its
 * ObservationDirection + OrientNormals pair may stand without one), and with a carried reading, SurfaceNormalOutlierFilter
 * and no SurfaceNormalDataPointsFilter in the reading's section out->normals.reading_normals_given is 1.  carried 0 is
 * lsgpu_chain_load in every byte and text.  lsgpu_chain_load_parts_carried: the other four loaders under the same
 * declaration, each output nullable. */
#define LSGPU_CARRIED_READING 1
#define LSGPU_CARRIED_REFERENCE 2
int lsgpu_chain_load_carried(const lsgpu_yaml_module* mods, int n_mods, unsigned carried, lsgpu_loaded_chain* out, char* why, int why_cap);
int lsgpu_chain_load_parts_carried(const lsgpu_yaml_module* mods, int n_mods, unsigned carried, lsgpu_chain_cuts* cuts,
                                   lsgpu_shadow_config* shadow, lsgpu_motion_config* motion, lsgpu_cov_sampling_config* cov_sampling,
                                   char* why, int why_cap);
/* A document's whole module set, and the two calls a front end needs: load it, apply it.
 * lsgpu_chain_load_modules: the one walk of lsgpu_chain_load_carried and lsgpu_chain_load_parts_carried, every part into one
 * record (byte for byte what those return; the same verdict and text; `carried` is kept in the record).
 * lsgpu_icp_set_modules: the record's eight modules onto a handle in one call -- RobustOutlierFilter (chain.has_robust), the
 * normals config (chain.has_normals), the covariance and MaxDensity (lsgpu_loaded_chain_covariance / _max_density), the cut
 * modules, Shadow, CovarianceSampling and the motion config -- each through the code of its lsgpu_icp_set_* setter, in that
 * order, a module the record does not hold being switched off.  All or nothing: where a step refuses, the call returns its
 * code with its text in lsgpu_last_error and the handle is as it was.  A record not made by the loader starts from the
 * *_config_default values.  Which modules run together is one rule set for all these entries (csrc/lsgpu_modules.h). */
typedef struct lsgpu_chain_modules {
  lsgpu_loaded_chain chain;
  lsgpu_chain_cuts cuts;
  lsgpu_shadow_config shadow;
  lsgpu_motion_config motion;
  lsgpu_cov_sampling_config cov_sampling;
  unsigned carried;   /* LSGPU_CARRIED_*: what the document was loaded under */
  int reserved[3];    /* 0 */
} lsgpu_chain_modules;
int lsgpu_chain_load_modules(const lsgpu_yaml_module* mods, int n_mods, unsigned carried, lsgpu_chain_modules* out, char* why, int why_cap);
int lsgpu_icp_set_modules(lsgpu_icp* h, const lsgpu_chain_modules* set);
/* SurfaceNormalDataPointsFilter's parameters as the loader judges the reading's module (knn 3..32, keepNormals 1, epsilon 0,
 * no maxDist, nothing else kept): LSGPU_OK and *knn, or LSGPU_BAD_CONFIG and the loader's text.  For a chain outside the ICP
 * file that runs the module (the input filters).  Host only. */
int lsgpu_surface_normal_params_check(const lsgpu_yaml_param* params, int n_params, int* knn, char* why, int why_cap);

/* ---- Ingest: a raw scan through the input filters, with its normals, into a cloud slot -- one call, on this handle
 * lsgpu_cloud_ingest on a cloud in host or device memory does what these three calls do, bit for bit:
 *   lsgpu_apply_point_filters(h, filters, n_filters, xyz1, n, seed, kept, &m);
 *   if (normals_knn > 0) lsgpu_icp_reading_normals(h, kept, m, normals_knn, orient, sensor, normals);
 *   lsgpu_cloud_upload_normals(h, slot, kept, normals_knn > 0 ? normals : NULL, m);
 * with one upload of the raw scan and no second handle: the point modules, the grid, the normals search and one store kernel
 * run on this handle's stream and buffers (which grow on demand; nothing is freed per call).  The same are: the slot's points
 * (4th component included) and normals, the number and order of the draws consumed, seed's meaning, filters[k].state of
 * FixStepSampling.  normals_knn 0 ingests without normals: no grid is built and the slot carries none afterwards.
 * out_xyz1 (room for n points) and out_normals (3 n floats), each nullable, host or device, receive the kept cloud: one copy
 * each on the handle's stream, one synchronise at the end.  *n_out (nullable): the kept count (on a failure of the normals'
 * step what the point modules had kept, else 0 on failure).
 *  - Argument and configuration errors return before the device or the slot is touched: the slot stays as it was, no draw is
 *    consumed, seed is not taken.  These are what lsgpu_apply_point_filters refuses (LSGPU_BAD_ARG, LSGPU_BAD_CONFIG with its
 *    texts), and LSGPU_BAD_ARG with a text for normals_knn not 0 and outside 3..32, orient outside 0..2, orient set without
 *    sensor or with normals_knn 0, out_normals given with normals_knn 0.
 *  - Once device work has begun any failure leaves the slot EMPTY (lsgpu_cloud_size: -1) and carries the composition's code
 *    and text: LSGPU_NO_CONVERGENCE "no points to filter", LSGPU_BAD_ARG for fewer kept points than knn or for a NaN reaching
 *    VoxelGrid, OctreeGrid or the normals' grid, a HIP error.
 *  - A chain whose last module keeps nothing, with normals_knn 0, succeeds with an empty cloud (size 0), as the composition.
 *  - With normals_knn > 0 the handle's reference is replaced, as by lsgpu_icp_filter_reference_normals (the search runs on
 *    the handle's own grid).  lsgpu_icp_compute* rebuild the reference anyway; a caller of lsgpu_icp_align must call
 *    lsgpu_icp_set_reference again.  With normals_knn 0 the reference is untouched.
 *  - After lsgpu_icp_comm_init (split-scan handle) normals_knn > 0 is LSGPU_BAD_CONFIG by name, as carried normals are.
 * lsgpu_cloud_download: a slot's points to out_xyz1 (room for cap_points), and its normals where out_normals is given; host
 * or device.  LSGPU_BAD_ARG with a text for an empty slot, cap_points smaller than the cloud, out_normals on a slot that
 * carries none. */
int lsgpu_cloud_ingest(lsgpu_icp* h, int slot, lsgpu_point_filter* filters, int n_filters, const float* xyz1, int64_t n,
                       int64_t seed, int normals_knn, int orient, const float sensor[3], float* out_xyz1, float* out_normals,
                       int64_t* n_out);
int lsgpu_cloud_download(lsgpu_icp* h, int slot, float* out_xyz1, float* out_normals, int64_t cap_points);

const char* lsgpu_strerror(int code);
const char* lsgpu_last_error(lsgpu_icp* h); /* detail of the last failure on this handle */
int         lsgpu_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
