/*
 * srrg2_slam_amd.h -- C ABI of the MI355X-native multi-cue aligner hot path.
 *
 * This header is the drop-in boundary of the build.  The reference has no C ABI:
 * its boundary is a set of C++ classes found by name in the BOSS registry
 * (S/instances.cpp:21-23,28-84) and configured through PARAM()s.  Every entry
 * point below cites the reference interface it replaces, using the path
 * abbreviations of SURVEY.md:
 *   S/ = srrg2_slam_interfaces/src/srrg2_slam_interfaces/
 *   T/ = srrg2_slam_interfaces/tests/
 *
 * Conventions
 *  - every function returns an int: 0 on success, <0 on error (replaces the
 *    reference's `throw std::runtime_error`, e.g. S/registration/aligners/
 *    multi_aligner_impl.cpp:30,40,49).  srrg2_amd_last_error() returns the text.
 *  - handles are opaque; one handle = one non-thread-safe object (the reference
 *    objects are single threaded, SURVEY.md section 8b "Threading").
 *  - transforms: SE(3) = row-major 3x4 float [R|t] (12 floats);
 *                SE(2) = row-major 3x3 homogeneous float (9 floats).
 *    `moving_in_fixed` maps moving-frame points into the fixed frame
 *    (S/registration/aligners/aligner.h:103-109).
 *  - clouds are borrowed for the duration of the call only: set_fixed/set_moving/
 *    compute_batch ingest (copy + reorder) the data into HBM and return when they
 *    have finished reading, so the caller may free or reuse its buffer on return.
 *    `mem` says where the caller's pointer lives.  SRRG2_MEM_DEVICE buffers are read
 *    on the handle's own (non-blocking) stream, which is NOT ordered after the
 *    stream that produced them: the producer must have completed (stream/event/
 *    device synchronised) before the call.  SRRG2_MEM_DEVICE_KEPT (set_fixed / set_moving):
 *    a device buffer that the caller leaves valid and unchanged until the next compute()
 *    on the handle has returned -- the reference's own contract (its aligner keeps raw
 *    pointers to the caller's clouds: aligner.h:130-131) -- so the call returns as soon as
 *    the ingest is queued; a tracker's frame (scene arrays in HBM: srrg2_scene_device_arrays)
 *    saves two host waits that way.
 *  - all arithmetic is float32 / int32 at the interface.
 */
#ifndef SRRG2_SLAM_AMD_H
#define SRRG2_SLAM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRRG2_AMD_ABI_VERSION 4
#define SRRG2_MAX_SLICES 8

/* ---- enums -------------------------------------------------------------- */

/* variable flavours of S/registration/aligners/multi_aligner.h:152-158 */
enum srrg2_variable_kind {
  SRRG2_SE2_RIGHT       = 0, /* MultiAligner2D   = MultiAlignerBase_<VariableSE2RightAD>           */
  SRRG2_SE3_EULER_RIGHT = 1, /* MultiAligner3D   = MultiAlignerBase_<VariableSE3EulerRightAD>      */
  SRRG2_SE3_QUAT_RIGHT  = 2  /* MultiAligner3DQR = MultiAlignerBase_<VariableSE3QuaternionRightAD> */
};

/* AlignerBase::Status, S/registration/aligners/aligner.h:23-28 (values identical) */
enum srrg2_status {
  SRRG2_SUCCESS                    = 0,
  SRRG2_NOT_ENOUGH_CORRESPONDENCES = 1,
  SRRG2_NOT_ENOUGH_INLIERS         = 2,
  SRRG2_FAIL                       = 3
};

/* which factor a slice linearises (FactorCorrespondenceDriven_ subclasses used through
 * S/registration/aligners/aligner_slice_processor.h:7,29,44; prior factors through
 * S/registration/aligners/aligner_slice_odometry_prior.h:9,33) */
enum srrg2_slice_kind {
  SRRG2_SLICE_P2P          = 0, /* point-to-point   (SE2: 2x3 J, SE3: 3x6 J)            */
  SRRG2_SLICE_P2PLANE      = 1, /* point-to-plane   (1x3 / 1x6 J), needs fixed normals  */
  SRRG2_SLICE_REPROJECTION = 2, /* pinhole reprojection error (2x6 J), SE3 only         */
  SRRG2_SLICE_PRIOR        = 3  /* unary prior on the estimate (AlignerSliceProcessorPrior_) */
};

/* concrete CorrespondenceFinder_ behind S/registration/correspondence_finder.h:56 */
enum srrg2_finder_kind {
  SRRG2_FINDER_NONE       = 0, /* prior slices                                        */
  SRRG2_FINDER_NN_GATED   = 1, /* exact nearest neighbour within max_distance         */
  SRRG2_FINDER_PROJECTIVE = 2, /* pinhole projection into the organised fixed cloud   */
  SRRG2_FINDER_CORRESPONDENCES = 3 /* no search: the correspondences are given and stay locked during the
                                      optimisation (MultiLoopDetectorHBST_::_computeAlignments,
                                      S/registration/loop_detector/multi_loop_detector_hbst_impl.cpp:320-352) */
};

/* robustifier bound per slice (S/registration/aligners/aligner_slice_processor_base.h:34-38,
 * RobustifierClamp swap in multi_aligner_impl.cpp:184-201) */
enum srrg2_robustifier_kind {
  SRRG2_ROBUST_NONE      = 0,
  SRRG2_ROBUST_CLAMP     = 1, /* w = 0            for chi >= threshold */
  SRRG2_ROBUST_SATURATED = 2, /* w = thr/chi      for chi >= threshold */
  SRRG2_ROBUST_CAUCHY    = 3  /* w = 1/(1+chi/thr) for chi >= threshold */
};

/* FactorStats::Status as used by multi_aligner_impl.cpp:244 */
enum srrg2_factor_status {
  SRRG2_FACTOR_INLIER     = 0,
  SRRG2_FACTOR_KERNELIZED = 1, /* robustifier fired: counted in num_outliers */
  SRRG2_FACTOR_SUPPRESSED = 2  /* residual could not be evaluated            */
};

enum srrg2_mem { SRRG2_MEM_HOST = 0, SRRG2_MEM_DEVICE = 1, SRRG2_MEM_DEVICE_KEPT = 2 };

/* error codes (<0) */
enum srrg2_error {
  SRRG2_OK            = 0,
  SRRG2_E_INVALID     = -1, /* bad argument / misuse (reference: std::runtime_error) */
  SRRG2_E_NO_DEVICE   = -2, /* no usable HIP device: the product path never falls back to CPU */
  SRRG2_E_HIP         = -3, /* a HIP runtime call failed */
  SRRG2_E_UNSUPPORTED = -4,
  SRRG2_E_STATE       = -5  /* e.g. compute() before clouds were set */
};

/* ---- PODs --------------------------------------------------------------- */

/* srrg2_core::Correspondence: {int fixed_idx; int moving_idx; float response}
 * (field names S/trackers/tracker_slice_processor_impl.cpp:51-55, ctor order
 * S/registration/loop_detector/multi_loop_detector_hbst_impl.cpp:183-191). 12 bytes. */
typedef struct srrg2_correspondence {
  int32_t fixed_idx;
  int32_t moving_idx;
  float   response; /* NN finder: squared distance; projective finder: depth difference */
} srrg2_correspondence;

/* srrg2_solver::IterationStats, the fields the reference reads:
 * num_inliers/num_outliers/chi_inliers (multi_aligner_impl.cpp:81-82,
 * aligner_termination_criteria_impl.cpp:30-32, multi_loop_detector_hbst_impl.cpp:388-391). */
typedef struct srrg2_iteration_stats {
  int32_t iteration;           /* index in the stats vector of this compute()             */
  int32_t num_inliers;         /* factors whose robustifier did not fire (priors included) */
  int32_t num_outliers;        /* factors whose robustifier fired                          */
  int32_t num_suppressed;      /* factors whose residual was not evaluable                 */
  int32_t num_correspondences; /* MultiAlignerBase_::numCorrespondences() at that iteration */
  int32_t solver_status;       /* 0 = SolverBase::Success, 1 = linear system not solvable  */
  float   chi_inliers;
  float   chi_outliers;
} srrg2_iteration_stats;

/* PARAMs of AlignerBase + MultiAlignerBase_ (aligner.h:30; multi_aligner.h:45-57) */
typedef struct srrg2_aligner_params {
  int32_t max_iterations;                   /* default 10 */
  int32_t min_num_inliers;                  /* default 10 */
  int32_t enable_inlier_only_runs;          /* default 0  */
  int32_t keep_only_inlier_correspondences; /* default 0  */
} srrg2_aligner_params;

/* PARAMs of AlignerTerminationCriteriaStandard_ (aligner_termination_criteria.h:40-56) */
typedef struct srrg2_termination_params {
  int32_t window_size;               /* default 5   */
  int32_t num_correspondences_range; /* default 20  */
  int32_t num_inliers_range;         /* default 20  */
  int32_t num_outliers_range;        /* default 20  */
  float   chi_epsilon;               /* default 0.2 */
} srrg2_termination_params;

/* One AlignerSliceProcessor_ / AlignerSliceProcessorPrior_ with its finder and robustifier
 * (aligner_slice_processor.h:56-66,133-150; aligner_slice_processor_base.h:34-53;
 * aligner_slice_odometry_prior.h:17-21,41-45). */
typedef struct srrg2_slice_config {
  int32_t kind;                      /* srrg2_slice_kind */
  int32_t finder;                    /* srrg2_finder_kind */
  int32_t robustifier;               /* srrg2_robustifier_kind */
  float   robustifier_chi_threshold;
  int32_t min_num_correspondences;   /* strict '>' test, aligner_slice_processor_impl.cpp:77-79 */
  float   finder_max_distance;       /* NN gate [m]; projective: max |depth difference| [m] */
  float   finder_normal_cos;         /* accept only if n_f . (R n_m) > this; <= -1 disables */
  float   finder_cell_size;          /* search-grid cell edge [m]; 0 = choose automatically */
  float   sensor_in_robot[12];       /* setSensorInRobot (aligner_slice_processor.h:149); SE2: first 9 */
  float   camera_matrix[9];          /* row-major K, projective finder / reprojection factor */
  int32_t image_rows;
  int32_t image_cols;
  float   depth_min;                 /* projective finder: accepted depth range of the moving point */
  float   depth_max;
  float   prior_information_diag[6]; /* diagonal_info_matrix; SE2 uses the first 3 */
  int32_t prior_sets_initial_guess;  /* init() overrides the guess (aligner_slice_odometry_prior.cpp:19,34) */
} srrg2_slice_config;

/* result record of one alignment of a batch (loop body of
 * S/registration/loop_detector/multi_loop_detector_brute_force_impl.cpp:64-91) */
typedef struct srrg2_batch_result {
  float   moving_in_fixed[12];
  int32_t status;              /* srrg2_status */
  int32_t num_iterations;      /* IterationStats entries produced */
  srrg2_iteration_stats last;  /* iterationStats().back() */
  int32_t num_correspondences; /* aligner->numCorrespondences() AFTER compute(), i.e. after _pruneCorrespondences when
                                  keep_only_inlier_correspondences is set (what the accept gates read:
                                  multi_loop_detector_brute_force_impl.cpp:89, multi_relocalizer_impl.cpp:101) */
  int32_t reserved_;
  float   information[36];     /* H = sum w J^T J (+ priors) of the last Gauss-Newton iteration, D x D row-major in the
                                  first D*D entries (D = 3 | 6): the information of the estimate, e.g. for a closure edge
                                  or for the all-reduce of SURVEY.md section 8e */
} srrg2_batch_result;

typedef struct srrg2_aligner_s* srrg2_aligner_h;

/* ---- library ------------------------------------------------------------ */

int         srrg2_amd_abi_version(void);
const char* srrg2_amd_last_error(void);
/* number of visible HIP devices (<0 on error) */
int         srrg2_amd_device_count(void);

/* ---- aligner: MultiAlignerBase_<Variable> -------------------------------- */

/* ctor of MultiAlignerBase_ (multi_aligner.h:60-66): one variable, graph id 0,
 * solver max_iterations forced to [1].  `device` = HIP device ordinal. */
int srrg2_aligner_create(int variable_kind, int device, srrg2_aligner_h* out);
int srrg2_aligner_destroy(srrg2_aligner_h h);

void srrg2_aligner_default_params(srrg2_aligner_params* p);
void srrg2_termination_default_params(srrg2_termination_params* p);
void srrg2_slice_default_config(srrg2_slice_config* c, int variable_kind);

/* param_max_iterations / min_num_inliers / enable_inlier_only_runs /
 * keep_only_inlier_correspondences (aligner.h:30, multi_aligner.h:45-57) */
int srrg2_aligner_set_params(srrg2_aligner_h h, const srrg2_aligner_params* p);
/* param_termination_criteria (aligner.h:31-35); NULL = run max_iterations */
int srrg2_aligner_set_termination(srrg2_aligner_h h, const srrg2_termination_params* p);
/* param_slice_processors.pushBack (multi_aligner.h:34-37); sets _slices_changed_flag */
int srrg2_aligner_add_slice(srrg2_aligner_h h, const srrg2_slice_config* c, int* slice_idx_out);
int srrg2_aligner_clear_slices(srrg2_aligner_h h);
/* swap a slice's robustifier (slice->param_robustifier.setValue, multi_aligner_impl.cpp:197) */
int srrg2_aligner_set_robustifier(srrg2_aligner_h h, int slice_idx, int kind, float chi_threshold);

/* MultiAlignerBase_::setFixed / setMoving -> slice->bindFixed/bindMoving
 * (multi_aligner_impl.cpp:8-24; aligner_slice_processor_impl.cpp:82-93).
 * coords: n points of dim floats (dim 2 for SE2, 3 for SE3) `coord_stride_bytes` apart;
 * normals may be NULL.  Marks the finder's search structure stale
 * (correspondence_finder.h:80-91). */
int srrg2_aligner_set_fixed(srrg2_aligner_h h, int slice_idx, const float* coords,
                            int coord_stride_bytes, const float* normals,
                            int normal_stride_bytes, int n, int mem);
int srrg2_aligner_set_moving(srrg2_aligner_h h, int slice_idx, const float* coords,
                             int coord_stride_bytes, const float* normals,
                             int normal_stride_bytes, int n, int mem);

/* slice->setSensorInRobot() with the transform the slice looks up on EVERY setMovingInFixed
 * (aligner_slice_processor_impl.cpp:20-36: platform TF frame_id -> base_frame_id): call it whenever the sensor pose
 * changed; valid between computes, takes effect from the next compute() on.  T: 12 (SE3) / 9 (SE2) floats. */
int srrg2_aligner_set_sensor_in_robot(srrg2_aligner_h h, int slice_idx, const float* T);

/* prior slices: the measurement the factor gets in setupFactor()
 * (aligner_slice_odometry_prior.cpp:6-14,23-29; aligner_slice_motion_model.hpp:75-79) */
int srrg2_aligner_set_prior_measurement(srrg2_aligner_h h, int slice_idx, const float* T);

/* setMovingInFixed / movingInFixed (multi_aligner_impl.cpp:27-44) */
int srrg2_aligner_set_moving_in_fixed(srrg2_aligner_h h, const float* T);
int srrg2_aligner_get_moving_in_fixed(srrg2_aligner_h h, float* T_out);

/* MultiAlignerBase_::compute() (multi_aligner_impl.cpp:47-95): blocking; on return the
 * estimate, status and iteration stats are host visible. */
int srrg2_aligner_compute(srrg2_aligner_h h, int* status_out);
/* AlignerBase::status() (aligner.h:51-53) */
int srrg2_aligner_status(srrg2_aligner_h h, int* status_out);

/* Aligner_::iterationStats() (aligner.h:115-117): all iterations of the last compute().
 * *n_inout: capacity of buf on entry, number of entries on return (buf may be NULL to query). */
int srrg2_aligner_get_iteration_stats(srrg2_aligner_h h, srrg2_iteration_stats* buf, int* n_inout);

/* H = sum w J^T J over every factor of every slice (priors included) of the LAST Gauss-Newton iteration of the last
 * compute(): what the solver of MultiAlignerBase_ holds after solver->compute() (multi_aligner_impl.cpp:112-116; the
 * information of the estimate that loop_closure.h:21-79 attaches to a closure).  D x D row-major float (D = 3 or 6);
 * the same values as srrg2_batch_result::information, for plain compute() with any number of cue slices (ABI v4). */
int srrg2_aligner_get_information(srrg2_aligner_h h, float* H_out);

/* MultiAlignerBase_::numCorrespondences() (multi_aligner_impl.cpp:275-285): priors count 1 */
int srrg2_aligner_num_correspondences(srrg2_aligner_h h, int* n_out);
/* slice->correspondences() (aligner_slice_processor.h:92-98), after pruning if enabled;
 * ascending moving_idx.
 * LIFETIME: the passes do not store per-point records; this call (and get_factor_status, the scene merge)
 * DERIVES them from the state the last compute() left on the device -- the clouds, the neighbour of every moving point, the
 * transform of the last executed pass.  They stay derivable until a cloud of the aligner is replaced: after the next
 * set_fixed / set_moving / share_clouds / compute_batch upload the correspondences of the earlier compute() are gone (n = 0),
 * because their indices would refer to the new cloud.  A tracker reads (or stores) them before it binds the next frame,
 * as the reference's does (multi_tracker_impl.cpp:105-108: compute(), then storeCorrespondences()). */
int srrg2_aligner_get_correspondences(srrg2_aligner_h h, int slice_idx, srrg2_correspondence* buf,
                                      int* n_inout);
/* solver->measurementStats() of the last iteration for one cue slice
 * (multi_aligner_impl.cpp:215,244): one srrg2_factor_status byte per correspondence of the
 * un-pruned vector of the last iteration. */
int srrg2_aligner_get_factor_status(srrg2_aligner_h h, int slice_idx, uint8_t* buf, int* n_inout);

/* K independent alignments against the fixed scene already set on `h`
 * (MultiLoopDetectorBruteForce_::compute, multi_loop_detector_brute_force_impl.cpp:63-91;
 * MultiRelocalizer_::compute, multi_relocalizer_impl.cpp:74-88).  Semantically equal to K x
 * { set_moving(slice 0, k); set_moving_in_fixed(guess k); compute() }.  All moving clouds are
 * given as one concatenated array with offsets[K+1] (in points). */
int srrg2_aligner_compute_batch(srrg2_aligner_h h, int K, const float* coords,
                                int coord_stride_bytes, const float* normals,
                                int normal_stride_bytes, const int32_t* offsets, int mem,
                                const float* guesses /* K x 12 (or 9) */,
                                srrg2_batch_result* results);

/* Slices with SRRG2_FINDER_CORRESPONDENCES: factor->setCorrespondences(corrs)
 * (multi_loop_detector_hbst_impl.cpp:330) -- fixed_idx / moving_idx index the clouds given to
 * set_fixed / set_moving; every compute() linearises exactly these pairs (a pair with a
 * non-finite point is Suppressed).  No gate applies: the fixed-point scale of the sums follows
 * the estimate. */
int srrg2_aligner_set_correspondences(srrg2_aligner_h h, int slice_idx, const srrg2_correspondence* correspondences,
                                      int n);
/* K such alignments against the fixed cloud already set (the loop over _correspondences_per_reference,
 * :296-374): moving clouds concatenated with offsets[K+1], correspondences concatenated with
 * corr_offsets[K+1] (moving_idx relative to its own cloud).  Host pointers for the correspondences.
 * Neither table needs to start at 0 (the clouds and the records of a pooled array); a negative first entry or a
 * decreasing table is SRRG2_E_INVALID, refused before the handle is touched. */
int srrg2_aligner_compute_batch_correspondences(srrg2_aligner_h h, int K, const float* coords, int coord_stride_bytes,
                                                const float* normals, int normal_stride_bytes, const int32_t* offsets,
                                                int mem, const srrg2_correspondence* correspondences,
                                                const int32_t* corr_offsets, const float* guesses,
                                                srrg2_batch_result* results);

/* K independent alignments, alignment k = fixed cloud k against moving cloud k, in one call.  Result k is bit for bit
 * what a handle with the same slices, params, termination and tuning returns from
 *   set_fixed(0, F_k, NF_k); set_moving(0, M_k, NM_k); set_moving_in_fixed(G_k); compute()
 * (the all-distinct C4 variant: closure hints between arbitrary pairs of local maps).  Fixed and moving
 * clouds are given concatenated with offsets[K+1] (in points) each, normals optional (null: none), all in host memory or all
 * in device memory (`mem`: SRRG2_MEM_HOST | SRRG2_MEM_DEVICE).  Each fixed cloud gets a search grid of its own, built with
 * those of the other pairs; nothing of a pair but its bounding-box row goes through the host.
 *   supported    slice 0 is the one cue slice: SRRG2_FINDER_NN_GATED, kind P2P or P2PLANE; prior slices may sit beside it
 *                (with the handle's prior measurement, as in compute_batch); SE2_RIGHT, SE3_EULER_RIGHT, SE3_QUAT_RIGHT.
 *   refused      SRRG2_E_UNSUPPORTED: projective, reprojection or given-correspondence slices, more than one cue slice, a
 *                handle with set_point_shard.  SRRG2_E_INVALID, the handle unchanged: K < 0 or K > 65535, decreasing
 *                offsets, null pointers where points exist, bad strides, SRRG2_MEM_DEVICE_KEPT, grids of more than 2^31
 *                cells in all (checked from the fixed clouds' boxes, before the moving clouds are bound).  SRRG2_E_STATE: a
 *                point-to-plane slice without fixed normals, a prior slice without measurement.  K = 0 returns 0.
 *   returns      after it has finished reading the caller's buffers, on success and on error (as compute_batch).
 *   handle after status, estimate, iteration stats and information are those of pair K-1 (as after compute_batch).  The
 *                moving cloud of slice 0 is unbound: a plain compute() needs set_moving first (SRRG2_E_STATE otherwise).
 *                get_correspondences / get_factor_status of the cue slice return SRRG2_E_STATE until the next compute():
 *                pair records are not kept.  The slice's OWN fixed cloud, its grid and its neighbour lists are untouched
 *                (pairs use buffers of their own): a loop detector may interleave compute_batch against its bound map with
 *                pair calls. */
int srrg2_align_pairs(srrg2_aligner_h h, int K,
                      const float* fixed_coords, int fixed_stride_bytes,
                      const float* fixed_normals, int fixed_normal_stride_bytes, const int32_t* fixed_offsets /* K+1 */,
                      const float* moving_coords, int moving_stride_bytes,
                      const float* moving_normals, int moving_normal_stride_bytes, const int32_t* moving_offsets /* K+1 */,
                      int mem /* SRRG2_MEM_HOST | SRRG2_MEM_DEVICE */, const float* guesses /* K x 12 (or 9) */,
                      srrg2_batch_result* results);

/* The K moving clouds of one cue slice in a srrg2_align_batch_slices call: concatenated, offsets[K+1] in points.  A prior slice
 * or a slice that shares another slice's clouds (share_clouds) has an all-null entry. */
typedef struct srrg2_batch_slice_clouds {
  const float*   coords;  int coord_stride_bytes;
  const float*   normals; int normal_stride_bytes;   /* null: none */
  const int32_t* offsets;                            /* K+1 (in points); null: no entry */
} srrg2_batch_slice_clouds;

/* K independent alignments against the bound fixed clouds, every cue slice with a moving cloud of its own per alignment
 * (the loop of MultiLoopDetectorBruteForce_ / MultiRelocalizer_, which bind a whole property container per candidate:
 * every slice picks its moving cloud by name).  Result k is bit for bit what a handle with the same slices, params,
 * termination and tuning returns from
 *   set_moving(s, M[s][k], N[s][k]) for every cue slice s that owns its clouds; set_moving_in_fixed(G_k); compute()
 * Slices bound by share_clouds take their source's cloud k; prior slices use the handle's prior measurement and fixed clouds
 * are the ones bound with set_fixed (as in compute_batch).  A slice's cloud k may be empty: the result is then what compute()
 * gives with that empty cloud bound.  Every (slice, alignment) sizes its fixed-point exponent from its own cloud.
 *   clouds       [nslices], one entry per slice of the handle; all clouds in host memory or all in device memory (`mem`).
 *   supported    any number of cue slices up to SRRG2_MAX_SLICES: nearest-neighbour P2P / P2PLANE slices with clouds of their
 *                own, projective slices (shared clouds too: the RGB-D pack of a point-to-plane and a reprojection slice),
 *                mixtures of the two, prior slices anywhere; SE2_RIGHT, SE3_EULER_RIGHT, SE3_QUAT_RIGHT (projective and
 *                reprojection slices: SE(3) only, as everywhere).
 *   refused      before anything is bound, the handle unchanged.  SRRG2_E_INVALID: nslices differs from the handle's slice
 *                count, K < 0 or K > 65535, a cue slice that owns its clouds without offsets, a prior or sharing slice with a
 *                non-empty entry, decreasing offsets, null pointers where points exist, bad strides, SRRG2_MEM_DEVICE_KEPT.
 *                SRRG2_E_UNSUPPORTED: a given-correspondences slice (compute_batch_correspondences is its batch), a handle
 *                with set_point_shard.  SRRG2_E_STATE: a cue slice without a fixed cloud, P2PLANE without fixed normals, a
 *                projective slice whose fixed cloud is not rows x cols, a prior slice without measurement.  K = 0 returns 0.
 *   memory       a projective slice that owns its association reserves 2 K rows cols 64-bit z-buffer words (VGA: 157 MB at
 *                K = 32, 1.26 GB at K = 256); the batch runs as one launch sequence (no pipelined parts).
 *   returns      after it has finished reading the caller's buffers, on success and on error (as compute_batch).
 *   handle after status, estimate, iteration stats and information are those of alignment K-1 (as after compute_batch);
 *                every cue slice's get_correspondences / get_factor_status returns alignment K-1's records.  The moving
 *                clouds of the batch stay bound as a batch: a plain compute() needs set_moving first (SRRG2_E_STATE). */
int srrg2_align_batch_slices(srrg2_aligner_h h, int K, int nslices, const srrg2_batch_slice_clouds* clouds /* [nslices] */,
                             int mem /* SRRG2_MEM_HOST | SRRG2_MEM_DEVICE */, const float* guesses /* K x 12 (or 9) */,
                             srrg2_batch_result* results);

/* ---- multi-GPU (no reference counterpart) ------------------------------------------
 * Loop-closure candidate alignments are independent: alignment k of K lives on rank k mod G, one process per GPU, one
 * aligner handle per process on its own device; there is no exchange while the alignments run.  The library does not
 * own a communicator (the host side's torch.distributed / RCCL process group does); these helpers fix the sharding
 * rule and the wire format of the one exchange at the end, so that every binding produces the same table.
 *   multi_gpu_init       binds the calling process to device local_rank mod device_count, checks it, returns its ordinal
 *   shard_count/indices  the alignments of `rank`: k = rank, rank + world, ...
 *   pack / unpack        srrg2_batch_result <-> SRRG2_RECORD_FLOATS float64 (X 12, status, num_iterations, num_inliers,
 *                        num_outliers, num_correspondences (after compute), chi_inliers, k, D, H upper triangle 21)
 *   An all-gather of the packed records = the all-reduce(sum) of a K-row table in which every rank fills its own rows
 *   and leaves the others zero: both forms are offered by the host side (distributed.py). */
#define SRRG2_RECORD_FLOATS 41
int srrg2_multi_gpu_init(int local_rank, int* device_out);
int srrg2_multi_gpu_shard_count(int K, int world, int rank);
int srrg2_multi_gpu_shard_indices(int K, int world, int rank, int32_t* indices_out);
int srrg2_multi_gpu_pack_record(int k, int variable_kind, const srrg2_batch_result* r, double* record_out);
int srrg2_multi_gpu_unpack_record(const double* record, int variable_kind, int* k_out, srrg2_batch_result* r_out);

/* Two cue slices that read the SAME clouds: slice `slice_idx` shares the fixed and the moving cloud of slice
 * `source_slice_idx` (no copy; -1 gives it clouds of its own again, to be set).  In the reference a slice finds its clouds
 * BY NAME in the scene (fixed_slice_name / moving_slice_name, aligner_slice_processor_base.h:41-53,
 * aligner_slice_processor_base_impl.cpp:27-50): two slices with the same names bind to the same cloud objects, which is
 * what this call says.  set_fixed / set_moving on the source then serve both; on the sharing slice they are an error.
 * Slices with the projective finder only.  When, on top, their finder parameters agree (camera matrix, image size, depth
 * range, gate, sensor pose) they share ONE association pass per iteration: same results, half the traffic (ABI v4). */
int srrg2_aligner_share_clouds(srrg2_aligner_h h, int slice_idx, int source_slice_idx);

/* ---- one alignment sharded by moving points (second mode; no reference counterpart) ---------
 * For clouds of millions of points one alignment can be spread over G GPUs: the fixed cloud is set on every rank, rank g
 * sets ITS share of the moving points, and every Gauss-Newton iteration adds the ranks' partial sums before the control
 * step -- solver->compute() over all factors (multi_aligner_impl.cpp:112) as an all-reduce(sum) of the per-slice
 * fixed-point sums (int64, exact: the result is bit-identical to the one-GPU alignment of the whole cloud, whatever G
 * is and however the points are dealt).  The library does not own a communicator: it calls `fn` on the aligner's stream
 * order, the host side (torch.distributed / RCCL) performs the reduction IN PLACE on the device buffer:
 *   op SRRG2_REDUCE_SUM_I64  `count` int64 values  (before every control step: the slot sets of the cue slice)
 *   op SRRG2_REDUCE_MAX_U32  `count` uint32 values (once per compute(): the bit pattern of max |coordinate|, which sizes
 *                            the fixed-point exponent and must be the same on every rank)
 * `stream` is the hipStream_t the buffer's producers and consumers are ordered on; fn returns 0 on success.
 * total_moving_points = the number of moving points over all ranks (the other input of the exponent).
 * fn == NULL switches the mode off.  compute() only (K = 1), one nearest-neighbour cue slice plus prior slices. */
#define SRRG2_REDUCE_SUM_I64 0
#define SRRG2_REDUCE_MAX_U32 1
typedef int (*srrg2_reduce_fn)(void* user, int op, void* device_buffer, size_t count, void* stream);
int srrg2_aligner_set_point_shard(srrg2_aligner_h h, srrg2_reduce_fn fn, void* user, int64_t total_moving_points);
/* plain copies for bindings that cannot touch device memory themselves (kind 0: device -> host, 1: host -> device,
 * 2: device -> device; stream == NULL: synchronous, else asynchronous on that hipStream_t) */
int srrg2_amd_memcpy(void* dst, const void* src, size_t bytes, int kind, void* stream);
/* wait for everything queued on `stream` (the hipStream_t a reduction hook was handed) to finish */
int srrg2_amd_stream_synchronize(void* stream);
/* device memory on the calling thread's current device, for bindings that stage a collective's buffer themselves (the record
 * table of a sharded batch on RCCL: include/srrg2_slam_amd_multi_device.hpp, RcclRecordExchange) */
int srrg2_amd_device_malloc(size_t bytes, void** out);
int srrg2_amd_device_free(void* p);

/* ---- pose graph: the global Solver of MultiGraphSLAM_ ---------------------- */
/* MultiGraphSLAM_::optimize() (S/system/multi_graph_slam_impl.cpp:300-317): graph->bindFactors();
 * global_solver->setGraph(graph); global_solver->compute().  The graph holds only pose variables
 * (LocalMap2D/3D = VariableSE2RightAD / VariableSE3QuaternionRightAD, S/mapping/local_map.h:64,75) and binary
 * SE{2,3}PosePoseGeodesicErrorFactor edges (S/registration/loop_closure.h:110-111) built at
 * multi_graph_slam_impl.cpp:71-79 (odometry, Omega = I * info_scale) and :241-293 (closures, created disabled). */
typedef struct srrg2_posegraph_params {
  int32_t max_iterations;     /* Gauss-Newton iterations of one compute() */
  int32_t pcg_max_iterations; /* linear solver: block-Jacobi preconditioned CG */
  float   pcg_tolerance;      /* stop when |r| <= tol * |b| */
  float   damping;            /* lambda added to the diagonal (0 = pure Gauss-Newton) */
} srrg2_posegraph_params;

typedef struct srrg2_posegraph_stats {
  int32_t iteration;
  int32_t num_factors;    /* enabled factors linearised */
  int32_t pcg_iterations;
  int32_t solver_status;  /* 0 = ok, 1 = preconditioner block not positive definite */
  float   chi;            /* sum e^T Omega e at the linearisation point of this iteration */
  float   pcg_residual;   /* |r| / |b| at exit */
} srrg2_posegraph_stats;

typedef struct srrg2_posegraph_s* srrg2_posegraph_h;

/* variable_kind: SRRG2_SE2_RIGHT or SRRG2_SE3_QUAT_RIGHT */
int srrg2_posegraph_create(int variable_kind, int device, srrg2_posegraph_h* out);
int srrg2_posegraph_destroy(srrg2_posegraph_h h);
void srrg2_posegraph_default_params(srrg2_posegraph_params* p);
/* (re)define the whole graph.  poses: V transforms (12 or 9 floats each); fixed_mask: V bytes, non-zero =
 * VariableBase::Fixed (multi_graph_slam_impl.cpp:86), NULL = only pose 0 fixed; ij: E pairs (from, to);
 * Z: E measurements (setMeasurement, :76); omega: E information matrices, row-major DxD float (D = 3 or 6),
 * NULL = identity; enabled: E bytes (LoopClosure_ factors are created disabled, loop_closure.h:71), NULL = all. */
int srrg2_posegraph_set(srrg2_posegraph_h h, int V, const float* poses, const uint8_t* fixed_mask, int E,
                        const int32_t* ij, const float* Z, const float* omega, const uint8_t* enabled);
/* enable / disable factors in place (multi_graph_slam_impl.cpp:285-293) */
int srrg2_posegraph_set_enabled(srrg2_posegraph_h h, const uint8_t* enabled);
/* global_solver->compute(): blocking; poses are updated in place.  stats: one entry per GN iteration. */
int srrg2_posegraph_solve(srrg2_posegraph_h h, const srrg2_posegraph_params* p, srrg2_posegraph_stats* stats,
                          int* n_inout);
int srrg2_posegraph_get_poses(srrg2_posegraph_h h, float* poses_out);

/* Strategy knobs of the pose-graph solver (ABI v4; VERDICT r3: they were environment-only).  Like srrg2_aligner_tuning:
 * a handle starts from srrg2_posegraph_default_tuning() overridden ONCE, in srrg2_posegraph_create, by the SRRG2_AMD_PG_*
 * variables named below; solve() contains no getenv.  Every setting solves the same linear systems to the same tolerance:
 * the knobs choose the preconditioner's shape and how it is launched.  No reference counterpart (the reference's solver is
 * srrg2_solver's sparse Cholesky, configured through BOSS). */
typedef struct srrg2_posegraph_tuning {
  int32_t match_passes;     /* SRRG2_AMD_PG_PASSES: pairwise-matching passes per multigrid level: aggregates of <= 2^passes
                               poses (3)                                                                             */
  int32_t two_phase;        /* SRRG2_AMD_PG_TWO_PHASE: levels below level 0 take one launch down and one up (1) instead of
                               six (0)                                                                               */
  int32_t use_graph;        /* SRRG2_AMD_PG_GRAPH: chunks of 10 CG iterations replayed from a HIP graph (1); 0 = launched one
                               by one (needed under rocprofv3 --kernel-trace)                                        */
  int32_t debug;            /* SRRG2_AMD_PG_DEBUG: print the hierarchy and the host's set-up time by phase to stderr (0) */
  int32_t keep_structure;   /* the multigrid hierarchy's STRUCTURE (aggregates, sparsity patterns: 13 ms per build on C5)  
                               is kept while the graph's topology does not change -- srrg2_posegraph_set with the same
                               edges, fixed and enabled masks -- (1); 0 = rebuilt by the first solve after every set    */
  float   omega_p;          /* SRRG2_AMD_PG_OMEGA_P: damping of the Jacobi sweep that smooths the interpolation (0.75; 0 =
                               plain aggregation)                                                                    */
  float   omega;            /* SRRG2_AMD_PG_OMEGA: damping of the block-Jacobi smoother (0.8)                           */
  float   lag_below;        /* SRRG2_AMD_PG_LAG: a Gauss-Newton iteration keeps the hierarchy's numerics of the previous one
                               when that one moved no variable by more than this (0.05; 0 = never: every iteration rebuilds
                               interpolation and coarse operators, 3 ms each on C5)                                   */
  int32_t device_structure; /* SRRG2_AMD_PG_DEVICE_STRUCTURE: the sparsity patterns of the hierarchy (interpolation, Q = H Ps, column
                               lists, coarse edges) are built on the device by sort + unique (1) instead of on the host (0: 13 of
                               the 25 ms a structure build takes on C5); the arrays are the same entry for entry          */
  int32_t reserved_[7];
} srrg2_posegraph_tuning;
void srrg2_posegraph_default_tuning(srrg2_posegraph_tuning* t);
int srrg2_posegraph_get_tuning(srrg2_posegraph_h h, srrg2_posegraph_tuning* t_out);
int srrg2_posegraph_set_tuning(srrg2_posegraph_h h, const srrg2_posegraph_tuning* t);

/* Incremental interface = the pose-graph lifecycle of MultiGraphSLAM_.  The graph
 * stays in device memory between solves; graph ids are indices in insertion order.
 *   add_variable          _graph->addVariable(local map)  (S/system/multi_graph_slam_impl.cpp:70; the first one is
 *                         Fixed, :86: pass fixed = 1)
 *   add_factor            _graph->addFactor(odometry factor / closure)  (:71-79, :238-241); information = D x D
 *                         row-major or null for identity; closures enter with enabled = 0
 *   set_factor_enabled    closure->setEnabled(true) after validation  (:247-249, :283-286)
 *   remove_factor         _graph->removeFactor(rejected closure)  (:279-281); the other ids do not change
 *   size                  variables, factors still in the graph, enabled factors */
int srrg2_posegraph_add_variable(srrg2_posegraph_h h, const float* pose, int fixed, int* id_out);
int srrg2_posegraph_add_factor(srrg2_posegraph_h h, int i, int j, const float* Z, const float* information, int enabled,
                               int* id_out);
int srrg2_posegraph_set_factor_enabled(srrg2_posegraph_h h, int factor_id, int enabled);
int srrg2_posegraph_remove_factor(srrg2_posegraph_h h, int factor_id);
int srrg2_posegraph_size(srrg2_posegraph_h h, int* num_variables, int* num_factors, int* num_enabled_factors);
/* How the last solve treated what was appended since the multigrid hierarchy's structure was built: `hierarchy_builds` =
 * structure builds of this handle so far; `eliminated_leaves` = variables the last solve eliminated exactly instead of rebuilding
 * (makeNewMap's pattern, multi_graph_slam_impl.cpp:52-90: one new variable with one factor to an older one -- a leaf of the graph,
 * whose Schur complement leaves the older graph's system and with it the hierarchy untouched; up to 32 of them, then a rebuild; a
 * factor between two older variables, a changed flag or keep_structure = 0 rebuild as before). */
int srrg2_posegraph_structure_info(srrg2_posegraph_h h, int* hierarchy_builds, int* eliminated_leaves);

/* Robust kernels on pose-graph factors (the reference robustifies its solver factors too: factor->setRobustifier,
 * multi_loop_detector_hbst_impl.cpp:337).  A factor's weight is the aligner's formula (srrg2_robustifier_kind), in double:
 * w = 1 for chi < thr; for chi >= thr CLAMP gives 0, SATURATED thr/chi, CAUCHY 1/(1 + chi/thr).
 * Iteratively reweighted Gauss-Newton: every iteration of srrg2_posegraph_solve computes w from the chi at that iteration's
 * linearisation point and adds w J^T Omega J and w J^T Omega e.  srrg2_posegraph_stats.chi stays the raw sum of e^T Omega e
 * over the enabled factors.  Defaults: srrg2_posegraph_set resets every factor to NONE, add_factor starts one at NONE,
 * remove_factor drops it; ids keep their meaning across remove_factor.  Robustifiers are numerics, not topology: setting
 * one does not rebuild the multigrid hierarchy (structure_info's hierarchy_builds stays) nor disturb the elimination of
 * appended leaves, which are eliminated with their weight.  A free variable whose factors are all weighted 0 (CLAMP) has a
 * singular block: solver_status = 1, the poses are left as they were.
 * Errors: a bad or removed id, an unknown kind, or a threshold that is not positive and finite (kind != NONE) return
 * SRRG2_E_INVALID and leave the handle unchanged. */
/* robustifier of one factor (kind: srrg2_robustifier_kind; chi_threshold > 0 and finite unless kind == NONE) */
int srrg2_posegraph_set_factor_robustifier(srrg2_posegraph_h h, int factor_id, int kind, float chi_threshold);
/* the same for every factor id 0..E-1 at once (like set_enabled: entries of removed ids are ignored);
 * kinds == NULL: all NONE */
int srrg2_posegraph_set_robustifiers(srrg2_posegraph_h h, const int32_t* kinds, const float* chi_thresholds);
/* chi = e^T Omega e and the robust weight w(chi) of every factor id at the CURRENT poses, enabled or not (E floats each;
 * either pointer may be NULL); a removed id gives chi = NaN, weight = 0.  Changes nothing in the graph. */
int srrg2_posegraph_evaluate_factors(srrg2_posegraph_h h, float* chi_out, float* weight_out);

/* ---- scene slices kept in HBM between frames: clipping and correspondence-based merging ------
 * the tracker-side steps either side of align()
 * (S/trackers/tracker_slice_processor_impl.cpp:111-205: merge(), clip()).  A scene is a point
 * cloud with optional normals (PointNormal2f / PointNormal3f clouds, S/mapping/
 * merger_correspondence_homo.h:38-47); a point is Valid iff its coordinates are finite.  Scenes
 * live in device memory with spare capacity, so adapt -> clip -> align -> merge runs without
 * moving clouds across PCIe. */

typedef struct srrg2_scene* srrg2_scene_h;

/* MergerBase::Status, S/mapping/merger.h:19-23 (values identical) */
enum srrg2_merger_status { SRRG2_MERGER_ERROR = 0, SRRG2_MERGER_INITIALIZING = 1, SRRG2_MERGER_SUCCESS = 2 };
/* SceneClipper_::Status, S/mapping/scene_clipper.h:24-28 (values identical) */
enum srrg2_clipper_status { SRRG2_CLIPPER_ERROR = 0, SRRG2_CLIPPER_SUCCESSFUL = 1, SRRG2_CLIPPER_READY = 2 };

/* PARAMs of MergerCorrespondence_ / MergerCorrespondenceHomo_ (S/mapping/merger.h:126-131,
 * S/mapping/merger_correspondence_homo.h:22-31), same defaults: 50, 0.25, 200 */
typedef struct srrg2_merger_params {
  float maximum_response;
  float maximum_distance_geometry_squared;
  int32_t target_number_of_merges;
} srrg2_merger_params;

typedef struct srrg2_merge_result {
  int32_t status;            /* srrg2_merger_status */
  int32_t num_correspondences;
  int32_t num_merged;        /* distinct measurement points merged into the scene (merged_points_moving.size()) */
  int32_t num_added;         /* measurement points appended to the scene */
  int32_t scene_size;        /* after the merge */
} srrg2_merge_result;

int srrg2_merger_default_params(srrg2_merger_params* p);

/* dim = 2 | 3.  An empty scene. */
int srrg2_scene_create(int dim, int device, srrg2_scene_h* out);
int srrg2_scene_destroy(srrg2_scene_h h);
/* replace the content (strides in bytes; normals may be null; mem = srrg2_mem) */
int srrg2_scene_set(srrg2_scene_h h, const float* coords, int coord_stride_bytes, const float* normals,
                    int normal_stride_bytes, int n, int mem);
int srrg2_scene_size(srrg2_scene_h h, int* n);
/* copy out up to `capacity` points as packed dim-float records (normals_out may be null) */
int srrg2_scene_get(srrg2_scene_h h, float* coords_out, float* normals_out, int capacity, int* n);
/* borrow the device arrays (float4 records: stride 16 bytes) -- e.g. to feed
 * srrg2_aligner_set_fixed/set_moving with SRRG2_MEM_DEVICE without touching the host.  Valid
 * until the scene is next modified. */
int srrg2_scene_device_arrays(srrg2_scene_h h, const float** coords, const float** normals, int* n);

/* Per-point features: a 256-bit descriptor (SRRG2_DESCRIPTOR_BYTES bytes) and a float intensity, the extra fields of
 * PointIntensityDescriptor2f / 3f -- the cloud type of the reference's second merger (S/mapping/
 * merger_correspondence_homo.h:36-40) and of its HBST detector, which reads the descriptors back from the local map's cloud
 * (multi_loop_detector_hbst_impl.cpp:84-85, :131-136).  They travel with the point through every scene operation:
 *   set_features   n must equal the scene's size (else SRRG2_E_INVALID, scene unchanged).  Either pointer may be NULL: that
 *                  field is then absent; both NULL drops the features.  Strides in bytes: descriptors >= 32 (any alignment),
 *                  intensity >= 4 and a multiple of 4 (else SRRG2_E_INVALID).  mem: SRRG2_MEM_HOST | SRRG2_MEM_DEVICE.
 *   srrg2_scene_set replaces the content and so drops the features.  A scene that never got features behaves as before.
 *   validity       unchanged: a point is Valid iff its coordinates are finite; an invalid point keeps its features and index.
 *   clip_ball / clip_projective / clip_scan
 *                  `clipped` receives the features of the points it keeps (clipped[k] = full[global_indices[k]]) and
 *                  the feature presence of `full`.
 *   merge / merge_from_aligner
 *                  a merged scene point takes the measurement point's descriptor and intensity (point_scene = point_meas,
 *                  merger_correspondence_homo_impl.cpp:71); of several correspondences onto one scene point the last one that
 *                  passed both gates, in correspondence order, decides.  Appended points carry their features unchanged
 *                  (:35-40, :103-115).  An EMPTY scene adopts the measurement's feature presence; otherwise scene and
 *                  measurement must agree field by field: SRRG2_E_STATE, both handles unchanged.
 *   get_features   like srrg2_scene_get: up to `capacity` points, descriptors as packed 32-byte rows; an absent field is
 *                  not written (either pointer may be NULL).
 *   device_features  like srrg2_scene_device_arrays: descriptors as rows of 32 bytes (16-byte aligned), intensities as
 *                  floats; NULL for an absent field.  Valid until the scene is next modified. */
#ifndef SRRG2_DESCRIPTOR_BYTES
#define SRRG2_DESCRIPTOR_BYTES 32
#endif
int srrg2_scene_set_features(srrg2_scene_h h, const uint8_t* descriptors, int descriptor_stride_bytes, const float* intensity,
                             int intensity_stride_bytes, int n, int mem);
int srrg2_scene_has_features(srrg2_scene_h h, int* has_descriptors, int* has_intensity);
int srrg2_scene_get_features(srrg2_scene_h h, uint8_t* descriptors_out, float* intensity_out, int capacity, int* n);
int srrg2_scene_device_features(srrg2_scene_h h, const uint8_t** descriptors, const float** intensity, int* n);

/* SceneClipper_::compute() (S/mapping/scene_clipper.h:17-122; the reference ships the interface
 * only, concrete clippers live in the SLAM pipelines): ball policy -- keeps the Valid points of
 * `full` within `range` of the robot, in scene order, expressed in the robot frame
 * (local_map_in_robot * p, normals rotated: "the clipped scene will be compared directly with
 * the measurement", :106-107).  `clipped` receives the points and the local -> global index map
 * (globalIndices(), :98-101).  status: Ready when `full` is empty, else Successful. */
int srrg2_scene_clip_ball(srrg2_scene_h full, const float* robot_in_local_map, float range, srrg2_scene_h clipped,
                          int* status);
int srrg2_scene_global_indices(srrg2_scene_h clipped, int32_t* buf, int* n_inout);

/* SceneClipper_::compute() with the projective policy (defined here from first principles, like the ball policy: the
 * reference's concrete projective clipper lives in its RGB-D pipeline).  Keeps the Valid points of `full` that a pinhole camera
 * mounted at sensor_in_robot (SceneClipper_::setSensorInRobot, scene_clipper.h:86-89) sees from robot_in_local_map:
 *   r = robot_in_local_map^-1 * p, c = sensor_in_robot^-1 * r, projected exactly as the projective finder projects
 *   (depth_min <= c.z <= depth_max, u = (K0*c.x)/c.z + K2, v = (K4*c.y)/c.z + K5, in view iff 0 <= u+0.5 < cols and
 *   0 <= v+0.5 < rows, pixel = floor(v+0.5)*cols + floor(u+0.5));
 *   occlusion_margin < 0: every in-view point is kept (frustum only); >= 0: only those with
 *   c.z <= (minimum c.z over the in-view points of the pixel) + occlusion_margin -- 0 keeps every point that ties for the
 *   minimum, +inf equals frustum only.  DESIGN.md section 4 "Projective clipping" is the arithmetic contract.
 * Output as clip_ball: the kept points in scene order, in the ROBOT frame (r, bit for bit what clip_ball writes for the same
 * point; the aligner applies robot_in_sensor itself), normals rotated, global indices, features and their presence.
 *   refused   `clipped` unchanged.  SRRG2_E_INVALID: a null handle, pose or params; full == clipped; different devices or dims;
 *             rows or cols <= 0 or rows*cols beyond int32; !(depth_min > 0) or !(depth_max >= depth_min); fx or fy zero / not
 *             finite; a NaN margin.  SRRG2_E_UNSUPPORTED: scenes of dim 2 (their clipper is srrg2_scene_clip_scan), K with
 *             skew.
 *   status    Ready when `full` is empty, else Successful -- also when nothing is kept (`clipped` is then empty). */
typedef struct srrg2_projective_clip_params {
  float   camera_matrix[9];   /* row-major K; K[0][1] != 0 -> SRRG2_E_UNSUPPORTED (as the depth adaptor) */
  int32_t image_rows, image_cols;
  float   depth_min, depth_max;
  float   sensor_in_robot[12];
  float   occlusion_margin;   /* < 0: frustum only; >= 0: metres behind the nearest point of the pixel */
} srrg2_projective_clip_params;
typedef struct srrg2_clip_result {
  int32_t status;        /* srrg2_clipper_status */
  int32_t num_valid;     /* Valid points of full */
  int32_t num_in_view;   /* of those, inside the depth range and the image */
  int32_t num_kept;      /* == srrg2_scene_size(clipped) */
} srrg2_clip_result;
/* identity sensor, depth 0.4 .. 8 m, margin -1 (frustum only); camera_matrix (identity) / rows / cols (0) are the caller's */
void srrg2_clip_default_projective_params(srrg2_projective_clip_params* p);
int srrg2_scene_clip_projective(srrg2_scene_h full, const float* robot_in_local_map, const srrg2_projective_clip_params* p,
                                srrg2_scene_h clipped, srrg2_clip_result* out /* may be NULL */);

/* SceneClipper_::compute() with the scan policy, the 2-D twin of the projective one (first principles as well).  Keeps the Valid
 * points of a 2-D `full` that a planar laser scanner mounted at sensor_in_robot sees from robot_in_local_map:
 *   r = robot_in_local_map^-1 * p, c = sensor_in_robot^-1 * r, rho = sqrtf(c.x*c.x + c.y*c.y), range_min <= rho <= range_max,
 *   bearing dm::atan2(c.y, c.x) binned to the nearest beam of angle_min + k*angle_increment, k in [0, num_beams), after at most
 *   one turn of 2 pi either way (the sector may cross +-pi; a clockwise scanner has a negative increment);
 *   occlusion_margin < 0: every in-view point is kept (sector only); >= 0: only those with
 *   rho <= (minimum rho over the in-view points of the beam) + occlusion_margin -- 0 keeps every point that ties for the
 *   minimum, +inf equals sector only.  DESIGN.md section 4 "Scan clipping" is the arithmetic contract.
 * Output as clip_ball: the kept points in scene order, in the ROBOT frame (r, bit for bit what clip_ball writes for the same
 * point), normals rotated, global indices, features and their presence.  srrg2_clip_result.num_in_view: inside the range
 * interval and the sector.
 *   refused   `clipped` unchanged.  SRRG2_E_INVALID: a null handle, pose or params; full == clipped; different devices or dims;
 *             num_beams <= 0; angle_increment zero or not finite; angle_min not finite or |angle_min| > 2 pi;
 *             |angle_increment| * num_beams beyond 2 pi plus one increment (361 beams over 360 degrees are legal, two turns are
 *             not; a relative slack of 2^-20 admits increments rounded to float32); !(range_min > 0) or
 *             !(range_max >= range_min); a NaN margin.  SRRG2_E_UNSUPPORTED: scenes of dim 3 (a 3-D lidar's view:
 *             srrg2_scene_clip_spherical; a camera's: srrg2_scene_clip_projective).
 *   status    Ready when `full` is empty, else Successful -- also when nothing is kept (`clipped` is then empty). */
typedef struct srrg2_scan_clip_params {
  double  angle_min, angle_increment;   /* as srrg2_scan_adaptor_params: bearing of beam k = angle_min + k*angle_increment */
  int32_t num_beams;
  float   range_min, range_max;         /* accepted range in the SENSOR frame, both inclusive */
  float   sensor_in_robot[9];           /* SE(2), row-major 3x3 */
  float   occlusion_margin;             /* < 0: sector only; >= 0: metres behind the nearest point of the beam */
} srrg2_scan_clip_params;
/* identity sensor, range 0.05 .. 30 m (the scan adaptor's), margin -1 (sector only); bearings / num_beams (0) are the caller's */
void srrg2_clip_default_scan_params(srrg2_scan_clip_params* p);
int srrg2_scene_clip_scan(srrg2_scene_h full, const float* robot_in_local_map /* 3x3 */, const srrg2_scan_clip_params* p,
                          srrg2_scene_h clipped, srrg2_clip_result* out /* may be NULL */);

/* The spherical sensor model of a spinning 3-D lidar: a range image of rows (rings, uniformly spaced in elevation; a per-ring
 * table: srrg2_scene_clip_spherical_rings, srrg2_lidar_sweep_extras) x cols (azimuth steps).  Shared by srrg2_adapt_lidar_sweep and srrg2_scene_clip_spherical, which project a sensor-frame point
 * c = (x, y, z) the same way (DESIGN.md section 4 "Lidar sweeps" is the arithmetic contract):
 *   rho = sqrtf((x*x + y*y) + z*z), range_min <= rho <= range_max;
 *   azimuth dm::atan2(y, x) binned to the nearest column after at most one turn of 2 pi either way (as clip_scan bins a
 *   bearing); elevation dm::atan2(z, sqrt(x*x + y*y)) binned to the nearest row, no wrap; pixel = row*cols + col.
 *   invalid   (SRRG2_E_INVALID from both calls) rows or cols <= 0 or rows*cols beyond int32; an increment zero or not finite;
 *             azimuth_min not finite or |azimuth_min| > 2 pi; |azimuth_increment| * cols beyond 2 pi plus one increment (slack
 *             2^-20, as clip_scan); elevation_min not finite, or the first or last row's elevation outside [-pi/2, pi/2]
 *             (slack 2^-20); !(range_min > 0) or !(range_max >= range_min).
 *   wrap      the columns close the circle iff | |azimuth_increment| * cols - 2 pi | <= 2 pi * 2^-20 (the adaptor's normals). */
typedef struct srrg2_spherical_model {
  double  azimuth_min, azimuth_increment;     /* azimuth of column c = azimuth_min + c*azimuth_increment (radians; negative
                                                 increment = clockwise) */
  double  elevation_min, elevation_increment; /* elevation of row r = elevation_min + r*elevation_increment (negative increment
                                                 = row 0 on top) */
  int32_t rows, cols;
  float   range_min, range_max;               /* accepted range, both inclusive */
} srrg2_spherical_model;
/* a full turn: azimuth_increment = 2 pi / cols, azimuth_min = -pi + pi / cols (the columns tile [-pi, pi)), elevation_min =
 * elevation_first, elevation_increment = (elevation_last - elevation_first) / (rows - 1), range 0.5 .. 120 m.
 * SRRG2_E_INVALID (m unchanged): null m, rows < 2, cols < 1, elevations not finite or equal. */
int srrg2_spherical_model_full_turn(srrg2_spherical_model* m, int rows, int cols, double elevation_first, double elevation_last);

/* SceneClipper_::compute() with the spherical policy, the 3-D twin of the scan one.  Keeps the Valid points of a 3-D `full`
 * that a lidar mounted at sensor_in_robot sees from robot_in_local_map:
 *   r = robot_in_local_map^-1 * p, c = sensor_in_robot^-1 * r (c finite), projected by the model above;
 *   occlusion_margin < 0: every in-view point is kept (field of view only); >= 0: only those with
 *   rho <= (minimum rho over the in-view points of the pixel) + occlusion_margin -- 0 keeps every point that ties for the
 *   minimum, +inf equals field of view only.
 * Output as clip_ball: the kept points in scene order, in the ROBOT frame (r, bit for bit what clip_ball writes for the same
 * point), normals rotated, global indices, features and their presence.  srrg2_clip_result.num_in_view: inside the range
 * interval and the image.
 *   refused   `clipped` unchanged.  SRRG2_E_INVALID: a null handle, pose or params; full == clipped; different devices or dims;
 *             an invalid model; a NaN margin; reserved != 0.  SRRG2_E_UNSUPPORTED: scenes of dim 2 (srrg2_scene_clip_scan).
 *   status    Ready when `full` is empty, else Successful -- also when nothing is kept (`clipped` is then empty). */
typedef struct srrg2_spherical_clip_params {
  srrg2_spherical_model model;
  float   sensor_in_robot[12];
  float   occlusion_margin;   /* < 0: field of view only; >= 0: metres behind the nearest point of the pixel */
  int32_t reserved;           /* 0 */
} srrg2_spherical_clip_params;
/* identity sensor, range 0.5 .. 120 m, margin -1 (field of view only); the model's angles / rows / cols (0) are the caller's */
void srrg2_clip_default_spherical_params(srrg2_spherical_clip_params* p);
int srrg2_scene_clip_spherical(srrg2_scene_h full, const float* robot_in_local_map, const srrg2_spherical_clip_params* p,
                               srrg2_scene_h clipped, srrg2_clip_result* out /* may be NULL */);

/* srrg2_scene_clip_spherical for a sensor whose rings are not uniformly spaced: ring_elevations[r] (HOST memory, p->model.rows
 * doubles, radians) is the elevation of row r, strictly ascending or strictly descending.  The model's elevation_min and
 * elevation_increment are then neither read nor validated; everything else is srrg2_scene_clip_spherical's.
 *   rows      boundaries in float64: b[0] = e[0] - (e[1] - e[0])*0.5, b[k] = (e[k-1] + e[k])*0.5, b[rows] = e[rows-1] +
 *             (e[rows-1] - e[rows-2])*0.5; a point of elevation eps is in view iff it lies in [b[0], b[rows]) (descending
 *             table: (b[rows], b[0]]) and takes the row whose interval holds it; a point on a boundary goes to the higher row
 *             index.  The adaptor (srrg2_lidar_sweep_extras.ring_elevations) bins the same way.
 *   NULL      ring_elevations == NULL is srrg2_scene_clip_spherical, bit for bit.
 *   refused   `clipped` unchanged.  SRRG2_E_INVALID: rows < 2; an entry not finite or beyond (pi/2)(1 + 2^-20) in magnitude; a
 *             table that is not strictly monotonic; whatever srrg2_scene_clip_spherical refuses.  SRRG2_E_UNSUPPORTED: rows > 256.
 *   waits     the table is consumed before the call returns. */
int srrg2_scene_clip_spherical_rings(srrg2_scene_h full, const float* robot_in_local_map, const srrg2_spherical_clip_params* p,
                                     const double* ring_elevations /* HOST, p->model.rows entries; NULL = plain */,
                                     srrg2_scene_h clipped, srrg2_clip_result* out /* may be NULL */);

/* Normals for a scene that arrived as a plain list of points (a 3-D lidar sweep, a map from disk, srrg2_scene_set without
 * normals, a merged map whose averaged normals have drifted): per point the PCA of its radius neighbourhood, on the device.
 * No reference counterpart; DESIGN.md section 4 "Normals of unorganised scenes" is the arithmetic contract, bit for bit.
 *   neighbours   j is a neighbour of i iff both have finite coordinates and d2 <= radius*radius (float32, the gated finder's
 *                operation order, inclusive); i is its own neighbour.  Scenes of dim 2: the 2x2 problem, z ignored.
 *   normal       the eigenvector of the smallest eigenvalue of the neighbourhood's covariance (float64, fixed Jacobi sweeps),
 *                turned towards `viewpoint` (scene frame); a NaN in any of the three components of viewpoint = no viewpoint:
 *                the component of largest magnitude is made positive.  curvature = lambda0 / (sum of lambdas).
 *   no normal    a point with a non-finite coordinate; fewer than min_neighbours neighbours (too_few); all neighbours
 *                coincident, trace <= 0 or not finite (degenerate); float32(curvature) > max_curvature (too_curved) -- counted in
 *                the first that applies.  drop_points_without_normal = 1: such points leave the scene (stable compaction;
 *                descriptor and intensity move with their point; srrg2_scene_global_indices gives every survivor's index before
 *                the call, as the adaptors' compact mode).  0: order, size and global indices stay, their normal is NaN.
 *   afterwards   the scene has normals (existing ones are replaced).  curvature_out[i] (host, capacity = the size before the
 *                call, may be NULL) refers to index i BEFORE the call: the curvature where a covariance was formed and not
 *                degenerate, else NaN.
 *   refused      the scene unchanged.  SRRG2_E_INVALID: null handle or params; radius not finite or <= 0, or so large / small
 *                that radius*radius is infinite / 0 in float32 (admissible: about 1e-22 .. 1.8e19); min_neighbours <
 *                dim + 1; max_curvature NaN; drop_points_without_normal not 0 / 1.  SRRG2_E_UNSUPPORTED: the extent.  Points are
 *                binned into cells floor((p - bbox_min) / h), h = radius * (1 + 2^-16), in float64; the 64-bit cell key holds at
 *                most 2^30 cells per axis and 63 bits over the axes (an axis of c cells takes the bits of c - 1): two clusters
 *                10^7 radii apart along one axis are fine, 10^7 radii apart along all three are refused.  Memory is O(n)
 *                whatever the extent.
 *   empty scene  succeeds, all-zero result.
 *   waits        one host wait when out, curvature_out or the compaction needs a number.  With drop = 0 and both NULL the work
 *                is queued on the scene's stream and the call returns (the next srrg2_scene_* call settles it, like an
 *                organised adaptor write): srrg2_scene_device_arrays + set_fixed(..., SRRG2_MEM_DEVICE_KEPT) can follow at
 *                once.  The extent cannot be refused from there: beyond the key range every normal comes out NaN. */
typedef struct srrg2_normals_params {
  float   radius;                 /* neighbourhood: d2 <= radius*radius, INCLUSIVE; finite, > 0 (default 0.1) */
  int32_t min_neighbours;         /* neighbours counted INCLUDING the point itself; >= dim+1; default 5 (dim 3) / 3 (dim 2) */
  float   max_curvature;          /* lambda0 / (sum of lambdas) above this -> no normal; default 1 (gate off) */
  float   viewpoint[3];           /* in the scene's frame; normals face it (default: the origin); NaN = no viewpoint */
  int32_t drop_points_without_normal; /* 1 (default): such points leave the scene; 0: they stay, normal = NaN */
  int32_t reserved;               /* 0 (default_params sets it); not read: keeps the struct at 32 bytes */
} srrg2_normals_params;

typedef struct srrg2_normals_result {
  int32_t num_points, num_finite, num_with_normal, num_too_few, num_degenerate, num_too_curved, scene_size;
} srrg2_normals_result;

void srrg2_normals_default_params(srrg2_normals_params* p, int dim);
int  srrg2_scene_estimate_normals(srrg2_scene_h scene, const srrg2_normals_params* p,
                                  float* curvature_out /* host, may be NULL, capacity = size before the call */,
                                  srrg2_normals_result* out /* may be NULL */);
/* the exponents of the fixed-point moment sums (first moments scaled by 2^e1, second by 2^e2): functions of the radius and
 * the scene size alone -- with radius < 2^E (frexp) and n <= 2^L: e1 = min(61 - L - E, 50 - E), e2 = min(61 - L - 2E, 50 - 2E).
 * No device needed. */
void srrg2_normals_exponents(float radius, int n, int* e1, int* e2);

/* Voxel-grid decimation: `dst` receives one point per occupied cell of a grid of `leaf_size` cubes (squares for dim 2), on the
 * device.  No reference counterpart (the caller is srrg2_core's cloud voxelize); DESIGN.md section 4 "Voxel-grid decimation" is
 * the contract and tests/voxel_restatement.py its executable form: the result is a function of the points and the parameters
 * alone, bit for bit.  The call has a clipper's shape: two distinct scenes of one dim on one device, `src` untouched, `dst`
 * replaced (it takes src's feature presence and has_normals), srrg2_scene_global_indices(dst) names each emitted point's
 * representative in src.
 *   cell            a point takes part iff its dim coordinates are finite; c_d = floor(((double) p_d - origin_d) / leaf) in
 *                   float64 (dim 2: z ignored; a point on a face belongs to the upper cell; negative coordinates floor down).
 *   representative  the cell's participating point with the lowest scene index.  A cell is emitted when it has at least
 *                   min_points_per_voxel participating points; cells come out in ascending order of their representative:
 *                   "the first point seen of every cell, in scene order".  A cloud with one point per cell comes back unchanged.
 *   FIRST           the representative verbatim: coordinates, normal, descriptor, intensity.
 *   CENTROID        coordinates: a cell of one point emits it verbatim; k > 1 points: about corner_d = origin_d + c_d * leaf the
 *                   offsets are rounded to multiples of 2^-e (half to even), summed in int64, and
 *                   float32(corner_d + (S_d * 2^-e) / k) comes out; e = e1 of srrg2_normals_exponents(leaf_size, size of src).
 *                   Normals (src has normals): a normal contributes iff its dim components are finite and below 2 in magnitude;
 *                   components rounded to multiples of 2^-en (en = e1 of srrg2_normals_exponents(1, size of src)), summed in
 *                   int64, normalised in float64; NaN when none contributed or the sum is zero.
 *                   Descriptor and intensity: the representative's (descriptors cannot be averaged).
 *   counts_out[k]   (host, may be NULL, capacity = the size of src) participating points in the cell of emitted point k; words
 *                   beyond the size of dst are zeroed.
 *   result          num_occupied counts cells before the min_points gate, max_points_per_voxel is over the occupied cells,
 *                   num_with_normal counts the emitted points whose normal has no NaN component (0 when src has no normals).
 *   refused         `dst` keeps its content.  SRRG2_E_INVALID: a null handle or params; src == dst; different dims or devices; a
 *                   leaf not finite or <= 0; an origin not finite; a mode outside the enum; min_points_per_voxel < 1; non-zero
 *                   reserved.  SRRG2_E_UNSUPPORTED: the extent -- cell coordinates are keyed relative to the lowest occupied
 *                   cell per axis; the 64-bit cell key holds at most 2^30 cells per axis and 63 bits over the axes (as
 *                   srrg2_scene_estimate_normals).  Memory is O(n) whatever the extent.
 *   empty src       succeeds, all-zero result, `dst` empty.
 *   waits           one host wait (a `dst` without room for the result: a second one, as the clippers). */
enum srrg2_voxel_mode { SRRG2_VOXEL_CENTROID = 0, SRRG2_VOXEL_FIRST = 1 };
typedef struct srrg2_voxel_params {
  float   leaf_size;             /* cell edge [m], finite, > 0; default 0.05 */
  float   origin[3];             /* a grid corner, scene frame; default 0: the grid is anchored to the frame, not to the data */
  int32_t mode;                  /* srrg2_voxel_mode; default CENTROID */
  int32_t min_points_per_voxel;  /* >= 1; default 1; cells with fewer finite points emit nothing */
  int32_t reserved[2];           /* 0; struct = 32 bytes */
} srrg2_voxel_params;
typedef struct srrg2_voxel_result {
  int32_t num_points, num_finite, num_occupied, num_voxels /* emitted == size of dst */, num_with_normal, max_points_per_voxel;
} srrg2_voxel_result;
void srrg2_voxel_default_params(srrg2_voxel_params* p);
int  srrg2_scene_voxelize(srrg2_scene_h src, const srrg2_voxel_params* p, srrg2_scene_h dst,
                          int32_t* counts_out /* host, may be NULL, capacity = size of src */,
                          srrg2_voxel_result* out /* may be NULL */);

/* MergerCorrespondenceHomo_::compute() (S/mapping/merger_correspondence_homo_impl.cpp:11-125).
 * correspondences: fixed_idx = scene point, moving_idx = measurement point, processed in order
 * (a scene point hit twice sees the first update, :55-73); n_correspondences < 0 = "no
 * correspondences set" (:30-41: every Valid measurement point is appended).  Merged points take
 * all fields of the measurement point, coordinates = mean of both (:66-70); if fewer than
 * target_number_of_merges were merged, the unmerged Valid measurement points are appended
 * (:92-115). */
int srrg2_scene_merge(srrg2_scene_h scene, srrg2_scene_h measurement, const float* measurement_in_scene,
                      const srrg2_correspondence* correspondences, int n_correspondences, const srrg2_merger_params* p,
                      srrg2_merge_result* out);
/* the same, with the correspondences taken on the device from slice `slice_idx` of an aligner
 * whose moving cloud was `clipped` and whose fixed cloud was `measurement`: flipped and mapped
 * to the global scene as TrackerSliceProcessor_::merge() does (S/trackers/
 * tracker_slice_processor_impl.cpp:160-186). */
int srrg2_scene_merge_from_aligner(srrg2_scene_h scene, srrg2_scene_h measurement, const float* measurement_in_scene,
                                   srrg2_aligner_h aligner, int slice_idx, srrg2_scene_h clipped,
                                   const srrg2_merger_params* p, srrg2_merge_result* out);

/* ---- measurement adaptors: raw sensor data -> measurement scene, on the device ---------------------------------
 * The adapt step of MultiTrackerBase_::compute() (S/trackers/multi_tracker_impl.cpp:57-80 ->
 * S/trackers/tracker_slice_processor_base_impl.cpp:32-49 -> RawDataPreprocessor_::compute(),
 * S/raw_data_preprocessors/raw_data_preprocessor.h:13-88).  The reference ships the interface only; the concrete
 * adaptors here are defined from first principles (DESIGN.md section 4 "Measurement adaptors" is the arithmetic contract):
 *   depth image -> PointNormal3f cloud   pinhole unprojection, normals from the cross product of two central differences
 *   laser scan  -> PointNormal2f cloud   polar -> Cartesian, normals from the chord between beams k-w and k+w
 *   lidar sweep -> PointNormal3f cloud   point list -> range image (nearest point per pixel), normals as for the depth image
 * All write straight into a scene (replacing its content like srrg2_scene_set; global indices and descriptors are
 * dropped), so the frame is adapt -> clip -> align -> merge on device handles. */

/* RawDataPreprocessor_::Status, raw_data_preprocessor.h:22 (values identical) */
enum srrg2_adaptor_status { SRRG2_ADAPTOR_READY = 0, SRRG2_ADAPTOR_INITIALIZING = 1, SRRG2_ADAPTOR_ERROR = 2 };
enum srrg2_image_type { SRRG2_IMAGE_NONE = 0, SRRG2_IMAGE_U8 = 1, SRRG2_IMAGE_U16 = 2, SRRG2_IMAGE_F32 = 3 };

typedef struct srrg2_depth_adaptor_params {
  float camera_matrix[9];            /* row-major K; fx, fy finite and non-zero; K[0][1] != 0 -> SRRG2_E_UNSUPPORTED */
  int32_t rows, cols;
  float depth_scale;                 /* metres per count of a U16 image (default 0.001); F32 images are metres */
  float depth_min, depth_max;        /* accepted z, both inclusive */
  int32_t normal_col_gap, normal_row_gap; /* pixels; both 0 = no normals (a scene without normals) */
  float normal_max_distance_squared; /* gate on each of the two difference vectors */
  int32_t drop_points_without_normal; /* default 1: a depth-valid pixel that gets no normal becomes invalid;
                                         0: it stays Valid with a NaN normal */
  int32_t compact;                   /* 0: organised, rows*cols points, invalid = NaN (what the projective finder reads);
                                        1: only the Valid points, in row-major pixel order (nearest-neighbour finder) */
} srrg2_depth_adaptor_params;

typedef struct srrg2_scan_adaptor_params {
  double angle_min, angle_increment; /* bearing of beam k = angle_min + k * angle_increment (radians) */
  float range_min, range_max;        /* accepted range, both inclusive */
  int32_t normal_half_window;        /* w: normal from beams k-w and k+w; 0 = no normals */
  float normal_max_distance_squared; /* gate on the chord p[k+w] - p[k-w] */
  int32_t drop_points_without_normal;
  int32_t compact;
} srrg2_scan_adaptor_params;

typedef struct srrg2_adapt_result {
  int32_t status;       /* srrg2_adaptor_status */
  int32_t num_raw;      /* pixels / beams */
  int32_t num_in_range; /* finite and inside [min, max] */
  int32_t num_valid;    /* points left Valid in dst */
  int32_t scene_size;   /* srrg2_scene_size(dst) afterwards */
} srrg2_adapt_result;

/* defaults: identity-free (camera_matrix / rows / cols / bearings are the caller's); depth_scale 0.001, depth 0.4 .. 8 m,
 * gaps 1 / 1, normal_max_distance_squared 0.0625, drop 1, organised; scan: range 0.05 .. 30 m, half window 1, 0.01, drop 1,
 * organised */
void srrg2_adapt_default_depth_params(srrg2_depth_adaptor_params* p);
void srrg2_adapt_default_scan_params(srrg2_scan_adaptor_params* p);
/* dst: a scene of dim 3.  depth / intensity: images with a row stride in bytes (a multiple of the element size, the pointer
 * aligned to it), both in `mem` = SRRG2_MEM_HOST | SRRG2_MEM_DEVICE.  depth_type: U16 (raw counts, 0 = no reading) or F32
 * (metres).  intensity_type NONE: dst has no features afterwards; U8 / F32: dst gets the intensity feature (the value as
 * float, U8 not rescaled), moved with its point in compact mode.
 *   refused   SRRG2_E_INVALID, dst unchanged: wrong dim, null params, a null image of more than zero pixels, rows or cols
 *             < 0 or rows*cols beyond int32, a gap < 0 or exactly one of the two gaps 0, depth_type NONE / U8, intensity_type
 *             U16, a stride smaller than a row or misaligned, fx or fy zero / not finite, bad mem.
 *   status    an image of zero pixels leaves an empty scene, INITIALIZING; otherwise READY (also when no point is Valid).
 *   compact   srrg2_scene_global_indices(dst) gives every point's pixel index r*cols + c.
 *   waits     organised mode with out == NULL queues its work on the scene's stream and returns: the size (rows*cols) is
 *             known on the host, so srrg2_scene_device_arrays + set_fixed(..., SRRG2_MEM_DEVICE_KEPT) can follow at once
 *             (a SRRG2_MEM_HOST image in pageable memory is consumed before the call returns, as for any upload).
 *             With out != NULL, and always in compact mode, the call returns when dst is complete. */
int srrg2_adapt_depth_image(srrg2_scene_h dst, const void* depth, int depth_type, int depth_row_stride_bytes,
                            const void* intensity, int intensity_type, int intensity_row_stride_bytes, int mem,
                            const srrg2_depth_adaptor_params* p, srrg2_adapt_result* out /* may be NULL */);
/* dst: a scene of dim 2; ranges: num_beams floats (metres), 4-byte aligned.  Refusals, status and waits as above
 * (num_beams < 0, normal_half_window < 0); compact: global indices = beam indices. */
int srrg2_adapt_laser_scan(srrg2_scene_h dst, const float* ranges, int num_beams, int mem,
                           const srrg2_scan_adaptor_params* p, srrg2_adapt_result* out /* may be NULL */);

/* 3-D lidar sweep (a list of n points x, y, z in the sensor frame) -> organised or compact PointNormal3f cloud, through the
 * range image of srrg2_spherical_model (declared with srrg2_scene_clip_spherical; DESIGN.md section 4 "Lidar sweeps").
 *   bin       every point with finite coordinates is projected; of the points of one pixel the nearest wins, of equal ranges
 *             the lowest input index: the result depends on the points alone.
 *   scene     pixel by pixel, as the depth adaptor: an empty pixel is a NaN point; an occupied one stores its winner's input
 *             coordinates verbatim.  Normal: the cross product of the central differences over c +- normal_col_gap (modulo cols
 *             when the columns wrap) and r +- normal_row_gap, all four neighbours occupied and inside the image, each
 *             difference within normal_max_distance_squared, normalised, turned towards the sensor.  Validity,
 *             drop_points_without_normal and compact as srrg2_depth_adaptor_params.
 *   intensity NULL: dst has no features afterwards; else dst gets the intensity feature, the winner's value (an empty pixel
 *             of an organised scene: 0).  intensity = points + 3 with both strides 16 reads interleaved XYZI records.
 *   result    num_raw = n, num_in_range = occupied pixels, num_valid, scene_size; status INITIALIZING when n == 0 (dst is then
 *             an empty scene), else READY.
 *   refused   SRRG2_E_INVALID, dst unchanged: wrong dim, null params, null points with n > 0, n < 0, a stride < 12 (intensity:
 *             < 4) or no multiple of 4, a pointer not 4-byte aligned, bad mem, an invalid model, a gap < 0 or exactly one of
 *             the two gaps 0, reserved != 0.
 *   waits     as srrg2_adapt_depth_image: organised mode with out == NULL queues its work on the scene's stream and returns.
 *             A SRRG2_MEM_HOST cloud is consumed before the call returns.  A SRRG2_MEM_DEVICE cloud must stay untouched until
 *             the next srrg2_scene_* call on dst settles it. */
typedef struct srrg2_lidar_adaptor_params {
  srrg2_spherical_model model;
  int32_t normal_col_gap, normal_row_gap; /* pixels; both 0 = no normals; exactly one 0 = SRRG2_E_INVALID */
  float   normal_max_distance_squared;    /* gate on each of the two difference vectors; default 1.0 (untuned) */
  int32_t drop_points_without_normal;     /* default 1 */
  int32_t compact;                        /* 0: organised rows*cols, empty = NaN; 1: only the Valid points, pixel order */
  int32_t reserved;                       /* 0 */
} srrg2_lidar_adaptor_params;
/* model zeroed except range 0.5 .. 120 m; gaps 1 / 1; normal_max_distance_squared 1.0; drop 1; organised */
void srrg2_adapt_default_lidar_params(srrg2_lidar_adaptor_params* p);
int srrg2_adapt_lidar_sweep(srrg2_scene_h dst /* dim 3 */, const float* points, int point_stride_bytes,
                            const float* intensity /* may be NULL */, int intensity_stride_bytes, int n, int mem,
                            const srrg2_lidar_adaptor_params* p, srrg2_adapt_result* out /* may be NULL */);

/* srrg2_adapt_lidar_sweep for real sensors: a per-ring elevation table and the de-skew of a sweep taken while the sensor moved
 * (DESIGN.md section 4 "Lidar sweeps", contracts 1 and 2).  x == NULL, or the defaults, give srrg2_adapt_lidar_sweep bit for bit.
 *   rings     ring_elevations as in srrg2_scene_clip_spherical_rings (same rows, same refusals; the model's elevation_min /
 *             elevation_increment are then neither read nor validated).  A host table, consumed before the call returns.
 *   de-skew   deskew != 0.  The image stays the sensor's firing grid: every point is projected and binned from its RAW
 *             coordinates (nearest-wins with the raw range); what the scene stores for a winner, what its neighbours lend to a
 *             normal and what turns the normal towards the sensor are the DE-SKEWED coordinates.
 *             time     s = ((double) times[i] - time_begin) / (time_end - time_begin), not clamped: points outside the interval
 *                      are extrapolated; a point whose time is not finite is treated as a point with a non-finite coordinate.
 *                      times == NULL: s = tf / cols, tf the continuous column coordinate of the point's raw projection -- column 0
 *                      is taken as the sweep's start, so the columns a sensor fires again past the seam get SMALL s (they are
 *                      de-skewed as if fired at the start); give per-point times where that matters.
 *             motion   3x4 [R|t], the sensor at s = 1 in the sensor frame at s = 0 (prev^-1 * curr of a constant-velocity
 *                      model).  Constant rotation rate about the fixed axis of R, translation linear in s (not the SE(3) screw):
 *                      q = Rot(axis, s*theta) * p + s*t, out = Rot(axis, reference*theta)^T * (q - reference*t), float64, each
 *                      component rounded to float32 once.  reference = 1 expresses the scene in the sensor frame at the sweep's
 *                      end, 0 at its start.  The result is specified for |s*theta| <= 1e6 rad.
 *   refused   SRRG2_E_INVALID, dst unchanged: whatever srrg2_adapt_lidar_sweep refuses; reserved != 0; a bad ring table; with
 *             deskew: motion or reference not finite; with deskew and times: time_begin or time_end not finite or equal, a
 *             stride < 4 or no multiple of 4, times not 4-byte aligned.  SRRG2_E_UNSUPPORTED: a ring table with rows > 256.
 *   waits     as srrg2_adapt_lidar_sweep; times live in the same `mem` as the points and follow the points' rules. */
typedef struct srrg2_lidar_sweep_extras {
  const double* ring_elevations;  /* HOST, model.rows entries (radians); NULL: the model's uniform rows */
  const float*  times;            /* per point, in the same `mem` as the points; NULL with deskew != 0: time from the raw azimuth */
  int32_t time_stride_bytes;      /* >= 4, multiple of 4 (20 with times = points + 4 reads XYZIT records) */
  int32_t deskew;                 /* 0: off -- times, time_*, reference, motion are not looked at */
  double  time_begin, time_end;   /* the times that mean s = 0 and s = 1; used only when times != NULL */
  double  reference;              /* s of the frame the output is expressed in; default 1 (the sweep's end) */
  float   motion[12];             /* 3x4 [R|t]: the sensor at s = 1 in the sensor frame at s = 0 */
  int32_t reserved[2];            /* 0 */
} srrg2_lidar_sweep_extras;
/* all off: no table, no times, deskew 0, reference 1, motion identity */
void srrg2_adapt_default_lidar_sweep_extras(srrg2_lidar_sweep_extras* x);
int srrg2_adapt_lidar_sweep_ex(srrg2_scene_h dst /* dim 3 */, const float* points, int point_stride_bytes,
                               const float* intensity /* may be NULL */, int intensity_stride_bytes, int n, int mem,
                               const srrg2_lidar_adaptor_params* p, const srrg2_lidar_sweep_extras* x /* NULL = plain */,
                               srrg2_adapt_result* out /* may be NULL */);

/* Image features: an 8-bit intensity image (+ optional depth image) -> a compact scene of keypoints, each with a 3-D point, a
 * 256-bit descriptor and an intensity -- the producer of the PointIntensityDescriptor3f clouds that srrg2_scene_set_features,
 * the merger and srrg2_descriptor_db_add_scene / match_scene carry (S/mapping/merger_correspondence_homo.h:36-40,
 * multi_loop_detector_hbst_impl.cpp:84-85, :131-136).  No reference counterpart; DESIGN.md section 4 "Image features" is the
 * contract, all image arithmetic is integer, tests/features_restatement.py restates it and the library gives the same bits.
 *   score     FAST on the 16-pixel circle of radius 3: the largest t below which 9 contiguous circle pixels are all brighter
 *             than centre + t or all darker than centre - t; 0 within 3 pixels of a border.
 *   maxima    keypoint: score > fast_threshold, at least 16 pixels from every border, score strictly above the 4 of its 8
 *             neighbours that precede it in raster order and not below the 4 that follow.
 *   cap       max_features > 0 and more keypoints than that: those above the cut score s* stay, of those at s* the first in
 *             raster order, max_features in all (256-bin histogram, no sort).  Output order: ascending pixel index.
 *   angle     oriented: the bin k of 32 that maximises m10 * C_k + m01 * S_k (lowest k of equals), m10 / m01 the first moments
 *             of the intensity over the disc of radius 15, C_k / S_k = round(16384 cos / sin (2 pi k / 32)); else bin 0.
 *   bits      bit i = B(a_i) < B(b_i): B the 5x5 box sum, (a_i, b_i) pair i of srrg2_feature_pattern(angle_bin); bit i lies in
 *             byte i / 8, bit i % 8.
 *   point     with a depth image (U16 / F32 as srrg2_adapt_depth_image): a keypoint is kept iff its own depth pixel is in range,
 *             its coordinates are what srrg2_adapt_depth_image stores for that pixel; without (depth NULL, depth_type NONE):
 *             the unprojection at z = 1.  The cap comes before the depth gate.
 *   cam       read: camera_matrix, rows, cols, depth_scale, depth_min, depth_max; the normal and compact fields are not read.
 *   scene     dst (dim 3) holds the kept keypoints in pixel order: no normals, both features (the intensity is the pixel's value
 *             as float), srrg2_scene_global_indices(dst) = pixel indices r*cols + c.  keypoints_out (host) receives up to
 *             keypoint_capacity records in the same order.
 *   refused   SRRG2_E_INVALID, dst unchanged: wrong dim, null params, a null intensity image of more than zero pixels, rows or
 *             cols < 0 or rows*cols beyond int32, a stride smaller than a row, a depth image not aligned to its element, bad
 *             mem, fast_threshold outside 0 .. 254, max_features < 0, oriented not 0 / 1, reserved != 0, keypoint_capacity < 0,
 *             a depth image with depth_type NONE or U8 (or a depth_type without an image), fx or fy zero / not finite.
 *             SRRG2_E_UNSUPPORTED: intensity_type U16 or F32, K[0][1] != 0.
 *   status    zero pixels: an empty scene, INITIALIZING.  Either side below 33 (no admissible pixel): an empty scene, READY.
 *   waits     ONE host wait in the middle, for the number of kept keypoints (it sizes dst); the call returns when dst, and
 *             keypoints_out, are complete.  SRRG2_MEM_HOST images are consumed before the call returns. */
typedef struct srrg2_feature_params {
  int32_t fast_threshold; /* 0 .. 254, default 20 */
  int32_t max_features;   /* 0 = no cap, default 1000 */
  int32_t oriented;       /* 0 | 1, default 1 */
  int32_t reserved;       /* 0 */
} srrg2_feature_params;
typedef struct srrg2_keypoint {
  int32_t pixel, score, angle_bin, reserved;
} srrg2_keypoint;
typedef struct srrg2_feature_result {
  int32_t status;         /* srrg2_adaptor_status */
  int32_t num_pixels;
  int32_t num_candidates; /* score > fast_threshold inside the margin */
  int32_t num_maxima;
  int32_t num_selected;   /* after the cap */
  int32_t num_with_depth;
  int32_t scene_size;
} srrg2_feature_result;
void srrg2_adapt_default_feature_params(srrg2_feature_params* p);
int srrg2_adapt_image_features(srrg2_scene_h dst /* dim 3 */, const void* intensity, int intensity_type /* U8 */,
                               int intensity_row_stride_bytes, const void* depth /* may be NULL */, int depth_type,
                               int depth_row_stride_bytes, int mem, const srrg2_depth_adaptor_params* cam,
                               const srrg2_feature_params* p, srrg2_keypoint* keypoints_out /* host, may be NULL */,
                               int keypoint_capacity, srrg2_feature_result* out /* may be NULL */);
/* the 256 point pairs (ax, ay, bx, by) of orientation bin 0 .. 31, rotated: 1024 values.  Needs no device. */
int srrg2_feature_pattern(int angle_bin, int8_t* pairs_out);

/* Image features over a scale pyramid: srrg2_adapt_image_features on every level of an integer-resampled pyramid of the image,
 * into ONE ordinary feature scene -- a landmark seen from another distance finds its descriptor on another level.  No reference
 * counterpart; DESIGN.md section 4 "Image features: scale pyramid" is the contract, all image arithmetic is integer,
 * tests/pyramid_restatement.py restates it and the library gives the same bits.
 *   levels    level 0 is the caller's image; rows_l = rows_{l-1} * den / num, cols_l = cols_{l-1} * den / num (floor), each level
 *             resampled from the level before it.  The first level with a side <= 32 (no admissible pixel) ends the pyramid: it
 *             and all later levels are not built.
 *   resample  bilinear with 8 fractional bits at pixel centres.  Destination column c: X = ((2c+1) * num * 256) / (2 * den) - 128
 *             (floor; never negative), x0 = min(X >> 8, cols_{l-1} - 1), x1 = min((X >> 8) + 1, cols_{l-1} - 1), fx = X & 255;
 *             rows likewise.  Value: (I00 (256-fx)(256-fy) + I01 fx (256-fy) + I10 (256-fx) fy + I11 fx fy + 32768) >> 16.  A
 *             constant image stays constant; at 2/1 the value is (a + b + c + d + 2) >> 2 of the 2x2 block.  No blur.
 *   per level score, maxima, angle and bits are exactly those of srrg2_adapt_image_features on the level's image (same
 *             thresholds, margin and pattern).
 *   cap       max_features > 0: with A_l = rows_l * cols_l over the built levels, level l keeps at most q_l = max_features * A_l
 *             / sum A (floor, 64 bits), level 0 also the remainder max_features - sum q; inside a level the cap of
 *             srrg2_adapt_image_features.  A quota of 0 keeps nothing on that level.  Unused quota is not handed on.
 *             max_features == 0: no cap on any level.
 *   position  of (r, c) on level l: u_q8 = ((2c+1) * num^l * 128) / den^l - 128 (floor, 64 bits; 256 c at level 0), v_q8 from r;
 *             the nearest level-0 pixel is c0 = min((u_q8 + 128) >> 8, cols_0 - 1), r0 likewise.
 *   point     the depth gate reads depth pixel (r0, c0) with the rule of srrg2_adapt_image_features; the point is
 *             (((u - cx) * (1/fx)) * z, ((v - cy) * (1/fy)) * z, z) with u = (float) u_q8 * (1/256), that call's expression
 *             order, so at level 0 it is that call's point bit for bit.  Without a depth image z = 1.  The cap comes before the depth gate.
 *   scene     dst (dim 3) holds the kept keypoints level-major, in raster order within a level: no normals, both features (the
 *             intensity is the LEVEL image's pixel value as float).  srrg2_scene_global_indices(dst) = `pixel`, the nearest
 *             level-0 pixel: NOT ascending across levels, and the same pixel may appear once per level -- keypoints of different
 *             levels on one corner are all kept (as ORB does), there is no cross-level suppression.  The descriptor database, the
 *             consensus pose, the clippers and the merger take the scene as it is; srrg2_scene_track_features takes it as `moving`
 *             and, as long as dst is as this call left it, as `fixed` (it searches the levels one by one).
 *   refused   (dst unchanged) everything srrg2_adapt_image_features refuses, with its codes; SRRG2_E_INVALID: a null pyr,
 *             num_levels outside 1 .. 8, a ratio outside 1 <= den < num <= 2 den, num <= 8, reserved != 0; SRRG2_E_UNSUPPORTED:
 *             rows or cols above 4194304 (u_q8 / v_q8 would leave int32).
 *   status    as srrg2_adapt_image_features; level 0 with a side below 33: an empty scene, READY, num_levels_built 0.
 *   result    rows / cols / counters per built level (0 beyond); quota[l] = q_l (0 when max_features == 0).
 *   waits     ONE host wait in the middle, for all levels' kept counts together (they size dst and place the levels in it); the
 *             call returns when dst and keypoints_out are complete.  SRRG2_MEM_HOST images are consumed before the call returns.
 *   identity  num_levels = 1: the scene, the counters and the records' first three fields are those of
 *             srrg2_adapt_image_features. */
typedef struct srrg2_pyramid_params {
  int32_t num_levels; /* 1 .. 8, default 4 */
  int32_t scale_num;  /* default 6 */
  int32_t scale_den;  /* default 5;  1 <= den < num <= 2*den, num <= 8 */
  int32_t reserved;   /* 0 */
} srrg2_pyramid_params;
typedef struct srrg2_pyramid_keypoint { /* 32 bytes */
  int32_t pixel;       /* nearest level-0 pixel r0*cols + c0 (also the scene's global index) */
  int32_t score, angle_bin, level;
  int32_t level_pixel; /* r*cols_l + c in the level's own image */
  int32_t u_q8, v_q8;  /* level-0 position of the keypoint's centre, 1/256 pixel */
  int32_t reserved;
} srrg2_pyramid_keypoint;
typedef struct srrg2_pyramid_result {
  int32_t status, num_levels_built, scene_size, reserved;
  int32_t rows[8], cols[8], num_candidates[8], num_maxima[8], num_selected[8], num_with_depth[8], quota[8];
} srrg2_pyramid_result;
void srrg2_adapt_default_pyramid_params(srrg2_pyramid_params* p);
int srrg2_adapt_image_features_pyramid(srrg2_scene_h dst /* dim 3 */, const void* intensity, int intensity_type /* U8 */,
                                       int intensity_row_stride_bytes, const void* depth /* may be NULL */, int depth_type,
                                       int depth_row_stride_bytes, int mem, const srrg2_depth_adaptor_params* cam,
                                       const srrg2_feature_params* p, const srrg2_pyramid_params* pyr,
                                       srrg2_pyramid_keypoint* keypoints_out /* host, may be NULL */, int keypoint_capacity,
                                       srrg2_pyramid_result* out /* may be NULL */);

/* Stereo features: a rectified pair of 8-bit images -> a compact scene of matched, triangulated, described keypoints (the
 * clouds of the reference's stereo pipeline, initializers/initializer_camera.h InitializerStereoCamera_).  No reference
 * counterpart; DESIGN.md section 4 "Stereo features" is the contract, tests/stereo_restatement.py restates it and the library
 * gives the same bits.
 *   extract   each image alone goes through score, maxima, cap, angle and bits of srrg2_adapt_image_features with fp.  cam: rows,
 *             cols, camera_matrix, depth_min, depth_max are read; both images have that shape and lie in `mem`.
 *   candidates  of a left keypoint (r, cl): the right keypoints (rr, cr) with |rr - r| <= row_tolerance and d = cl - cr in
 *             [min_disparity, max_disparity].
 *   best      the candidate of smallest (Hamming distance h, right pixel index rr*cols + cr); accepted iff h <= max_distance.
 *   cross     cross_check: the same rule from the right (candidates: left keypoints in the band with d in range, smallest
 *             (h, left pixel index)); a left keypoint stays iff its best right keypoint's best is that left keypoint.
 *   subpixel  integer costs cost(k) = sum over the 7x7 window of |L(r+dy, cl+dx) - R(rr+dy, cr+k+dx)|, k = -1, 0, 1;
 *             D = cost(-1) - 2 cost(0) + cost(1); cost(0) <= both neighbours and D > 0: off = (float)(cost(-1) - cost(1)) /
 *             (float)(2 D), else 0; disparity = (float) d - off.  subpixel 0: disparity = (float) d.
 *   point     z = (fx * baseline) / disparity in float32; kept iff z is finite and depth_min <= z <= depth_max; the coordinates
 *             are those of srrg2_adapt_image_features for the left pixel under an F32 depth image holding z there.
 *   scene     dst (dim 3): the kept left keypoints in left pixel order, no normals, the left descriptor and the left pixel's
 *             intensity as features, srrg2_scene_global_indices(dst) = left pixel indices.  keypoints_out / matches_out (host,
 *             may be NULL) receive up to their capacity of records in the same order.
 *   refused   what srrg2_adapt_image_features refuses for either image, with its codes; SRRG2_E_INVALID: a null sp, baseline
 *             not finite or <= 0, min_disparity < 1, max_disparity < min_disparity, row_tolerance outside 0 .. 8, max_distance
 *             outside 0 .. 256, cross_check or subpixel not 0 / 1, reserved != 0, a negative capacity.  dst is unchanged.
 *   status    zero pixels: an empty scene, INITIALIZING.  Either side below 33: an empty scene, READY.
 *   waits     TWO host waits in the middle: for both images' keypoint counts (both pipelines are queued before it) and for the
 *             number of kept keypoints (it sizes dst); the call returns when dst and the records are complete.
 * max_distance 48 and max_disparity 128 are UNTUNED defaults: nobody has derived or measured them. */
typedef struct srrg2_stereo_params {
  float baseline;        /* metres, finite, > 0: the right camera sits at +baseline along the left camera's x axis */
  int32_t min_disparity; /* >= 1, default 1 */
  int32_t max_disparity; /* >= min_disparity, default 128 (untuned) */
  int32_t row_tolerance; /* 0 .. 8, default 1: |row_right - row_left| allowed (rectified pair) */
  int32_t max_distance;  /* 0 .. 256, default 48 (untuned): largest accepted Hamming distance */
  int32_t cross_check;   /* 0 | 1, default 1 */
  int32_t subpixel;      /* 0 | 1, default 1 */
  int32_t reserved;      /* 0 */
} srrg2_stereo_params;
typedef struct srrg2_stereo_match {
  int32_t left_pixel, right_pixel, distance;
  float disparity;
} srrg2_stereo_match;
typedef struct srrg2_stereo_result {
  int32_t status;       /* srrg2_adaptor_status */
  int32_t num_pixels;
  int32_t num_left;     /* keypoints selected (after the cap) in the left image */
  int32_t num_right;    /* ... in the right image */
  int32_t num_matched;  /* left keypoints with a best right candidate inside all three gates */
  int32_t num_mutual;   /* ... that survive the cross check (= num_matched when it is off) */
  int32_t num_in_range; /* ... whose z lies in [depth_min, depth_max] */
  int32_t scene_size;
} srrg2_stereo_result;
/* baseline 0 (the caller must set it), disparity 1 .. 128, row_tolerance 1, max_distance 48, cross_check 1, subpixel 1 */
void srrg2_adapt_default_stereo_params(srrg2_stereo_params* p);
int srrg2_adapt_stereo_features(srrg2_scene_h dst /* dim 3 */, const void* left, int left_row_stride_bytes, const void* right,
                                int right_row_stride_bytes, int mem, const srrg2_depth_adaptor_params* cam,
                                const srrg2_feature_params* fp, const srrg2_stereo_params* sp,
                                srrg2_keypoint* keypoints_out /* host, may be NULL */, int keypoint_capacity,
                                srrg2_stereo_match* matches_out /* host, may be NULL */, int match_capacity,
                                srrg2_stereo_result* out /* may be NULL */);

/* Dense stereo: a rectified pair of 8-bit images -> a disparity for every pixel that earns one -> depth -> the scene
 * srrg2_adapt_depth_image leaves for that depth image with the left image as its intensity, without leaving the device.  No
 * reference counterpart; DESIGN.md section 4 "Dense stereo" is the contract, tests/stereo_dense_restatement.py restates it and
 * the library gives the same bits.  cam: rows, cols (both images have that shape and lie in `mem`) and everything the depth
 * adaptor reads.  The right camera sits at +baseline along the left camera's x axis.
 *   census    62 bits per pixel with 3 <= r < rows-3, 4 <= c < cols-4: one per (dy, dx) in [-3,3] x [-4,4] but (0,0), set iff
 *             I(r+dy, c+dx) < I(r, c).
 *   rectangle rows 3 .. rows-4, columns 4 + max_disparity .. cols-5: every disparity of the range is defined for each of its
 *             pixels; pixels outside never get a disparity.  Empty (rows < 7 or cols < max_disparity + 9): no disparities, READY.
 *   cost      C(p, d) = popcount(censusL(r, c) ^ censusR(r, c-d)), 0 .. 62.
 *   paths     4: for e in (0,+1), (0,-1), (+1,0), (-1,0): L_e(p,d) = C(p,d) when p-e lies outside the rectangle, else C(p,d) +
 *             min(L_e(p-e,d), L_e(p-e,d-1)+p1, L_e(p-e,d+1)+p1, M+p2) - M with M = min_k L_e(p-e,k), terms beyond the range
 *             omitted; S = sum of the four.  0: S = C.
 *   best      d* = argmin_d S(p,d), the smallest d on ties.
 *   unique    uniqueness_ratio u > 0: with S2 the minimum of S over |d - d*| > 1, the pixel passes iff there is no such d or
 *             S2 (100-u) > 100 S(p,d*) (strict: a flat image is rejected everywhere).
 *   lr_check  dR(r,x) = argmin over d with (r, x+d) in the rectangle of S((r,x+d), d), the smallest d on ties -- the left
 *             volume read along its diagonal; the pixel passes iff |dR(r, c-d*) - d*| <= lr_tolerance.
 *   subpixel  for min < d* < max, with a = S(d*-1), b = S(d*), cc = S(d*+1), D = a - 2b + cc > 0:
 *             disparity = (float) d* + (float)(a - cc) / (float)(2 D); otherwise (float) d*.
 *   scene     Z = (fx * baseline) / disparity in float32, NaN without a disparity; dst is bit for bit what
 *             srrg2_adapt_depth_image(dst, Z, F32, ..., left, U8, ..., cam, ...) leaves (the same code runs).
 *   disparity_out  rows x cols floats in `mem` (may be NULL), 0.0f where there is no disparity; bytes between rows are not written.
 *   refused   dst and disparity_out untouched, nothing read from the images.  Everything srrg2_adapt_depth_image refuses for
 *             cam, the images' strides and mem, with its codes.  SRRG2_E_INVALID: a null sp, baseline not finite or <= 0,
 *             min_disparity < 1, max_disparity < min_disparity, paths not 0 / 4, not 0 <= p1 <= p2 <= 255, uniqueness_ratio
 *             outside 0 .. 99, lr_check or subpixel not 0 / 1, lr_tolerance outside 0 .. 16, reserved != 0, dst and
 *             disparity_out both NULL, a disparity stride below 4 cols or no multiple of 4 (or a misaligned disparity_out).
 *             SRRG2_E_UNSUPPORTED: more than 256 disparities, a volume of more than 2^31 - 1 elements.
 *   status    zero pixels: an empty scene, INITIALIZING; otherwise READY.
 *   waits     none in the middle: every size follows from the shapes.  Organised mode, out == NULL and disparity_out NULL or in
 *             device memory: the call queues its work on the scene's stream and returns, like the depth adaptor.  Otherwise ONE
 *             wait at the end (compact mode: the depth adaptor's own wait for the scene's size comes before it).  dst == NULL:
 *             the call works on a scene of its own on the current device and returns when that scene has retired.
 * p1 8, p2 48 and uniqueness_ratio 10 are UNTUNED defaults: nobody has derived or measured them. */
typedef struct srrg2_dense_stereo_params {
  float   baseline;         /* metres, finite, > 0 (default 0: the caller must set it) */
  int32_t min_disparity;    /* >= 1, default 1 */
  int32_t max_disparity;    /* >= min_disparity; max - min + 1 <= 256 (else SRRG2_E_UNSUPPORTED); default 64 */
  int32_t paths;            /* 0: per-pixel census cost only; 4: aggregation along the four axis directions; default 4 */
  int32_t p1, p2;           /* 0 <= p1 <= p2 <= 255; defaults 8 / 48 (untuned) */
  int32_t uniqueness_ratio; /* 0 .. 99 per cent, 0 = no test; default 10 (untuned) */
  int32_t lr_check;         /* 0 | 1, default 1 */
  int32_t lr_tolerance;     /* 0 .. 16, default 1 */
  int32_t subpixel;         /* 0 | 1, default 1 */
  int32_t reserved;         /* 0 */
} srrg2_dense_stereo_params;
typedef struct srrg2_dense_stereo_result {
  int32_t status;           /* srrg2_adaptor_status */
  int32_t num_pixels;       /* rows * cols */
  int32_t num_evaluated;    /* pixels of the processed rectangle */
  int32_t num_unique;       /* ... that pass the uniqueness test */
  int32_t num_consistent;   /* ... and the left-right check: the pixels that carry a disparity */
  int32_t num_in_range, num_valid, scene_size; /* srrg2_adapt_result's, 0 when dst is NULL */
} srrg2_dense_stereo_result;
void srrg2_adapt_default_dense_stereo_params(srrg2_dense_stereo_params* p);
int srrg2_adapt_stereo_dense(srrg2_scene_h dst /* dim 3; may be NULL if disparity_out is not */, const void* left,
                             int left_row_stride_bytes, const void* right, int right_row_stride_bytes, int mem,
                             const srrg2_depth_adaptor_params* cam, const srrg2_dense_stereo_params* sp,
                             float* disparity_out /* rows x cols, in `mem`, may be NULL */, int disparity_row_stride_bytes,
                             srrg2_dense_stereo_result* out /* may be NULL */);

/* Rectification: lens undistortion and stereo rectification of raw images on the device -- the stage in front of the image
 * adaptors above, which all assume an ideal pinhole image (the stereo calls: a rectified pair).  No reference counterpart;
 * DESIGN.md section 4 "Rectification" is the contract, tests/rectify_restatement.py restates it and the library gives the same
 * bits.  A rectifier holds one camera and one target: a map with one entry per pixel of the target, built on the device.
 *   model     float64 throughout.  Pixel (r, c) of the target, integer coordinates being pixel centres:
 *               x = (c - cx') / fx', y = (r - cy') / fy';  (X, Y, W) = R^T (x, y, 1), each as (a x + b y) + c;
 *               xn = X / W, yn = Y / W;  r2 = xn xn + yn yn;
 *               num = 1 + r2 (k1 + r2 (k2 + r2 k3)), den = 1 + r2 (k4 + r2 (k5 + r2 k6)), rad = num / den;  xy = xn yn;
 *               xd = xn rad + ((2 p1) xy + p2 (r2 + 2 (xn xn))),  yd = yn rad + (p1 (r2 + 2 (yn yn)) + (2 p2) xy);
 *               u = fx xd + cx, v = fy yd + cy;  U = floor(u 256 + 0.5), V = floor(v 256 + 0.5)
 *             (Brown-Conrady with the rational denominator, OpenCV's order of the coefficients; R: X_rect = R X_src).
 *   map       entry (U, V), int32 with 8 fractional bits, valid iff W > 0, den > 0, u and v finite, 0 <= U <= 256 (src_cols - 1)
 *             and 0 <= V <= 256 (src_rows - 1); otherwise both words are INT32_MIN.
 *   U8        bilinear, the pyramid's formula: x0 = U >> 8, x1 = min(x0 + 1, src_cols - 1), fx = U & 255, rows likewise;
 *             (I00 (256-fx)(256-fy) + I01 fx (256-fy) + I10 (256-fx) fy + I11 fx fy + 32768) >> 16.  Invalid entry: `border`.
 *   U16, F32  depth images, never blended: the pixel ((V + 128) >> 8, (U + 128) >> 8) copied bit for bit (NaN payloads
 *             survive).  Invalid entry: 0 (U16), the quiet NaN 0x7fc00000 (F32).  A rotation that is not exactly the identity:
 *             SRRG2_E_UNSUPPORTED (z along the optical axis would change).
 *   dst       dst_rows x dst_cols at its stride; bytes between rows are never written.  Zero pixels: accepted, nothing written.
 *   waits     order_on != NULL and dst in device memory: the work is queued on that scene's stream and the call returns; a
 *             following srrg2_adapt_* on that scene with SRRG2_MEM_DEVICE images is ordered behind it (a pageable host source
 *             is consumed before the call returns, as for any upload).  order_on == NULL, or a host destination: the work runs on
 *             the rectifier's stream and the call returns when dst is complete.  srrg2_rectifier_destroy (and _set) wait for
 *             work queued with the handle's map.
 *   refused   dst untouched, nothing read from src.  SRRG2_E_INVALID: a null handle, params or image of more than zero pixels;
 *             a handle without srrg2_rectifier_set; a shape < 0 or rows*cols beyond int32; a stride below a row or misaligned (or
 *             such a pointer); bad mem or type; border outside 0 .. 255; fx, fy, fx', fy' zero; any parameter that is not
 *             finite; order_on on another device; the pair: targets of different shape, one handle twice.  SRRG2_E_UNSUPPORTED:
 *             skew in either camera matrix; a source side above 4194304 (U would leave int32); U16 / F32 under a rotation.
 *             srrg2_rectifier_set checks its parameters before its handle.
 * Not built: the fisheye (equidistant) model -- it needs atan, which is not bit-reproducible between hosts and the device; the
 * scaled / cropped target of OpenCV's alpha (pass any new_camera_matrix instead). */
typedef struct srrg2_rectifier_s* srrg2_rectifier_h;
typedef struct srrg2_rectifier_params {
  double  camera_matrix[9];     /* row-major K of the source: fx, fy finite and non-zero; K[0][1] != 0 -> SRRG2_E_UNSUPPORTED */
  double  distortion[8];        /* k1, k2, p1, p2, k3, k4, k5, k6; all zero = none */
  double  rotation[9];          /* row-major R, X_rect = R X_src; identity = plain undistortion */
  double  new_camera_matrix[9]; /* row-major K' of the target: fx', fy', cx', cy' as above */
  int32_t src_rows, src_cols, dst_rows, dst_cols;
} srrg2_rectifier_params;
typedef struct srrg2_rectifier_info {
  int32_t num_pixels;           /* dst_rows * dst_cols */
  int32_t num_valid;            /* entries that are valid */
  int32_t first_row, last_row;  /* the first and last target row, and */
  int32_t first_col, last_col;  /* column, that hold a valid entry; -1 when none does */
} srrg2_rectifier_info;
/* a rectifier on `device`: its own non-blocking stream, its map in device memory */
int srrg2_rectifier_create(int device, srrg2_rectifier_h* out);
int srrg2_rectifier_destroy(srrg2_rectifier_h h);
/* zeros, identity rotation */
void srrg2_rectifier_default_params(srrg2_rectifier_params* p);
/* builds the map on the device (one thread per target pixel); one wait */
int srrg2_rectifier_set(srrg2_rectifier_h h, const srrg2_rectifier_params* p, srrg2_rectifier_info* info_out /* may be NULL */);
/* the map on the host: dst_rows x dst_cols entries (U, V), row-major; capacity in int32 words */
int srrg2_rectifier_get_map(srrg2_rectifier_h h, int32_t* uv_out, int64_t capacity);
/* writes the target's camera matrix (as float), dst_rows and dst_cols into an adaptor's params; nothing else of them */
int srrg2_rectifier_camera(srrg2_rectifier_h h, srrg2_depth_adaptor_params* cam);
/* src: src_rows x src_cols of `type` (srrg2_image_type) in src_mem; dst: dst_rows x dst_cols of the same type in dst_mem */
int srrg2_rectify_image(srrg2_rectifier_h h, srrg2_scene_h order_on /* may be NULL */, const void* src, int type,
                        int src_row_stride_bytes, int src_mem, void* dst, int dst_row_stride_bytes, int dst_mem,
                        int border /* 0 .. 255, U8 only */);
/* both U8 images of a stereo pair in ONE launch; the two targets have one shape (the sources need not) */
int srrg2_rectify_pair(srrg2_rectifier_h left_h, srrg2_rectifier_h right_h, srrg2_scene_h order_on /* may be NULL */,
                       const void* left, int left_row_stride_bytes, const void* right, int right_row_stride_bytes, int mem,
                       void* dst_left, int dst_left_row_stride_bytes, void* dst_right, int dst_right_row_stride_bytes,
                       int dst_mem, int border);
/* Stereo calibration -> the two rectifying rotations; host only, float64, + - * / sqrt alone (bit for bit against the
 * restatement).  KL, KR: row-major camera matrices; R, t: X_right = R X_left + t.
 *   c = -R^T t (the right camera's centre in the left frame), baseline = |c|, e1 = c / |c|;
 *   zm = ((0,0,1) + row 3 of R) / 2;  e2 = (zm x e1) / |zm x e1|;  e3 = e1 x e2;  R1 = rows e1, e2, e3;  R2 = R1 R^T;
 *   Knew: fx' = fy' = (fyL + fyR) / 2, cx' = (cxL + cxR) / 2, cy' = (cyL + cyR) / 2.
 * The right camera then sits at +baseline along the rectified x axis, the convention of srrg2_adapt_stereo_dense.  Sums of
 * three products are (a + b) + c.  |c| = 0 or |zm x e1| = 0 (or an input that is not finite): SRRG2_E_INVALID.  Every output
 * may be NULL. */
int srrg2_stereo_rectify(const double* KL /* 9 */, const double* KR /* 9 */, const double* R /* 9 */, const double* t /* 3 */,
                         double* R1_out /* 9 */, double* R2_out /* 9 */, double* Knew_out /* 9 */, double* baseline_out);

/* Occupancy grid: laser scans and the poses they were taken from -> which cells of a 2-D grid are free, occupied or never seen,
 * on the device -- the map product of the 2-D laser pipeline (adapt_laser_scan, clip_scan, the aligner, merge, the SE(2) pose
 * graph).  No reference counterpart; DESIGN.md section 4 "Occupancy grid" is the contract, tests/gridmap_restatement.py restates
 * it and the library gives the same bits: behind the beam's end point everything is integer.
 *   grid      cols x rows cells of `resolution` metres; origin = world position of the corner of cell (0, 0); cell (ix, iy) lives
 *             at plane index iy*cols + ix, its centre is (ox + ((float) ix + 0.5f) res, oy + ((float) iy + 0.5f) res) in float32.
 *             The state is two int32 planes, hits and misses.
 *   beam      beam k with range r: the sensor-frame point b of srrg2_adapt_laser_scan (bearing angle_min + k angle_increment in
 *             float64, dm::sincos, (float) c * r, (float) s * r); T = dm::se2_compose(robot_in_world, sensor_in_robot); end point
 *             (T0 bx + T1 by) + T2, (T3 bx + T4 by) + T5 in float32; the ray starts at (T2, T5).
 *   cell      u = floorf((x - ox) / resolution) in float32, ix = (int) u; likewise iy.  A u that is NaN or outside
 *             [-2^30, 2^30) is never converted: a beam with such a start or end cell adds nothing (sides are at most 32768 and
 *             rays at most 32767 cells, so such a beam is nowhere near the grid).
 *   ray       (x0, y0) -> (x1, y1), dx = x1 - x0, dy = y1 - y0, n = max(|dx|, |dy|); step i = 0 .. n is the cell
 *             (x0 + sgn(dx) ((2 i |dx| + n) / (2 n)), y0 + sgn(dy) ((2 i |dy| + n) / (2 n))), integer division, 32-bit (n <= 32767
 *             keeps 2 n^2 + n inside int32; a beam with n > 32767 -- no rigid pose gives one -- adds nothing).  Steps 0 .. n-1
 *             add `weight` to misses, step n adds `weight` to hits and not to misses; n = 0 is a hit in the sensor's own cell.
 *             A cell outside the grid is skipped on its own: the ray may start outside, leave and re-enter.
 *   classes   a finite range inside [range_min, range_max]: a return, traced as above.  A range above range_max (+inf too):
 *             clear_beyond_max = 1 traces steps 0 .. n-1 towards the point at range_max as misses, no hit ("cleared only");
 *             = 0 skips the beam.  NaN, -inf, <= 0 or below range_min: skipped.
 *   counts    per beam, not per scan: a cell crossed by 300 beams of one scan gets 300 misses.  Integer adds commute: the
 *             planes do not depend on scheduling, scan order or batch split, and a batch with weight +1 followed by the same
 *             batch with -1 restores them bit for bit (take a scan out, put it back at its optimised pose).  No saturation: an
 *             int32 plane wraps after 2^31 adds to one cell, about 2^31 / num_beams scans through it (1.9 million of 1 081 beams).
 *   result    num_beams_total = num_scans * num_beams = num_returns + num_cleared_only + num_skipped (the classes above, whatever
 *             the geometry); num_hits_in_grid / num_miss_updates: the adds this call made to the two planes.
 *   render    per cell n = hits + misses: n < max(min_observations, 1), or a negative hits or misses (only a removal that was
 *             never integrated leaves one): 255 = unknown; else (100 hits + n / 2) / n in 64-bit integers, 0 .. 100.
 *   to_scene  every cell that renders into [occupied_percent, 100] becomes a point at its centre in a 2-D scene, in plane-index
 *             order, without normals or features; srrg2_scene_global_indices(dst) gives the plane indices.  The scene aligns
 *             like any other (set_fixed of its device arrays): scan-to-map tracking, relocalisation.
 *   waits     every call runs on the grid's stream, in order.  srrg2_gridmap_integrate_scans with out == NULL only queues and
 *             returns (host `ranges` / poses are consumed before it returns; device ones must stay untouched until a later call
 *             of this handle has waited); with `out` it waits once.  The other calls return when their output is complete.
 *   refused   every destination and the planes unchanged.  SRRG2_E_INVALID: a null handle, params or (where there is data) data
 *             pointer; a handle without srrg2_gridmap_reset; rows or cols outside 0 .. 32768; a resolution that is not finite or
 *             <= 0; an origin or sensor_in_robot that is not finite; num_scans or num_beams < 0; bad mem; a weight other than +1 /
 *             -1; clear_beyond_max other than 0 / 1; the scan-model refusals of srrg2_scene_clip_scan (increment zero or not
 *             finite, |angle_min| > 2 pi, |angle_increment| * num_beams beyond 2 pi plus one increment, !(range_min > 0),
 *             !(range_max >= range_min)), except that num_beams = 0 is accepted; range_max / resolution (float32) beyond 32000 or
 *             NaN; occupied_percent outside 0 .. 100; a stride below a row; a `dst` scene that is not 2-D or lives on another
 *             device.  SRRG2_E_UNSUPPORTED: num_scans * num_beams beyond int32.  Parameters are checked before the handle.
 *             num_scans = 0, num_beams = 0 and rows * cols = 0 are accepted and do nothing. */
typedef struct srrg2_gridmap_s* srrg2_gridmap_h;
typedef struct srrg2_gridmap_params {
  int32_t rows, cols;   /* 0 .. 32768 each */
  float   resolution;   /* metres per cell */
  float   origin[2];    /* world position of the corner of cell (0, 0) */
} srrg2_gridmap_params;
typedef struct srrg2_gridmap_scan_params {
  double  angle_min, angle_increment;   /* as srrg2_scan_adaptor_params: bearing of beam k = angle_min + k*angle_increment */
  int32_t num_beams;
  float   range_min, range_max;         /* a return lies inside, both inclusive */
  float   sensor_in_robot[9];           /* SE(2), row-major 3x3 */
  int32_t clear_beyond_max;             /* 1: a range above range_max clears the ray up to range_max; 0: it is skipped */
} srrg2_gridmap_scan_params;
typedef struct srrg2_gridmap_result {
  int64_t num_beams_total, num_returns, num_cleared_only, num_skipped;
  int64_t num_hits_in_grid, num_miss_updates;
} srrg2_gridmap_result;
/* a grid on `device`: its own non-blocking stream, its planes in device memory */
int srrg2_gridmap_create(int device, srrg2_gridmap_h* out);
int srrg2_gridmap_destroy(srrg2_gridmap_h h);
/* an empty grid (rows = cols = 0) of 0.05 m cells at the origin */
void srrg2_gridmap_default_params(srrg2_gridmap_params* p);
/* identity sensor, range 0.05 .. 30 m (the scan adaptor's), clear_beyond_max = 1; bearings / num_beams (0) are the caller's */
void srrg2_gridmap_default_scan_params(srrg2_gridmap_scan_params* p);
/* allocates and zeroes both planes */
int srrg2_gridmap_reset(srrg2_gridmap_h h, const srrg2_gridmap_params* p);
/* ranges: num_scans x num_beams floats, robot_in_world: num_scans x 9 floats (SE(2), row-major), both in `mem` = SRRG2_MEM_HOST |
 * SRRG2_MEM_DEVICE.  One upload, one kernel, whatever num_scans and num_beams are. */
int srrg2_gridmap_integrate_scans(srrg2_gridmap_h h, const float* ranges, int num_scans, const float* robot_in_world, int mem,
                                  const srrg2_gridmap_scan_params* p, int weight /* +1 | -1 */,
                                  srrg2_gridmap_result* out /* may be NULL: queue only */);
/* rows*cols words each, to `mem`; either pointer may be NULL */
int srrg2_gridmap_get_counts(srrg2_gridmap_h h, int32_t* hits, int32_t* misses, int mem);
/* the planes in device memory (valid until the next reset or destroy); waits for the grid's stream, as srrg2_scene_device_arrays */
int srrg2_gridmap_device_arrays(srrg2_gridmap_h h, const int32_t** hits, const int32_t** misses);
/* rows x cols bytes (0 .. 100, 255 = unknown) to dst in `mem`; bytes between rows are never written */
int srrg2_gridmap_render(srrg2_gridmap_h h, int min_observations, uint8_t* dst, int row_stride_bytes, int mem);
int srrg2_gridmap_to_scene(srrg2_gridmap_h h, int min_observations, int occupied_percent /* 0 .. 100 */, srrg2_scene_h dst);

/* Correlative scan matching against the grid: a pose for a scan whose guess is too far off for ICP (Olson 2009) -- every pose of
 * a window (x, y, theta) around the guess is scored against a smoothed likelihood field of the map, the best one wins.  No
 * reference counterpart; DESIGN.md section 4 "Correlative scan matching" is the contract, tests/scan_match_restatement.py restates
 * it and the library gives the same bits: behind a beam's end cell everything is integer.
 *   field     a third plane of the grid, rows x cols bytes.  A cell is occupied when srrg2_gridmap_render(min_observations)
 *             gives it a value in [occupied_percent, 100] (unknown, 255, is not occupied).  field(c) = the maximum of
 *             lut[dx^2 + dy^2] over the occupied cells c + (dx, dy) inside the grid with dx^2 + dy^2 <= R^2, 0 if there is none.
 *             lut: R^2 + 1 bytes of the caller's in host memory; it need not be monotone, the maximum decides.  R = 0 .. 16.
 *             srrg2_gridmap_default_likelihood_lut: lut[d2] = (255 (R^2 + 1 - d2)) / (R^2 + 1), integer division.
 *   fresh     srrg2_gridmap_reset and every accepted srrg2_gridmap_integrate_scans (one that adds nothing too) make the field
 *             stale; srrg2_gridmap_get_likelihood and srrg2_gridmap_match_scans refuse a stale or never-built field
 *             (SRRG2_E_INVALID, "stale"): build it again.
 *   window    candidates (j, dy, dx), j in [-half_steps_theta, half_steps_theta], dy in [-half_window_y, half_window_y], dx in
 *             [-half_window_x, half_window_x]; flat index ((j + ht) Ny + (dy + wy)) Nx + (dx + wx), Ny = 2 wy + 1, Nx = 2 wx + 1.
 *   rotation  Rj = the SE(2) matrix of dm::sincos((double) j * theta_step) (0 when half_steps_theta = 0), float64 rounded to
 *             float32; Pj = dm::se2_compose(guess, Rj); T = dm::se2_compose(Pj, sensor_in_robot).
 *   beams     only returns (a finite range inside [range_min, range_max]) are scored, and at rotation j only those the grid
 *             would trace from T: the end cell (x1, y1) is the one srrg2_gridmap_integrate_scans adds its hit to (the same
 *             float32 expressions, divide and floorf; start and end inside the 2^30 guard, a ray of at most 32767 cells).
 *   score     of (j, dy, dx): the int32 sum over those beams of field(x1 + dx, y1 + dy), 0 for a cell outside the grid -- the
 *             translation is a shift of whole cells.  At most 255 num_beams.
 *   best      the highest score; among equals the guess (0, 0, 0) if it is one of them, else the lowest flat index.  A scan
 *             without returns, an empty field or an empty grid hand the guess back; nothing depends on scheduling.
 *   result    robot_in_world = Pj with (float) dx * resolution added to entry 2 and (float) dy * resolution to entry 5 (float32);
 *             dx, dy, jtheta; score, score_at_guess; num_scored_beams = the returns of the scan (whatever the rotation: an
 *             upper bound of the beams summed at the winning one, so score <= 255 num_scored_beams).
 *   volume    scores_out, if not NULL: num_scans * Ntheta * Ny * Nx int32 in flat-index order, to scores_mem.
 *   effort    one upload, one host wait, and a launch count that depends neither on num_scans nor on the window.
 *   refused   every destination, the planes and the field unchanged; parameters are checked before the handle.
 *             SRRG2_E_INVALID: R outside 0 .. 16; occupied_percent outside 0 .. 100; a null lut; a null destination; a stride
 *             below a row; bad mem; a negative half window or half_steps_theta; with half_steps_theta > 0 a theta_step that is
 *             not finite or not > 0; null results with num_scans > 0; null or misaligned guesses with num_scans > 0 (whatever
 *             num_beams is: the guesses are always read, ranges only when there are beams); a misaligned scores_out; everything
 *             srrg2_gridmap_integrate_scans refuses of ranges, poses and the scan model; a stale field.  SRRG2_E_UNSUPPORTED:
 *             Ntheta * Ny * Nx beyond int32; with scores_out, num_scans * Ntheta * Ny * Nx beyond int32.  num_scans = 0 writes
 *             nothing; num_beams = 0 and an empty grid score 0 everywhere. */
typedef struct srrg2_gridmap_match_params {
  int32_t half_window_x, half_window_y;   /* cells, >= 0 */
  int32_t half_steps_theta;               /* >= 0 */
  int32_t reserved;                       /* 0 */
  double  theta_step;                     /* radians per step */
} srrg2_gridmap_match_params;
typedef struct srrg2_gridmap_match_result {
  float   robot_in_world[9];              /* SE(2), row-major 3x3 */
  int32_t dx, dy, jtheta;
  int32_t score, score_at_guess, num_scored_beams;
} srrg2_gridmap_match_result;
/* R*R + 1 bytes */
int srrg2_gridmap_default_likelihood_lut(int radius_cells, uint8_t* lut);
int srrg2_gridmap_build_likelihood(srrg2_gridmap_h h, int min_observations, int occupied_percent, int radius_cells, const uint8_t* lut);
/* rows x cols bytes to dst in `mem`; the stride as in srrg2_gridmap_render */
int srrg2_gridmap_get_likelihood(srrg2_gridmap_h h, uint8_t* dst, int row_stride_bytes, int mem);
/* ranges: num_scans x num_beams floats, guess_robot_in_world: num_scans x 9 floats, both in `mem`; results: num_scans structs in
 * host memory; scores_out: NULL or the volume in `scores_mem` */
int srrg2_gridmap_match_scans(srrg2_gridmap_h h, const float* ranges, int num_scans, const float* guess_robot_in_world, int mem,
                              const srrg2_gridmap_scan_params* scan_params, const srrg2_gridmap_match_params* match_params,
                              srrg2_gridmap_match_result* results, int32_t* scores_out, int scores_mem);

/* Pruned scan matching: the window of srrg2_gridmap_match_scans searched through a pyramid of upper bounds, so that a scan with
 * no usable guess can be placed against the whole map (relocalisation, a 2-D loop closure against the map).  The result is bit
 * for bit that of srrg2_gridmap_match_scans on the same inputs, ties included.  DESIGN.md section 4 "Pruned scan matching" is the
 * contract, tests/scan_match_pruned_restatement.py restates it; everything behind a beam's end cell is integer.
 *   planes    levels l = 1 .. L <= 6, a block of level l has side s = 2^l.  P_l(x, y) = the maximum of the field over the cells
 *             [x, x + s) x [y, y + s) inside the grid, 0 if there is none: defined for x in [-(s - 1), cols - 1] and y in
 *             [-(s - 1), rows - 1], 0 elsewhere; P_0 is the field and P_l a 2 x 2 maximum of P_(l-1) at offset s / 2.
 *             srrg2_gridmap_build_bounds builds P_1 .. P_num_levels from a fresh field (a stale one is refused);
 *             srrg2_gridmap_get_bounds hands out the (rows + s - 1) x (cols + s - 1) bytes of one level, row (y + s - 1), column
 *             (x + s - 1), to dst in `mem` (the stride as in srrg2_gridmap_render).  srrg2_gridmap_reset, every accepted
 *             srrg2_gridmap_integrate_scans and srrg2_gridmap_build_likelihood make the planes stale.
 *   blocks    window, rotations, scored beams, end cells (x1, y1) and flat candidate index are those of srrg2_gridmap_match_scans.
 *             At level l the Nx x Ny shifts are tiled by NBx x NBy blocks, NBx = ceil(Nx / s); block (j, by, bx) covers the shift
 *             indices [bx s, bx s + s) x [by s, by s + s) inside the window, its flat index is (j NBy + by) NBx + bx, its bound
 *             U_l = the sum of P_l(x1 + bx s - wx, y1 + by s - wy) over the beams scored at rotation j whose end cell some shift
 *             of the window brings inside the grid.  U_l >= the score of every candidate of the block, and U_(l+1) of the
 *             parent >= U_l of the child.
 *   search    per scan.  Every block of level L is bounded; the seed block is the one with the highest bound, among equals the
 *             lowest flat block index.  The guess and every candidate of the seed block are scored; floor = the highest of these
 *             scores, fixed from here on.  A block survives iff U >= floor, and iff U > floor when floor = score_at_guess (then
 *             nothing beats the guess under the tie rule).  Level by level, the children inside the window of a level's survivors
 *             are evaluated: bounds above level 0, scores at level 0.  The result is the best (the tie rule of
 *             srrg2_gridmap_match_scans) of everything scored: the guess, the seed block, the children at level 0.
 *   lists     the blocks of one scan to evaluate at one level below L are at most max_list_entries (0 = 2^20); a scan with more
 *             falls back: its whole window is scored exhaustively, fell_back = 1, the result is the same.  The limit is per scan,
 *             so that falling back depends on the inputs alone.
 *   stats     per scan, NULL or num_scans structs in host memory, a function of the inputs alone: num_evaluated[l] = the blocks
 *             bounded at level l = 1 .. L and, at l = 0, the candidates scored in the descent (seed block and guess are not
 *             counted); num_survivors[l], l = 1 .. L; floor_score; seed_block; fell_back.  After a fall-back the levels above
 *             the one whose list overflowed keep their counts, that level and those below have 0, and num_evaluated[0] =
 *             num_candidates.
 *   effort    one upload, one host wait, a launch count that depends on num_levels alone.  Device memory: 4 bytes per block of
 *             level L and, per scan, 8 bytes per entry of min(limit, num_candidates).
 *   refused   what srrg2_gridmap_match_scans refuses, and SRRG2_E_INVALID: null prune params; num_levels outside 1 .. 6 or above
 *             the number built; stale planes; a negative max_list_entries.  Parameters are checked before the handle; every
 *             destination stays as it was.  There is no score volume: srrg2_gridmap_match_scans has it. */
typedef struct srrg2_gridmap_prune_params {
  int32_t num_levels;                     /* L, 1 .. 6 and <= the levels built */
  int32_t max_list_entries;               /* per scan and level; 0 = 2^20 */
} srrg2_gridmap_prune_params;
typedef struct srrg2_gridmap_prune_stats {
  int32_t num_candidates;
  int32_t num_evaluated[7];               /* [l], l = 0 .. 6 */
  int32_t num_survivors[7];               /* [l], l = 1 .. 6; [0] = 0 */
  int32_t floor_score;
  int32_t seed_block;                     /* flat block index at level L */
  int32_t fell_back;
} srrg2_gridmap_prune_stats;
/* num_levels = 4, max_list_entries = 0 */
void srrg2_gridmap_default_prune_params(srrg2_gridmap_prune_params* p);
int srrg2_gridmap_build_bounds(srrg2_gridmap_h h, int num_levels /* 1 .. 6 */);
int srrg2_gridmap_get_bounds(srrg2_gridmap_h h, int level /* 1 .. the levels built */, uint8_t* dst, int row_stride_bytes, int mem);
int srrg2_gridmap_match_scans_pruned(srrg2_gridmap_h h, const float* ranges, int num_scans, const float* guess_robot_in_world, int mem,
                                     const srrg2_gridmap_scan_params* scan_params, const srrg2_gridmap_match_params* match_params,
                                     const srrg2_gridmap_prune_params* prune_params, srrg2_gridmap_match_result* results,
                                     srrg2_gridmap_prune_stats* stats /* NULL ok */);

/* TSDF volume: depth frames and the poses they were taken from -> one truncated signed-distance volume on the device, the dense
 * model of the 3-D pipeline (rectify_pair, adapt_stereo_dense / an RGB-D depth image, adapt_depth_image, the projective aligner,
 * the SE(3) pose graph).  A raycast from a pose gives an organised scene with normals -- set_fixed of the projective point-to-plane
 * slice: frame-to-model tracking --, the export a 3-D cloud.  No reference counterpart; DESIGN.md section 4 "TSDF volume" is the
 * contract, tests/tsdf_restatement.py restates it and the library gives the same bits.  All float work is float32 in the written
 * order, no FMA.
 *   volume    nx x ny x nz voxels of voxel_size metres; origin = world position of the corner of voxel (0, 0, 0); voxel (x, y, z)
 *             lives at plane index (z ny + y) nx + x, its centre is origin + ((float) i + 0.5f) * voxel_size per axis.  The state
 *             is two int32 planes, sum and weight, and -- with_intensity = 1 -- a third, isum.
 *   frame     per frame and voxel: c = world_in_camera * centre, world_in_camera = the inverse of camera_in_world formed once on
 *             the host (transposed rotation, the translation -((a + b) + c) in float64, rounded once), rows ((m0 x + m1 y) + m2 z)
 *             + m3; the projection of srrg2_scene_clip_projective: c.z > 0, u = (K0 c.x) / c.z + K2, v = (K4 c.y) / c.z + K5, in
 *             view iff 0 <= u + 0.5 < cols and 0 <= v + 0.5 < rows, pixel (floor(v + 0.5), floor(u + 0.5)); d = that pixel's U16
 *             count * depth_scale, or its F32 value: skipped unless finite and inside [depth_min, depth_max]; s = d - c.z: skipped
 *             if s < -mu; t = min(s, mu), q = (int32) floorf((t / mu) * 32767.0f + 0.5f); sum += weight q, weight plane += weight,
 *             isum += weight I (U8, or F32 as floorf(x + 0.5f) clamped to 0 .. 255, NaN = 0).
 *   adds      integers only: the planes do not depend on scheduling, frame order or batch split; a batch with weight -1 after
 *             the same batch with +1 restores them bit for bit.  No saturation.
 *   result    num_frames; num_pixels = num_frames rows cols; num_valid_depth: the pixels of all frames that pass the depth gate;
 *             num_voxel_updates: the adds made to the weight plane.
 *   raycast   voxel valid iff weight >= min_weight, F = (float) sum / (float) weight.  Sample at world point p: g = (p - origin) /
 *             voxel_size - 0.5f per axis, i0 = floorf(g), f = g - i0; valid iff all eight corners i0 + {0, 1}^3 lie in the volume
 *             and are valid; blended along x, then y, then z as a + f (b - a).  Pixel (r, c): z_i = depth_min + (float) i * step,
 *             i = 0 .. floorf((depth_max - depth_min) / step); camera point ((((float) c - K2) / K0) z_i, (((float) r - K5) / K4)
 *             z_i, z_i), world point camera_in_world * that (rows as above).  Surface at the first i >= 1 with samples i - 1 and i
 *             valid, F_{i-1} > 0 and F_i <= 0: z* = z_{i-1} + (step F_{i-1}) / (F_{i-1} - F_i); no such i, or z* outside
 *             [depth_min, depth_max]: depth 0.0f.  Intensity: the voxel (floorf((p* - origin) / voxel_size) per axis) that holds
 *             the world point p* of z*; inside the volume and weight >= 1: (isum + weight / 2) / weight clamped to 0 .. 255, else 0.
 *             The depth image (and the U8 intensity image of a volume that has one) then goes through srrg2_adapt_depth_image
 *             into dst with the caller's params: organised or compact, normals and gates are the adaptor's.  skip_empty = 1
 *             consults a mask of 8 x 8 x 8 blocks that hold a valid voxel before it fetches a sample's corners; the bits are those of
 *             skip_empty = 0.
 *   to_scene  per voxel v and axis a in (x, y, z) order: v and its +a neighbour both valid, F0 and F1 of opposite sign or exactly
 *             one of them 0 -> the point at v's centre moved by (F0 / (F0 - F1)) voxel_size along a:
 *             origin_a + (((float) i_a + 0.5f) + F0 / (F0 - F1)) * voxel_size.  Normal: (Fx+ - Fx-, Fy+ - Fy-, Fz+ - Fz-) of v's six
 *             neighbours divided by sqrtf((gx gx + gy gy) + gz gz); NaN when a neighbour is missing or invalid or the gradient is
 *             zero.  srrg2_scene_global_indices(dst) gives 3 (plane index) + a.
 *   waits     every call runs on the volume's stream, in order.  srrg2_tsdf_integrate_frames with out == NULL only queues and
 *             returns (host images are consumed before it returns; device images must stay untouched until a later call of
 *             this handle has waited); with `out` it waits once.  The other calls return when their output is complete.
 *   refused   every destination and the planes unchanged; parameters are checked before the handle.  SRRG2_E_INVALID: a null
 *             handle, params or (where there is data) data pointer; a handle without srrg2_tsdf_reset; nx, ny or nz outside
 *             0 .. 2048; with_intensity other than 0 / 1; a voxel_size, mu or step that is not finite or <= 0; an origin or pose
 *             that is not finite; a weight other than +1 / -1; num_frames < 0; a depth type other than U16 / F32; an intensity
 *             type other than U8 / F32 where the volume has the plane, other than NONE where it has not; a misaligned or too-small
 *             stride; what srrg2_adapt_depth_image refuses of its params; min_weight < 1; skip_empty other than 0 / 1; (depth_max -
 *             depth_min) / step NaN or beyond 2^20; a dst scene that is not 3-D or lives on another device; bad mem.
 *             SRRG2_E_UNSUPPORTED: K[0][1] != 0; nx ny nz beyond int32 (srrg2_tsdf_to_scene: 3 nx ny nz beyond int32).
 *             Zero frames, zero pixels and an empty volume are accepted and do nothing. */
typedef struct srrg2_tsdf_s* srrg2_tsdf_h;
typedef struct srrg2_tsdf_params {
  int32_t nx, ny, nz;       /* 0 .. 2048 each */
  float   voxel_size;       /* metres */
  float   origin[3];        /* world position of the corner of voxel (0, 0, 0) */
  int32_t with_intensity;   /* 1: the volume has the isum plane */
} srrg2_tsdf_params;
typedef struct srrg2_tsdf_frame_params {
  float   mu;               /* truncation distance, metres, > 0 */
  int32_t reserved;         /* 0 */
} srrg2_tsdf_frame_params;
typedef struct srrg2_tsdf_raycast_params {
  float   step;             /* march step along the optical axis, metres, > 0 */
  int32_t min_weight;       /* >= 1 */
  int32_t skip_empty;       /* 1: consult the block mask; 0 (default): the plain march */
  int32_t reserved;         /* 0 */
} srrg2_tsdf_raycast_params;
typedef struct srrg2_tsdf_result {
  int64_t num_frames, num_pixels, num_valid_depth, num_voxel_updates;
} srrg2_tsdf_result;
typedef struct srrg2_tsdf_raycast_result {
  int32_t num_pixels, num_surface;  /* rows cols; pixels with a depth other than 0 */
  srrg2_adapt_result adapt;         /* what srrg2_adapt_depth_image reported (zeros when dst is NULL) */
} srrg2_tsdf_raycast_result;
typedef struct srrg2_tsdf_export_result {
  int32_t num_points, reserved;
} srrg2_tsdf_export_result;
/* a volume on `device`: its own non-blocking stream, its planes in device memory */
int srrg2_tsdf_create(int device, srrg2_tsdf_h* out);
int srrg2_tsdf_destroy(srrg2_tsdf_h h);
/* an empty volume (0 x 0 x 0) of 0.02 m voxels at the origin, no intensity; mu 0.06; step 0.02, min_weight 1, skip_empty 0 */
void srrg2_tsdf_default_params(srrg2_tsdf_params* p);
void srrg2_tsdf_default_frame_params(srrg2_tsdf_frame_params* p);
void srrg2_tsdf_default_raycast_params(srrg2_tsdf_raycast_params* p);
/* allocates (or re-uses) the planes and zeroes them */
int srrg2_tsdf_reset(srrg2_tsdf_h h, const srrg2_tsdf_params* p);
/* depth (and intensity): num_frames images of cam->rows rows, one behind the other (image k begins k rows row_stride bytes behind
 * the first), in `mem` = SRRG2_MEM_HOST | SRRG2_MEM_DEVICE; camera_in_world: num_frames x 12 floats in HOST memory (the inverse is
 * formed on the host).  cam: camera_matrix, rows, cols, depth_scale, depth_min, depth_max are read.  One upload; the number of
 * launches does not depend on num_frames. */
int srrg2_tsdf_integrate_frames(srrg2_tsdf_h h, const void* depth, int depth_type, int depth_row_stride_bytes, const void* intensity,
                                int intensity_type, int intensity_row_stride_bytes, int num_frames, const float* camera_in_world,
                                int mem, const srrg2_depth_adaptor_params* cam, const srrg2_tsdf_frame_params* fp,
                                int weight /* +1 | -1 */, srrg2_tsdf_result* out /* may be NULL: queue only */);
/* dst: a 3-D scene on the volume's device, or NULL; depth_out: cam->rows x cam->cols floats, packed, in depth_mem, or NULL */
int srrg2_tsdf_raycast(srrg2_tsdf_h h, const float* camera_in_world /* 12, host */, const srrg2_depth_adaptor_params* cam,
                       const srrg2_tsdf_raycast_params* rp, srrg2_scene_h dst, float* depth_out, int depth_mem,
                       srrg2_tsdf_raycast_result* out /* may be NULL */);
int srrg2_tsdf_to_scene(srrg2_tsdf_h h, int min_weight, srrg2_scene_h dst, srrg2_tsdf_export_result* out /* may be NULL */);
/* nx ny nz int32 each to sum / weight / isum (isum: only a volume that has it) in `mem`; any pointer may be NULL */
int srrg2_tsdf_get_planes(srrg2_tsdf_h h, int32_t* sum, int32_t* weight, int32_t* isum, int mem);
/* the planes in device memory, valid until the next reset; isum receives NULL when the volume has none (isum itself may be NULL) */
int srrg2_tsdf_device_arrays(srrg2_tsdf_h h, const int32_t** sum, const int32_t** weight, const int32_t** isum);

/* Feature tracking: which keypoint of the measurement is which landmark of the clipped local map -- the per-frame data
 * association of a visual tracker, a projective window plus the Hamming distance of the 256-bit descriptors.  The reference
 * declares the slot and leaves it empty (CorrespondenceFinder_::compute() is pure virtual, S/registration/correspondence_finder.h:56;
 * its inputs are setFixed, setMoving and setLocalMapInSensor, :80-114).  DESIGN.md section 4 "Feature tracking" is the contract,
 * tests/tracking_restatement.py restates it and the library gives the same bits.
 *   fixed     the measurement: a dim-3 scene with descriptors whose srrg2_scene_global_indices are pixel indices r*cols + c in
 *             strictly ascending order (what srrg2_adapt_image_features / _stereo_features write, or a clip of such a scene).
 *             A scene as srrg2_adapt_image_features_pyramid left it is taken too: level-major, its pixels (the nearest level-0
 *             pixels) ascend strictly inside each level and may repeat across levels; the levels are searched one by one and
 *             merged, the result is that of the rules below on all keypoints (the window is in level-0 pixels on every level).
 *             Keypoint j is fixed point j, its pixel its global index.  Its coordinates are NOT read: a keypoint with a non-finite
 *             point still matches (the aligner reports such a given pair as Suppressed).
 *   moving    the clipped local map: a dim-3 scene with descriptors, in any order.
 *   project   a landmark with a non-finite coordinate is not in view; else c = moving_in_sensor * p (rows as ((m0 x + m1 y) + m2 z)
 *             + m3, float32, no FMA) and the steps of srrg2_scene_clip_projective: depth_min <= c.z <= depth_max,
 *             u = (K0 c.x) / c.z + K2, v = (K4 c.y) / c.z + K5, in view iff 0 <= u + 0.5 < cols and 0 <= v + 0.5 < rows,
 *             cu = floor(u + 0.5), rv = floor(v + 0.5).
 *   candidates  of landmark i: the keypoints j with |r_j - rv| <= search_radius and |c_j - cu| <= search_radius.
 *   best      the candidate of smallest (Hamming distance h, j); accepted iff h <= max_distance and -- min_margin > 0 --
 *             h2 - h >= min_margin, h2 being the smallest distance among the OTHER candidates (a lone candidate passes).
 *   cross     cross_check: per keypoint j, of the landmarks that have j as a candidate, the one of smallest (h, i); landmark i stays
 *             iff its best keypoint's best is i.  No gate is applied in that direction (as in the stereo matcher).
 *   output    the surviving pairs in ascending i as {fixed_idx = j, moving_idx = i, response = (float) h}: the aligner's
 *             convention for srrg2_aligner_set_correspondences (measurement fixed, clipped map moving).  moving_idx is the index
 *             in `moving`; srrg2_scene_global_indices(moving) leads to the map.  correspondences_out (host, may be NULL) receives
 *             min(capacity, num_correspondences) records; num_correspondences is not limited by capacity.
 *   refused   nothing is written.  SRRG2_E_INVALID: a null handle, pose or params; moving == fixed; different devices; a dim other
 *             than 3; rows or cols <= 0 or rows*cols beyond int32; fx or fy zero or not finite; !(depth_min > 0) or
 *             !(depth_max >= depth_min); search_radius outside 0 .. 255; max_distance or min_margin outside 0 .. 256; cross_check
 *             not 0 / 1; reserved != 0; capacity < 0; a non-finite moving_in_sensor; fixed global indices that do not ascend
 *             strictly (a pyramid scene: inside each level) inside [0, rows*cols) (found on the device, reported at the call's host wait).  SRRG2_E_UNSUPPORTED: K with
 *             skew (K[0][1] != 0), as the clipper.  SRRG2_E_STATE: a non-empty scene without descriptors; a non-empty fixed scene
 *             whose global indices do not cover its points (srrg2_scene_set leaves none).
 *   empty     an empty scene on either side: 0, no correspondences, the counters filled (an empty `moving` returns before the
 *             device is asked: fixed's indices are then not looked at).
 *   waits     ONE host wait: the counters, the error word, the number of pairs and the capacity-bounded records come back in one
 *             copy.  Both scenes are left as they were; the workspaces live on `moving`, a steady-state call allocates nothing.
 * search_radius 16 and max_distance 48 are UNTUNED defaults: nobody has derived or measured them. */
typedef struct srrg2_track_params {
  float   camera_matrix[9];      /* row-major K; K[0][1] != 0 -> SRRG2_E_UNSUPPORTED (as the clipper) */
  int32_t image_rows, image_cols;
  float   depth_min, depth_max;  /* gate on the landmark's c.z, as srrg2_scene_clip_projective; default 0.4, 8 */
  int32_t search_radius;         /* pixels, 0 .. 255, default 16 (untuned): the window is the square |dr| <= R, |dc| <= R */
  int32_t max_distance;          /* 0 .. 256, default 48 (untuned): largest accepted Hamming distance */
  int32_t min_margin;            /* 0 .. 256, default 0 = off; else second-best distance - best distance >= min_margin */
  int32_t cross_check;           /* 0 | 1, default 1 */
  int32_t reserved;              /* 0 */
} srrg2_track_params;            /* 72 bytes */
typedef struct srrg2_track_result {
  int32_t num_moving, num_fixed;
  int32_t num_in_view;           /* landmarks that project into the image inside the depth gate */
  int32_t num_with_candidate;    /* ... with at least one keypoint in their window */
  int32_t num_accepted;          /* ... whose best passes max_distance and min_margin */
  int32_t num_mutual;            /* ... that survive the cross check (= num_accepted when it is off) */
  int32_t num_correspondences;   /* == num_mutual; NOT limited by capacity */
  int32_t reserved;
} srrg2_track_result;            /* 32 bytes */
/* K, rows and cols zero (the caller must set them), depth 0.4 .. 8, search_radius 16, max_distance 48, min_margin 0, cross_check 1 */
void srrg2_track_default_params(srrg2_track_params* p);
int srrg2_scene_track_features(srrg2_scene_h moving, srrg2_scene_h fixed, const float* moving_in_sensor /* 3x4 */,
                               const srrg2_track_params* p, srrg2_correspondence* correspondences_out /* host, may be NULL */,
                               int capacity, srrg2_track_result* out /* may be NULL */);

/* Consensus pose: geometric verification of descriptor matches -- K candidates x H minimal-sample hypotheses x N matches of
 * transform-and-compare (RANSAC with a fixed hypothesis count), in one call.  The reference has no such step: its HBST detector
 * hands the raw matches to the locked Gauss-Newton solve (multi_loop_detector_hbst_impl.cpp:257-377).  DESIGN.md section 4
 * "Consensus pose" is the contract, tests/consensus_restatement.py restates it and the library gives the same bits.
 *   clouds    `fixed` is the query cloud, `moving` the K candidates' clouds one behind the other (moving_offsets: K + 1 point
 *             indices); both in `mem` = SRRG2_MEM_HOST | SRRG2_MEM_DEVICE (srrg2_scene_device_arrays: stride 16), borrowed for
 *             the call only.  Strides: multiples of 4, >= dim * 4 (12 and 16 among them).
 *   pairs     candidate k's records are correspondences[corr_offsets[k] .. corr_offsets[k+1]) (host), in the aligner's
 *             convention: fixed_idx indexes the query, moving_idx the candidate's OWN cloud.  A pair is valid iff both indices
 *             are in range and all `dim` coordinates of both points are finite; an invalid pair is never an inlier and is no error.
 *   sampling  s = 3 (dim 3) | 2 (dim 2).  mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *             (uint32).  base = mix32(mix32(seed) + h); index j of hypothesis h: for attempt a = 0 .. 3, r = mix32(base + 4 j + a),
 *             i = ((uint64) r * N) >> 32, the first i that differs from the hypothesis's earlier indices.  None, a sampled invalid
 *             pair or N < s: the hypothesis is DEGENERATE.  The candidate's index is not in the hash: result k of a batch is bit
 *             for bit the result of a K = 1 call on candidate k alone.
 *   solver    float64 from the float32 points, + - * / sqrt only (csrc/consensus_math.h).  dim 3: the orthonormal frames of the
 *             moving and the fixed triple (a = p1 - p0, b = p2 - p0, n = a x b, e1 = a / |a|, e3 = n / |n|, e2 = e3 x e1;
 *             degenerate iff |a|^2 < msd^2 or |n|^2 < msd^2 |a|^2), R = Ef Em^T, t = cf - R cm on the centroids.  dim 2: angle
 *             between the two segments, t on the midpoints.  A non-finite entry: degenerate.
 *   length    length_check: REJECTED iff for some two sample points | |m_i - m_j| - |f_i - f_j| | > 2 inlier_distance.
 *   score     float32, on the pose cast to float32 -- which is the pose returned: r_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i - f_i,
 *             e = (r0^2 + r1^2) + r2^2, inlier iff e <= tau * tau (float32).  cost = the int64 sum over the inliers of
 *             trunc((double) e * 2^cost_exponent): order-independent.
 *   best      largest count, then smallest cost, then smallest h, over the scored hypotheses; all H are always evaluated.
 *             status NO_HYPOTHESIS: none was scored (pose all zero, best_hypothesis -1); TOO_FEW_INLIERS: count <
 *             max(min_inliers, s), pose and counters still written; FOUND otherwise.
 *   inliers   the records of the best hypothesis's inliers in input order (response carried through), for FOUND candidates only,
 *             concatenated over the candidates: inliers_out (host, may be NULL) receives the first inlier_capacity of them,
 *             inlier_offsets_out (K + 1, may be NULL) is NOT limited by inlier_capacity.
 *   refused   SRRG2_E_INVALID, nothing written: a null handle, params or results (K > 0); K < 0; decreasing or negative offsets;
 *             null clouds or records where points / records exist; bad strides; num_hypotheses outside 1 .. 65536; inlier_distance
 *             not finite or <= 0; min_sample_distance not finite or < 0; min_inliers < 0; length_check not 0 / 1; reserved != 0;
 *             inlier_capacity < 0; a mem other than HOST | DEVICE (SRRG2_MEM_DEVICE_KEPT among them).  K = 0 returns 0.  A candidate
 *             without pairs gets NO_HYPOTHESIS.
 *   waits     ONE host wait: results, offsets and the capacity-bounded records come back in one copy.  The handle owns a stream
 *             and the workspaces; a steady-state call allocates nothing.  The number of launches does not depend on K, H or N.
 * inlier_distance 0.05, min_sample_distance 0.1 and num_hypotheses 256 are UNTUNED defaults: nobody has derived or measured them. */
typedef struct srrg2_consensus_s* srrg2_consensus_h;
enum srrg2_consensus_status { SRRG2_CONSENSUS_FOUND = 0, SRRG2_CONSENSUS_NO_HYPOTHESIS = 1, SRRG2_CONSENSUS_TOO_FEW_INLIERS = 2 };
typedef struct srrg2_consensus_params {
  int32_t  num_hypotheses;      /* 1 .. 65536, default 256 (untuned) */
  float    inlier_distance;     /* m, > 0 and finite, default 0.05 (untuned) */
  float    min_sample_distance; /* m, >= 0 and finite, default 0.1 (untuned): sample points closer than this, or a triangle
                                   flatter than this, are degenerate */
  int32_t  min_inliers;         /* >= 0, default 0: FOUND needs max(min_inliers, s) inliers */
  uint32_t seed;                /* default 0 */
  int32_t  length_check;        /* 0 | 1, default 1 */
  int32_t  reserved[2];         /* 0 */
} srrg2_consensus_params;       /* 32 bytes */
typedef struct srrg2_consensus_result {
  float   moving_in_fixed[12];  /* row-major 3 x 4; SE(2): the first 9, a row-major 3 x 3 */
  int32_t status;               /* srrg2_consensus_status */
  int32_t best_hypothesis;      /* -1 when none was scored */
  int32_t num_inliers;
  int32_t num_pairs, num_valid_pairs;
  int32_t num_degenerate, num_rejected, num_scored; /* sum to num_hypotheses */
  int32_t cost_exponent;
  int32_t reserved;
  int64_t cost;                 /* fixed point: sum of trunc(e * 2^cost_exponent) over the inliers */
} srrg2_consensus_result;       /* 96 bytes */
int  srrg2_consensus_create(int dim /* 2 | 3 */, int device, srrg2_consensus_h* out);
int  srrg2_consensus_destroy(srrg2_consensus_h h);
void srrg2_consensus_default_params(srrg2_consensus_params* p);
int  srrg2_consensus_compute(srrg2_consensus_h h, const float* fixed, int fixed_stride_bytes, int num_fixed, int K,
                             const float* moving, int moving_stride_bytes, const int32_t* moving_offsets /* K + 1 */,
                             int mem /* of both clouds: SRRG2_MEM_HOST | SRRG2_MEM_DEVICE */,
                             const srrg2_correspondence* correspondences /* host */, const int32_t* corr_offsets /* K + 1 */,
                             const srrg2_consensus_params* p, srrg2_consensus_result* results /* [K] */,
                             srrg2_correspondence* inliers_out /* host, may be NULL */, int64_t inlier_capacity,
                             int64_t* inlier_offsets_out /* [K + 1], may be NULL */);

/* ---- strategy knobs (no reference counterpart) ----------------------------------------------------------------
 * Every setting gives the SAME results (indices, estimates, statistics bit for bit): the knobs choose between exact
 * strategies of the finder / reduction / control step.  A handle starts from srrg2_aligner_default_tuning() overridden
 * by the SRRG2_AMD_* environment variables, which are read ONCE, in srrg2_aligner_create (never inside compute()).
 * Negative values of the `int32_t` switches mean "automatic" (the library picks by problem size).
 * strategy_mask holds only the SRRG2_TUNE_* bits below: each forces, on any configuration, a path the library also takes
 * by itself on others.  srrg2_aligner_set_tuning rejects any other bit with SRRG2_E_INVALID; SRRG2_AMD_TUNE has them
 * masked off, as the environment's other out-of-range values are clamped. */
#define SRRG2_TUNE_PROJ_SEPARATE_LAUNCHES (1 << 17) /* projective slices in launches of their own (taken anyway for one
                                                       projective slice, mixed slices or more than four)              */
#define SRRG2_TUNE_INIT_LAUNCH (1 << 23) /* the k_icp_init launch in front of every compute() (taken anyway on a handle's
                                            first compute() and wherever the prologue cannot ride in the first pass)  */
#define SRRG2_TUNE_KNOWN_BITS (SRRG2_TUNE_PROJ_SEPARATE_LAUNCHES | SRRG2_TUNE_INIT_LAUNCH)
typedef struct srrg2_aligner_tuning {
  int32_t strategy_mask;        /* SRRG2_AMD_TUNE: SRRG2_TUNE_* bits (DESIGN.md "Strategy knobs"); 0 = defaults       */
  int32_t queue_probe_iteration;/* SRRG2_AMD_QPROBE: iteration whose deferred-search counters decide whether the
                                   deferred-search launch is kept (default 1; -1 = never drop it)                      */
  int32_t small_max_points;     /* SRRG2_AMD_SMALL_MAX: upper limit of the clouds the one-workgroup kernel may take
                                   (1024; below it the faster of the two paths is chosen per configuration)            */
  int32_t fast_from_iteration;  /* SRRG2_AMD_FAST_FROM: first iteration the converged-pass kernel takes (3)           */
  int32_t fast_points_per_thread; /* SRRG2_AMD_FAST_PPT: 1, 2 or 4; 0 (default) = 2 for launches of 64 alignments or more, else 1 */
  int32_t fast_min_points;      /* SRRG2_AMD_FAST_MIN: smallest moving cloud using the converged-pass kernel (0)       */
  int32_t fast_gather;          /* SRRG2_AMD_FAST_GATHER: kept neighbours gathered from the fixed cloud (1) or streamed
                                   from per-point arrays (0); -1 = batches of more than 4 alignments gather            */
  int32_t fast_batch_queue;     /* SRRG2_AMD_FAST_QUEUE: batches hand failed certificates to the deferred-search kernel (0) */
  int32_t queue_min_points;     /* SRRG2_AMD_QUEUE_MIN: smallest moving cloud that uses the deferred-search kernel (90000) */
  int32_t msort_segments;       /* SRRG2_AMD_MSORT_SEGMENTS: workgroups per cloud of the batch Morton sort; 0 = automatic */
  int32_t msort_key_bits;       /* SRRG2_AMD_MSORT_BITS: total bits of the (anisotropic) Morton key of the moving-cloud
                                   sort; 0 = automatic (15: one kernel, histogram in LDS; 16 .. 18 take the global-histogram
                                   kernels); -1 = the
                                   round-2 isotropic keys (4 / 5 / 6 bits per axis by batch size)                      */
  int32_t lds_tile;             /* SRRG2_AMD_LDS_TILE: search passes of batches stage each wave's neighbourhood of the
                                   fixed cloud in LDS (1) or gather it per lane (0); -1 = automatic                     */
  float   cell_target;          /* SRRG2_AMD_CELL_TARGET: points per occupied grid cell the automatic cell size aims at (8) */
  float   rmax_cap;             /* SRRG2_AMD_RMAX_CAP: largest cube radius (cells) needed to cover the gate; 0 = default
                                   (3 for 2-D clouds, none for 3-D)                                                    */
  int32_t search_lists;         /* SRRG2_AMD_SEARCH_LISTS: search passes walk per-cell lists of occupied neighbour cells built
                                   once per fixed cloud (k_icp_step_cnl): 0 = never, 1 = batches of more than 4 alignments,
                                   2 = every alignment; -1 = automatic (carved out of reserved_: same struct size)        */
  int32_t search_team;          /* SRRG2_AMD_SEARCH_TEAM: low byte = lanes per moving point of that kernel: 0 = automatic, 1, 2 or
                                   4 = the most a point gets.  Launches of up to four alignments deal their points over
                                   tiles of 4, 2 and 1 lanes per point so that the launch fits the workgroups that are
                                   resident together (as many points as fit at the higher counts); larger batches take 4 or
                                   1 for every point.  Bits 8 and up, when not zero: the number of resident workgroups
                                   that plan assumes instead of the device's own (a sweep and test knob).  < 0: refused  */
  int32_t batch_pipeline;       /* SRRG2_AMD_BATCH_PIPELINE: compute_batch runs its alignments as P parts on P streams (one
                                   part's control steps and sort under the other parts' passes): 0 = never, 1 = two halves
                                   for every batch, 2 .. 8 = that many parts, -1 = automatic                             */
  int32_t fused_control;        /* SRRG2_AMD_FUSED_CONTROL: the control step of an ICP iteration (sums, Gauss-Newton step, update,
                                   statistics, termination) runs on one wave in the prologue of the next iteration's first
                                   pass kernel instead of as a launch of its own: 0 = never, 1 / -1 = whenever the aligner is ONE
                                   nearest-neighbour cue slice (searched over cell neighbour lists: every iteration; on the
                                   grid kernels -- a first compute() on a fixed cloud --: from the first converged pass on), or
                                   projective slices that share one association -- with up to two prior slices before or
                                   behind them (an odometry prior, a motion model: the control wave linearises their
                                   factors itself); 2 = as 1, but aligners WITH prior slices keep their control launches
                                   (carved out of reserved_)                                                             */
  int32_t reserved_[6];
} srrg2_aligner_tuning;
/* built-in defaults (the environment is NOT consulted) */
void srrg2_aligner_default_tuning(srrg2_aligner_tuning* t);
/* the handle's current knobs / replace them (takes effect from the next set_fixed / set_moving / compute) */
int srrg2_aligner_get_tuning(srrg2_aligner_h h, srrg2_aligner_tuning* t_out);
int srrg2_aligner_set_tuning(srrg2_aligner_h h, const srrg2_aligner_tuning* t);

/* ---- measurement hooks (no reference counterpart: the reference profiles with
 * PROFILE_TIME scopes outside the aligner) ------------- */

/* When enabled, every launch of the fused ICP step kernel is bracketed by a pair of HIP events
 * on the launch stream; get returns the accumulated time and launch count since the last reset. */
int srrg2_aligner_profile_enable(srrg2_aligner_h h, int enable);
int srrg2_aligner_profile_get(srrg2_aligner_h h, double* step_kernel_ms, int64_t* step_kernel_launches,
                              int reset);
/* Which launch path the handle's LAST compute() / compute_batch() took (strategy only: results do not depend on it; what the
 * tests of those paths assert).  Bits: */
#define SRRG2_PATH_FUSED_CONTROL 1   /* control steps inside the pass kernels (tuning.fused_control)                       */
#define SRRG2_PATH_ALL_PASSES_FUSED 2 /* ... of every pass (else: from the first converged pass on)                         */
#define SRRG2_PATH_FINAL_WAVE 4      /* the last control step + post / finalize on one wave (k_icp_final_wave)             */
#define SRRG2_PATH_PROLOGUE_IN_PASS 8 /* no k_icp_init launch: compute()'s prologue rode in the first pass kernel           */
#define SRRG2_PATH_ONE_WORKGROUP 16  /* the whole compute() in one workgroup per problem (k_icp_small)                     */
#define SRRG2_PATH_PRIORS_FUSED 32   /* prior slices linearised by the control wave                                        */
int srrg2_aligner_last_compute_path(srrg2_aligner_h h, int32_t* flags_out);

/* ---- binary descriptor database: the matching half of MultiLoopDetectorHBST_ -----------------------------------
 * (S/registration/loop_detector/multi_loop_detector_hbst_impl.cpp:41-70 addPreviousQuery, :72-161
 * computeCorrespondences, :163-197 _computeCorrespondencesFromMatches; PARAMs multi_loop_detector_hbst.h:45-74).
 * The reference keeps srrg_hbst::BinaryTree256<uint64_t>; this database is that tree with a single leaf: the search is
 * exhaustive and exact on the device ("Descriptor matching").
 *  - a descriptor is 256 bits = SRRG2_DESCRIPTOR_BYTES bytes (the ORB/BRIEF row of the reference); the Hamming distance
 *    does not depend on the bit order.
 *  - valid: one byte per point, nonzero = POINT_STATUS::Valid (NULL = all valid).  Invalid points are not matchables
 *    (:131-136) but keep their index: every index below is a POINT index of the caller's array, never compacted.
 *  - add: only the valid descriptors enter; the map's database index is the number of maps before it (:57);
 *    a map without valid descriptors is not added (*index_out = -1, :46-49).  The graph id -> index map is the caller's.
 *  - match: a pair (valid query q, database descriptor j of map r) matches iff hamming(q, j) < max_distance (strict;
 *    the float threshold against the integer distance).  Maps failing the age gate of :150-151 (unsigned indices:
 *    a map passes iff (r < query_index and query_index - r > min_age) or r > query_index) are not searched; a map is a
 *    candidate iff its number of matching pairs > min_matches (:152-154).  Per reference descriptor the query with the
 *    smallest distance is kept, the smallest query index on a tie (:168-197) -> srrg2_correspondence{fixed_idx = query
 *    point, moving_idx = reference point, response = distance}.  Candidates ascend in r, each one's correspondences in
 *    moving_idx.  A query holds at most 2^23 points.
 *  - getters (*n_inout: capacity on entry, number of entries on return; a NULL buffer queries the number):
 *    get_candidates       reference index, pre-deduplication match count, offsets of each candidate's
 *                         correspondences (corr_offsets has n + 1 entries)
 *    get_correspondences  all candidates' correspondences, concatenated in candidate order
 *    get_map_counts       the match count of EVERY map of the database, -1 for the maps the age gate skipped
 *    last_match_ms        HIP-event time of the last match(): query upload + search + compaction, without the readback */
#ifndef SRRG2_DESCRIPTOR_BYTES
#define SRRG2_DESCRIPTOR_BYTES 32
#endif
typedef struct srrg2_descriptor_db* srrg2_descriptor_db_h;
int srrg2_descriptor_db_create(int device, srrg2_descriptor_db_h* out);
int srrg2_descriptor_db_destroy(srrg2_descriptor_db_h h);
int srrg2_descriptor_db_add(srrg2_descriptor_db_h h, const uint8_t* descriptors, const uint8_t* valid, int n,
                            int* index_out);
int srrg2_descriptor_db_size(srrg2_descriptor_db_h h, int* maps, int64_t* descriptors);
int srrg2_descriptor_db_match(srrg2_descriptor_db_h h, const uint8_t* descriptors, const uint8_t* valid, int n,
                              int64_t query_index, float max_distance, uint32_t min_age, int64_t min_matches,
                              int* K_out);
int srrg2_descriptor_db_get_candidates(srrg2_descriptor_db_h h, int32_t* reference, int64_t* num_matches,
                                       int64_t* corr_offsets, int* n_inout);
int srrg2_descriptor_db_get_correspondences(srrg2_descriptor_db_h h, srrg2_correspondence* buf, int64_t* n_inout);
int srrg2_descriptor_db_get_map_counts(srrg2_descriptor_db_h h, int64_t* counts, int* n_inout);
int srrg2_descriptor_db_last_match_ms(srrg2_descriptor_db_h h, double* ms);
/* add / match with the descriptors of a scene that carries them (srrg2_scene_set_features), read on the device: EXACTLY
 * srrg2_descriptor_db_add / _match called with the scene's descriptors and valid[i] = (point i is Valid, i.e. has finite
 * coordinates) -- same database index, candidates, counts and correspondences (fixed_idx = the scene's point index, never
 * compacted), same getters afterwards.  The database keeps a copy: later changes of the scene do not reach it.  Only counts
 * cross to the host.  A scene without descriptors: SRRG2_E_STATE; a scene on another device than the database:
 * SRRG2_E_INVALID; both leave the database as it was.  An empty scene or one without Valid points behaves as n = 0 / no valid
 * descriptor does (*index_out = -1, K = 0).  The call is ordered behind the work queued on the scene's stream and returns
 * when the database no longer reads the scene. */
int srrg2_descriptor_db_add_scene(srrg2_descriptor_db_h h, srrg2_scene_h scene, int* index_out);
int srrg2_descriptor_db_match_scene(srrg2_descriptor_db_h h, srrg2_scene_h scene, int64_t query_index, float max_distance,
                                    uint32_t min_age, int64_t min_matches, int* K_out);

#ifdef __cplusplus
}
#endif
#endif /* SRRG2_SLAM_AMD_H */
