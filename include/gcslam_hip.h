/*
 * gcslam_hip.h -- C-ABI of the MI355X (gfx950) GC-SLAM bin-path per-scan backend.
 *
 * Plain pointers and sizes only.  "dev" pointers are HIP device pointers (HBM), "host"
 * pointers are ordinary host memory.  Every call returns 0 on success or a negative
 * gcs_status; gcs_last_error(ctx) holds the message.  A context owns one hypothesis on one
 * GPU (device buffers, HIP stream, belief, map-bin statistics); calls on one context must be
 * serialised by the caller, distinct contexts are independent (no global mutable state).
 *
 * Reference interfaces replaced (paths relative to the reference repo,
 * FS = fl_ws/src/fl_slam_poc/fl_slam_poc):
 *   gcs_scan                    FS/backend/pipeline.py:316-1591 process_scan_single_hypothesis
 *                               (14-step bin path, README.md:105-122)
 *   gcs_parse_pointcloud2       FS/backend/backend_node.py:377-468 parse_pointcloud2_vlp16 (+ :1677-1680)
 *   gcs_point_stage             FS/backend/operators/point_budget.py:117-221 point_budget_resample
 *                               + FS/backend/operators/deskew_constant_twist.py:72-117 (fused)
 *   gcs_bin_soft_assign         archive/legacy_operators/binning.py:79-131 bin_soft_assign
 *   gcs_scan_bin_moment_match   archive/legacy_operators/binning.py:212-324 (+ kappa.py:130-169)
 *   gcs_matrix_fisher_rotation  archive/legacy_operators/matrix_fisher_evidence.py:264-394
 *   gcs_planar_translation      archive/legacy_operators/matrix_fisher_evidence.py:502-671
 *   gcs_pushforward             PoseCovInflationPushforward (source deleted; CHANGELOG.md:1246)
 *                               + archive/bin_atlas.py:137-257 update/forgetting/derived stats
 *   gcs_psd_project             FS/common/primitives.py:80-123 domain_projection_psd_core
 *   gcs_info_fusion_additive    FS/backend/operators/fusion.py:150-230
 *   gcs_predict_diffusion       FS/backend/operators/predict.py:106-214
 *   gcs_preintegrate_imu        FS/backend/operators/imu_preintegration.py:47-147
 *   gcs_hypothesis_payload /    FS/backend/backend_node.py:1999-2119 (IW accumulation) and
 *   gcs_hypothesis_combine      FS/backend/operators/hypothesis.py:51-117 (barycenter)
 *   gcs_fibonacci_atlas         archive/bin_atlas.py:40-61
 *   gcs_associate_primitives_ot FS/backend/operators/primitive_association.py:239-553
 *                               associate_primitives_ot (+ tiling.py:148-186, measurement_batch.py:389-411)
 *   gcs_visual_pose_evidence    FS/backend/operators/visual_pose_evidence.py:260-412 visual_pose_evidence
 *   gcs_pmap_*                  FS/backend/structures/primitive_map.py:98-2031 (AtlasMap tiles in HBM;
 *                               extract_atlas_map_view, insert_masked, fuse, cull, forget,
 *                               recency_inflate, merge_reduce)
 *   gcs_extract_lidar_surfels   FS/backend/operators/lidar_surfel_extraction.py:339-431
 *                               extract_lidar_surfels (+ FS/common/ma_hex_web.py:243-303
 *                               bin_points_3d, FS/backend/structures/measurement_batch.py:272-381)
 *   gcs_camera_splats           FS/frontend/sensors/lidar_camera_depth_fusion.py + splat_prep.py:37-134
 *                               (lidar_depth_evidence, splat_prep_fused), FS/backend/backend_node.py:
 *                               1872-1925, FS/backend/structures/measurement_batch.py:165-259
 *   gcs_visual_features         src/visual_feature_node.cpp:228-652 (on_rgbd after ORB: depth_sample,
 *                               student_t_effective_var, quadratic_fit, backprojection_cov) and
 *                               FS/backend/backend_node.py:1589-1650 _feature_batch_to_list
 */
#ifndef GCSLAM_HIP_H
#define GCSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: the one-call live path (gcs_live_scan / gcs_live_collect, gcs_live_args / gcs_live_outputs) and
 * gcs_ma_hex_stencil.
 * 3: GCS_ASSOC_CERT_LEN 18 -> 21 (gcs_assoc_outputs grew), the scan mirror's sequence / checksum
 * (gcs_ctx_mirror_stats) and the state checksums (gcs_debug_state_checksums) */
#define GCS_ABI_VERSION 4
#define GCS_D_Z 22
#define GCS_SCAN_FIELDS 26   /* ScanBinStats, field-major: N, s_dir[3], S_dir_scatter[9], p_bar[3], Sigma_p[9], kappa */
#define GCS_MAP_FIELDS 26    /* MapBinStats: S_dir[3], S_dir_scatter[9], N_dir, N_pos, sum_p[3], sum_ppT[9] */
#define GCS_DERIVED_FIELDS 16 /* mu_dir[3], kappa, centroid[3], Sigma_c[9] */
#define GCS_PAYLOAD_LEN 840  /* hypothesis all-reduce payload (f64) */

typedef enum {
  GCS_OK = 0,
  GCS_ERR_ARG = -1,      /* maps to ValueError */
  GCS_ERR_HIP = -2,      /* maps to RuntimeError */
  GCS_ERR_NONFINITE = -3,/* maps to ValueError (reference fail-fast, pipeline.py:546-548) */
  GCS_ERR_STATE = -4
} gcs_status;

typedef enum { GCS_MODE_DENSE = 0, GCS_MODE_SCALE = 1 } gcs_mode;

typedef struct gcs_ctx gcs_ctx;

typedef struct {
  int32_t device;              /* HIP device ordinal */
  int32_t n_bins;              /* B */
  int32_t n_points_cap;        /* N_POINTS_CAP (constants.py:64; raised for C2/C3) */
  int32_t max_raw_points;      /* capacity of the raw input */
  int32_t mode;                /* gcs_mode */
  int32_t k_cand;              /* K candidates per point in scale mode (16) */
  double tau;                  /* soft-assign temperature (declared) */
  double lidar_origin[3];      /* LiDAR origin in base (pipeline.py:589-593) */
  int32_t deskew_rotation_only;/* pipeline.py:482-483 */
  double forgetting_factor;    /* PipelineConfig.forgetting_factor (0.99) */
  double gravity_W[3];         /* constants.py:80 */
  /* step 9 IMU / odometry evidence family (pipeline.py:595-776) and fusion scale (fusion.py:46-142);
   * PipelineConfig fields (pipeline.py:96-223).  Fill with gcs_config_defaults() first. */
  int32_t use_imu_odom;        /* 1: the reference's branch (default); 0: LiDAR-only ablation */
  double imu_gravity_scale;    /* PipelineConfig.imu_gravity_scale (1.0) */
  double planar_z_ref, planar_z_sigma, planar_vz_sigma;  /* constants.py:294-310 (0, 0.1, 0.01) */
  double alpha_min, alpha_max; /* constants.py:89-90 (1, 1) */
  double c0_cond;              /* constants.py:92 (1e6) */
} gcs_config;

typedef struct {
  /* LiDAR scan resident on the device (PointCloud2-like: float x,y,z at offsets 0,4,8) */
  const void* xyz_dev;
  int32_t point_step;
  const double* timestamps_dev;
  const double* weights_dev;
  int32_t n_points;
  /* IMU window (host, padded to imu_len with zero stamps) */
  const double* imu_stamps;    /* [imu_len] */
  const double* imu_gyro;      /* [imu_len*3] */
  const double* imu_accel;     /* [imu_len*3] */
  int32_t imu_len;
  double scan_start_time, scan_end_time, dt_sec;
  const double* Q;             /* [22*22] host; NULL = context's IW-derived Q */
  const double* L_ext;         /* optional external evidence [22*22] (IMU/odom family), may be NULL */
  const double* h_ext;         /* [22] */
  /* scan-to-scan IMU window of the measurement-noise IW statistics (pipeline.py:331-332,448-453) */
  double t_last_scan, t_scan;
  /* 0: float32 x,y,z at bytes 0,4,8 of each point_step record; 1: float64 x,y,z (gcs_parse_pointcloud2) */
  int32_t xyz_format;
  /* odometry (host; NULL = the node's "no odometry yet" inputs: identity pose, 1e12 I covariances,
   * backend_node.py:939-940,2047-2051).  Pose [t, rotvec] relative to the first odometry pose,
   * covariances row-major 6x6 in ROS [x,y,z,roll,pitch,yaw] order, twist [vx,vy,vz,wx,wy,wz] body. */
  const double* odom_pose;     /* [6] */
  const double* odom_cov_se3;  /* [36] */
  const double* odom_twist;    /* [6] */
  const double* odom_twist_cov;/* [36] */
  /* IMU noise proxies (3x3); NULL = IW mode of the context's measurement-noise state
   * (backend_node.py:2020-2023, measurement_noise_iw_jax.py:38-56) */
  const double* Sigma_g;
  const double* Sigma_a;
} gcs_scan_inputs;

/* Layout of a PointCloud2 message (sensor_msgs/PointField offsets and datatype codes) for
 * gcs_parse_pointcloud2; the VLP-16 layout has FLOAT32 x, y, z and a ring field. */
typedef struct {
  int32_t n_points;             /* width * height */
  int32_t point_step;
  int32_t off_x, off_y, off_z;  /* FLOAT32 */
  int32_t off_ring, ring_datatype;
  int32_t off_t, t_datatype;    /* per-point "t" (else "time") field; off_t < 0: none (header stamp) */
  double header_stamp_sec;
  double R_base_lidar[9];       /* row-major; points are returned in the base frame */
  double t_base_lidar[3];
} gcs_pointcloud2_layout;

typedef struct {
  double X_anchor[6];
  double stamp_sec;
  double z_lin[GCS_D_Z];
  double L[GCS_D_Z * GCS_D_Z];
  double h[GCS_D_Z];
} gcs_belief;

/* Certificate / diagnostic scalars of one scan (indices documented in DESIGN.md). */
#define GCS_CERT_LEN 64
typedef struct {
  gcs_belief belief;                 /* belief after AnchorDriftUpdate */
  double iw_process_dPsi[7 * 36];
  double iw_process_dnu[7];
  double z_t[6];                     /* post-recompose world pose used by the map update */
  double L_evidence[GCS_D_Z * GCS_D_Z];
  double h_evidence[GCS_D_Z];
  double R_mf[9];
  double t_wls[3];
  double cert[GCS_CERT_LEN];
  double stage_ms[8];                /* host-measured stage times */
  double iw_meas_dPsi[3 * 9];        /* measurement-noise IW statistics [gyro, accel, lidar] 3x3 blocks */
  double iw_meas_dnu[3];
  double L_imu_odom[GCS_D_Z * GCS_D_Z]; /* summed IMU/odometry evidence (pipeline.py:745-750), untempered */
  double h_imu_odom[GCS_D_Z];
  /* the eleven IMU/odometry certificates in all_certs order [odom, imu, imu_dep, gyro, preint, planar,
   * vz, odom_vel, odom_wz, kinematic, odom_dep], 7 fields each: [ess_total, support_frac, nll_per_ess,
   * lift_strength, psd_projection_delta, mass_epsilon_ratio, trust_alpha] */
  double imu_odom_certs[11 * 7];
} gcs_scan_outputs;

/* Inputs of the IMU/odometry evidence branch on its own (gcs_imu_odom_evidence): every quantity
 * the reference's _compute_imu_odom_branch reads (pipeline.py:595-776). */
typedef struct {
  int32_t m;                               /* IMU window length (>= 2) */
  const double *stamps, *gyro, *accel;     /* [m], [m*3], [m*3]; stamps <= 0 are padding */
  const double* w_int;                     /* scan-to-scan window weights [m] */
  double t_last_scan, t_scan, dt_sec;
  const double* pose0;                     /* belief_prev.mean_world_pose [6] */
  const double* pose_pred;                 /* belief_pred.mean_world_pose [6] */
  const double* mu_prev;                   /* belief_prev.mean_increment [22] */
  const double* mu_inc;                    /* belief_pred.mean_increment [22] */
  const double* gravity_W;                 /* [3], gravity scale applied */
  const double *Sigma_g, *Sigma_a;         /* [9] each */
  const double *odom_pose, *odom_cov_se3, *odom_twist, *odom_twist_cov;
  double planar_z_ref, planar_z_sigma, planar_vz_sigma;
} gcs_imu_odom_inputs;

/* ---------------------------------------------------------------- context */
const char* gcs_version(void);
int gcs_abi_version(void);
/* the reference's PipelineConfig / constants.py defaults (dense mode, B=48, cap 8192, K=16) */
int gcs_config_defaults(gcs_config* cfg);
int gcs_ctx_create(const gcs_config* cfg, gcs_ctx** out);
int gcs_ctx_destroy(gcs_ctx* ctx);
/* ctx NULL: the message of this thread's last failed gcs_ctx_create (e.g. an atlas the tiled bin
 * kernel cannot hold) */
const char* gcs_last_error(const gcs_ctx* ctx);
int gcs_ctx_set_stream(gcs_ctx* ctx, void* hip_stream);
int gcs_ctx_synchronize(gcs_ctx* ctx);
/* device stage timing: hipEvents stamped by the stages' own kernel dispatches on the context
 * stream.  stage_mask bit s enables stage s (0 = off): [0 point kernel (+ its fold when not
 * deferred), 1 sort+bucket, 2 bin moment-match kernel (+ fused Matrix-Fisher in scale mode),
 * 3 MF (dense / per-op), 4 planar, 5 pushforward, 6 budget kernel (row 1 mass sums),
 * 7 the bin kernel's partial-row fold (+ R_mf)].  Stages 6 + 0 + 2 + 7 are the
 * BinSoftAssign + ScanBinMomentMatch chain (bench.py roofline_chain).  Each timed stage costs a
 * few us of queue time. */
#define GCS_N_STAGES 8
int gcs_ctx_enable_timing(gcs_ctx* ctx, int32_t stage_mask);
/* Debug knobs (tests): GCS_DEBUG_SCAN_SPIN_LIMIT bounds k_scan's decoupled look-back spin (default
 * 1 << 22; when it runs out the scan returns GCS_ERR_HIP), GCS_DEBUG_INJECT_SCAN_FAIL != 0 makes
 * one look-back tile take that failure path on every scan. */
#define GCS_DEBUG_SCAN_SPIN_LIMIT 1
#define GCS_DEBUG_INJECT_SCAN_FAIL 2
/* GCS_DEBUG_SORTED_BUCKETS != 0: gcs_scan buckets points by the sorted path (k_scan, k_place,
 * k_bucket_rank) instead of the direct buckets; GCS_DEBUG_BUCKET_CAPACITY (4..32, multiple of 4)
 * lowers the direct buckets' row capacity so a test can force the overflow redo (cert[57] = 1). */
#define GCS_DEBUG_SORTED_BUCKETS 3
#define GCS_DEBUG_BUCKET_CAPACITY 4
/* (key 5 is not in use: gcs_ctx_set_debug answers "unknown debug key") */
/* GCS_DEBUG_POINT_KERNEL != 0: scale-mode scans run the round-3 point kernel (one wave per SIMD)
 * instead of k_points_lean (same arithmetic, bitwise the same outputs; A/B and its parity test). */
#define GCS_DEBUG_POINT_KERNEL 6
/* GCS_DEBUG_DEVICE_PREINT != 0 (or GCSLAM_DEVICE_PREINT=1): gcs_scan / gcs_scan_begin compute the
 * IMU window weights and the preintegration (deskew twist) on the device (k_preint) instead of the
 * host prologue.  A/B knob and its parity test. */
#define GCS_DEBUG_DEVICE_PREINT 7
/* GCS_DEBUG_PT_CLEAR (default 1; GCSLAM_PT_CLEAR=0 turns it off): gcs_scan's k_pt zeroes the next
 * scan's bucket counts and active-flag buffer, so that scan's k_budget only sums the weights; 0 keeps
 * the clears in k_budget (A/B knob and its bitwise test). */
#define GCS_DEBUG_PT_CLEAR 8
/* GCS_DEBUG_MIRROR_TORN (microseconds, 0 = off): the PT fold stores the scan mirror's sequence word
 * and checksum first and its data that long after, so the host meets a mirror whose data words have
 * not arrived; gcs_scan must re-read until the checksum matches (gcs_ctx_mirror_stats counts it) and
 * return the same results.  Test knob of the mirror guard. */
#define GCS_DEBUG_MIRROR_TORN 9
/* GCS_DEBUG_SENDBUF: where gcs_combine_allreduce's ncclAllReduce reads its send buffer.  -1 (default):
 * device memory when the communicator spans more than one rank (the packed payload is copied from the
 * pinned host buffer by the copy engine on the combine stream, so RCCL's ring kernels never read host
 * memory across PCIe inside the collective), the pinned host buffer itself at world size 1; 0: always
 * the host buffer; 1: always device memory (the world-1 test of the world > 1 path). */
#define GCS_DEBUG_SENDBUF 10
/* GCS_DEBUG_DEVICE_IMU_ODOM != 0 (or GCSLAM_DEVICE_IMU_ODOM=1): the step-9 IMU / odometry branch of gcs_scan /
 * gcs_scan_begin runs on the device (gcs_imu_odom_evidence_device's kernel) beside the bin path's kernels,
 * instead of the host C++ branch (the default). */
#define GCS_DEBUG_DEVICE_IMU_ODOM 11
/* GCS_DEBUG_COMBINE_DELAY (microseconds, 0 = off, at most 1,000,000): gcs_combine_allreduce queues a
 * kernel that waits this long on the combine stream ahead of ncclAllReduce -- the world-1 form of a
 * straggling peer rank.  A delay past the host poll's 20 ms sends the wait to its stream-synchronize
 * path (gcs_ctx_mirror_stats' payload syncs count it); the combined state must not change.  Test knob. */
#define GCS_DEBUG_COMBINE_DELAY 12
/* GCS_DEBUG_PUSH_DEFER (default 1; GCSLAM_PUSH_DEFER=0 turns it off): gcs_scan_combine submits the scan's
 * pushforward behind the combine's all-reduce and stage-out kernel instead of from the scan's tail; 0
 * keeps the tail's submit (the two-call API's order; A/B knob and its bitwise test). */
#define GCS_DEBUG_PUSH_DEFER 13
int gcs_ctx_set_debug(gcs_ctx* ctx, int32_t key, int64_t value);
/* The scan mirror (the PT fold's copy of the scan's scalars and device error words to pinned host
 * memory, with the scan's sequence number and a checksum; the host accepts it only when both match):
 * out[0] mirrors accepted, out[1] of them after at least one re-read (a data word arrived after the
 * sequence word), out[2] accepted only after the 20 ms poll gave up and the stream synchronized;
 * out[3..5] the same for the hypothesis all-reduce's stamped sum (gcs_combine_allreduce with a
 * communicator): all-reduces run, re-read, via stream sync. */
int gcs_ctx_mirror_stats(gcs_ctx* ctx, int64_t* out /*6*/);
/* Determinism diagnostics (tools/determinism_check.py, tests): 64-bit FNV-1a checksums of the
 * context's device state after its streams drain: [0] ScanBinStats, [1] MapBinStats, [2] derived map
 * stats, [3] touched bytes, [4] both active-flag buffers, [5] the bin kernel's partial rows, [6] the
 * device scalar block, [7] the host mirror's scalar block (device order; byte images). */
int gcs_debug_state_checksums(gcs_ctx* ctx, uint64_t* out /*8*/);
int gcs_ctx_stage_times(gcs_ctx* ctx, double* ms_sum /*GCS_N_STAGES*/, int64_t* counts /*GCS_N_STAGES*/,
                        int32_t reset);
/* The host split of every gcs_scan since the last reset, summed (ms): [0..7] the scan's stage_ms
 * (gcs_scan_outputs: pre-device, device submit + wait, tail, whole scan, budget launch + predict,
 * device launch calls, tail numerics, pushforward launch calls), [8] gcs_scan_combine's combine, [9]
 * gcs_scan_combine's whole call (which submits the pushforward from its combine unless GCS_DEBUG_PUSH_DEFER
 * is 0: its launch calls are then part of [8], not of [2] and [7]); *n the scans counted (n_combine[0]:
 * the combines).  Accumulated in the
 * library on every scan, so a caller's timed region decomposes exactly, with no per-scan reads. */
int gcs_ctx_host_split(gcs_ctx* ctx, double* ms_sum /*10*/, int64_t* n /*2*/, int32_t reset);
/* The same split per scan, for its distribution (p50 / p90 / max, slow scans): the latest
 * min(n_max, scans since the reset, 4096) scans, oldest first, 6 floats each -- [pre-device, device
 * submit + wait, tail, whole gcs_scan, combine, whole gcs_scan_combine call] in ms (the last two 0 for
 * a scan not run by gcs_scan_combine); *n_out the scans written. */
int gcs_ctx_host_split_history(gcs_ctx* ctx, float* out /*n_max*6*/, int32_t n_max, int32_t* n_out);
/* The OS thread id of the context's launch worker (0 before its first job): a caller that pins its
 * own thread can keep the worker off that core (bench.py). */
int64_t gcs_ctx_worker_tid(gcs_ctx* ctx);
int gcs_ctx_set_atlas(gcs_ctx* ctx, const double* dirs_host /*B*3*/);
int gcs_ctx_get_atlas(gcs_ctx* ctx, double* dirs_host /*B*3*/, int32_t* knn_host /*B*K*/);
int gcs_ctx_set_belief(gcs_ctx* ctx, const gcs_belief* b);
int gcs_ctx_get_belief(gcs_ctx* ctx, gcs_belief* b);
int gcs_ctx_set_map(gcs_ctx* ctx, const double* map_host /*26*B field-major*/);
int gcs_ctx_get_map(gcs_ctx* ctx, double* map_host /*26*B*/, double* derived_host /*16*B*/);
int gcs_ctx_get_scan_stats(gcs_ctx* ctx, double* scan_host /*26*B*/);
/* device pointers of the resident per-bin arrays (field-major, length-B rows) in DEVICE bin
 * order; set/get_map and get_scan_stats convert to reference (atlas) order.  scan_dev is
 * read-only for the caller: in scale mode the rows of bin tiles empty in consecutive scans are
 * left in place rather than rewritten. */
int gcs_ctx_device_arrays(gcs_ctx* ctx, double** scan_dev, double** map_dev, double** derived_dev);
/* order[device bin] = reference bin id (scale mode: Hilbert patches of the sphere; dense: identity) */
int gcs_ctx_get_bin_order(gcs_ctx* ctx, int32_t* order /*B*/);
int gcs_ctx_set_iw_state(gcs_ctx* ctx, const double* nu7, const double* Psi7x36);
int gcs_ctx_get_iw_state(gcs_ctx* ctx, double* nu7, double* Psi7x36, double* Q22x22);
/* measurement-noise IW state [gyro, accel, lidar] (structures/measurement_noise_iw_jax.py:29-68);
 * cert2 = [psd_delta, nu_delta] of the last apply in gcs_hypothesis_combine (may be NULL) */
int gcs_ctx_set_meas_iw_state(gcs_ctx* ctx, const double* nu3, const double* Psi3x9);
int gcs_ctx_get_meas_iw_state(gcs_ctx* ctx, double* nu3, double* Psi3x9, double* cert2);

/* ---------------------------------------------------------------- the per-scan pipeline */
int gcs_scan(gcs_ctx* ctx, const gcs_scan_inputs* in, gcs_scan_outputs* out);

/* ---------------------------------------------------------------- live primitive path
 * The same scan split around the live path's LiDAR evidence (FS/backend/pipeline.py:778-1011), which
 * the caller builds with the primitive-path entry points between the two calls:
 *   gcs_scan_begin: budget (device), PredictDiffusion, IMU window + preintegration, deskew (device:
 *     deskewed points / weights / budget timestamps into context-owned device arrays), the
 *     measurement-noise IW statistics and the IMU/odometry branch with its z_lin_pose (:751-755);
 *   the caller: extract_lidar_surfels on those arrays, recency inflation + map view at pose_pred,
 *     associate_primitives_ot, visual_pose_evidence at z_lin_pose -> L_lidar, h_lidar (:778-1011);
 *   gcs_scan_finish: evidence sum + power tempering with the LiDAR certificates' terms, excitation
 *     scaling, FusionScaleFromCertificates, InfoFusionAdditive, recompose, process IW statistics,
 *     AnchorDriftUpdate (:1038-1230, 1494-1502); no bin-map pushforward: the caller runs step 12b
 *     (the primitive map update) at out->z_t (:1232-1492).
 * Any context mode works (its bin atlas is not used). */
typedef struct {
  double z_lin_pose[6];          /* [t, rotvec] read by visual_pose_evidence (pipeline.py:755, :318-322) */
  double pose_pred[6];           /* belief_pred.mean_world_pose: the map branch's stencil centre (:801-802) */
  int32_t n_points;              /* rows of the arrays below (N_POINTS_CAP: selected rows + zero padding) */
  int32_t n_selected;
  /* in: caller-owned device buffers of N_POINTS_CAP rows, or NULL for the context's own (valid until
   * its next scan); out: the buffers written */
  double* points_dev;            /* [n_points*3] deskewed points */
  double* timestamps_dev;        /* [n_points] budget timestamps */
  double* weights_dev;           /* [n_points] deskewed weights */
  double deskew_ess;             /* the deskew certificate: ess_total (IMU preintegration ESS), */
  double deskew_support;         /* support_frac (retained weight fraction) */
  double cert[GCS_CERT_LEN];     /* the scan's certificate slots filled so far */
} gcs_scan_begin_outputs;

typedef struct {
  const double* L_lidar;         /* [22*22] visual_pose_evidence L_pose (build_visual_pose_evidence_22d) */
  const double* h_lidar;         /* [22] */
  double trigger_sum;            /* sum of total_trigger_magnitude over the map-branch certs (surfel,
                                    recency inflation, association) and the visual cert (pipeline.py:1211) */
  double ess_sum;                /* sum of support.ess_total over the LiDAR certs after deskew (surfel,
                                    association, visual; aggregate_certificates, pipeline.py:1049-1056) */
  int32_t n_certs;               /* their count */
  double nll_sum;                /* sum of mismatch.nll_per_ess over the same certs */
} gcs_lidar_evidence;

int gcs_scan_begin(gcs_ctx* ctx, const gcs_scan_inputs* in, gcs_scan_begin_outputs* out);
int gcs_scan_finish(gcs_ctx* ctx, const gcs_lidar_evidence* ev, gcs_scan_outputs* out);

/* ---------------------------------------------------------------- per-operator device entry points */
/* parse_pointcloud2_vlp16 (FS/backend/backend_node.py:377-468) + the no-TF base transform
 * (:1677-1680) on the device, over the raw message bytes: points_dev [n*3] f64 base frame (feed
 * gcs_scan with xyz_format = 1, point_step = 24), t_dev (s; ns converted when any value exceeds
 * 1e6), w_dev (range-sigmoid weights), ring_dev (u8, may be NULL).  Async on the context stream. */
int gcs_parse_pointcloud2(gcs_ctx* ctx, const void* data_dev, const gcs_pointcloud2_layout* layout,
                          double* points_dev, double* t_dev, double* w_dev, uint8_t* ring_dev);
/* PointBudgetResample + DeskewConstantTwist + directions + BinSoftAssign normalisers, fused.
 * Outputs (device, length n_points_cap; NULL to skip): deskewed points [cap*3], deskewed
 * weights, budget weights, nearest bin (scale mode).  cert_host receives scalars
 * [mass_in, mass_sel, mass_scale, sum_w_budget, sum_wn2, sum_w_deskew, sum_entropy, max_resp]. */
int gcs_point_stage(gcs_ctx* ctx, const void* xyz_dev, int32_t point_step, const double* t_dev, const double* w_dev,
                    int32_t n_points, double t0, double t1, const double* xi_body6,
                    double* p0_dev, double* w_out_dev, double* w_budget_dev, int32_t* nearest_dev, double* cert_host);
/* BinSoftAssign materialised for parity (scale: [cap*K] ids + responsibilities; dense: [cap*B]).
 * Requires a preceding gcs_point_stage on the same context. */
int gcs_bin_soft_assign(gcs_ctx* ctx, int32_t* ids_dev, double* resp_dev);
/* ScanBinMomentMatch (+Kappa) over the last point stage; writes the context's ScanBinStats
 * (gcs_ctx_device_arrays) and cert_host = [sum N, sum N^2, sum N/(N+eps), psd_delta, max eps ratio]. */
int gcs_scan_bin_moment_match(gcs_ctx* ctx, double* cert_host);
/* MatrixFisherRotation + PlanarTranslation over the context's scan and map stats.
 * mf_host  = [H(9), N_eff, map_scatter_total(9), map_N_dir_total, scan_N_total, R_mf(9), s(3), V(9)]
 * pt_host  = [L_full(9), h_full(3), N_eff] */
int gcs_matrix_fisher_rotation(gcs_ctx* ctx, double* mf_host);
int gcs_planar_translation(gcs_ctx* ctx, const double* R_hat9, double* pt_host);
/* PoseCovInflationPushforward of the context's scan stats into its map at pose z_t. */
int gcs_pushforward(gcs_ctx* ctx, const double* z_t6, const double* Sigma_pose36, double gamma);

/* ---------------------------------------------------------------- host-side numerics (no GPU) */
/* matrix orders n <= 24 (the 22-D state and its blocks); larger n returns GCS_ERR_ARG */
int gcs_psd_project(int32_t n, const double* M, double eps_psd, double* M_psd, double* cert6);
int gcs_spd_solve_lifted(int32_t n, const double* L, const double* b, double eps_lift, double* x);
int gcs_spd_inverse_lifted(int32_t n, const double* L, double eps_lift, double* Linv);
int gcs_svd3(const double* H, double* U, double* s, double* V);
/* The kernels' 3x3 DomainProjectionPSD (primitives.py:80-123; gcs_math.h psd_project3: exact-zero
 * and Cholesky fast paths, clamped-eigenpair deflation, Jacobi fallback), host build of the same
 * code; delta = ||M_psd - M_sym||_F. */
int gcs_psd_project3(const double* M /*3x3*/, double* M_psd /*3x3*/, double* delta);
/* Test entry: the bin kernel's tile dispatch order for per-tile active flags and staged-record counts
 * (n tiles; xcd != 0: grouped per XCD, n % 8 == 0), computed on `device` into order[n]. */
int gcs_debug_tile_order(int32_t device, const uint8_t* active, const uint32_t* work, int32_t n, int32_t xcd,
                         int32_t* order);
/* Test entry: k_preint on `device` over one IMU window (m samples; stamps[m], gyro/accel[m*3]):
 * smooth_window_weights(stamps, t0, t1, sigma) then preintegrate_imu_relative_pose_jax
 * (imu_preintegration.py:20-147) and the deskew twist se3_log(delta_pose) (pipeline.py:466-483;
 * rotation_only zeroes its translation).  out[16] = xi[6], ess, delta_pose[6], delta_v[3]. */
int gcs_debug_preintegrate(int32_t device, int32_t m, const double* stamps, const double* gyro, const double* accel,
                           double t0, double t1, double sigma, const double* rotvec /*3*/, const double* gyro_bias /*3*/,
                           const double* accel_bias /*3*/, const double* gravity /*3*/, int32_t rotation_only,
                           double* out /*16*/);
/* det-fixed Matrix-Fisher rotation R = U diag(1,1,det(UV^T)) V^T of H (matrix_fisher_evidence.py:215-222):
 * the same routine the device fold runs (polar Newton, SVD for reflections / rank deficiency) */
int gcs_mf_rotation(const double* H /*3x3*/, double* R /*3x3*/);
int gcs_predict_diffusion(const gcs_belief* prev, const double* Q, double dt_sec, gcs_belief* pred, double* cert4);
int gcs_info_fusion_additive(const gcs_belief* pred, const double* L_ev, const double* h_ev, double alpha,
                             gcs_belief* post, double* psd_delta);
int gcs_preintegrate_imu(int32_t m, const double* stamps, const double* gyro, const double* accel, const double* weights,
                         const double* rotvec_start, const double* gyro_bias, const double* accel_bias,
                         const double* gravity_W, double* delta_pose6, double* ess);
int gcs_belief_world_pose(const gcs_belief* b, double* pose6); /* belief.py:410-434 */
/* gyro + accel measurement-noise IW statistics of one IMU window (pipeline.py:522-566;
 * measurement_noise_iw_jax.py:130-218); w_int = scan-to-scan window weights, stamps <= 0 are padding */
/* _compute_imu_odom_branch (pipeline.py:595-776): L [22*22], h [22] (dependence scales applied);
 * cert = [trigger sum of the eleven certs, ess_imu_weighted, kappa, transport_sigma, imu scale,
 *         odom scale, mean reliability, odom nll, imu nll/ess, gyro nll, dt_int, dt_imu, omega_avg(3)] */
#define GCS_IMU_ODOM_CERT_LEN 15
int gcs_imu_odom_evidence(const gcs_imu_odom_inputs* in, double* L, double* h, double* cert);
/* The same branch on the device (gcs_imu_odom.hip k_imu_odom: one workgroup; window statistics, the
 * scan-to-scan preintegration and the IMU factor's medians and weighted sums in parallel, the eleven
 * factors' assembly -- the host branch's own code -- on lane 0) on ctx's stream for it, same outputs.
 * m <= 1024.  gcs_scan / gcs_scan_begin take it under GCS_DEBUG_DEVICE_IMU_ODOM / GCSLAM_DEVICE_IMU_ODOM=1. */
int gcs_imu_odom_evidence_device(gcs_ctx* ctx, const gcs_imu_odom_inputs* in, double* L, double* h, double* cert);
int gcs_imu_meas_iw_suffstats(int32_t m, const double* stamps, const double* gyro, const double* accel,
                              const double* w_int, const double* gyro_bias, const double* accel_bias,
                              const double* rotvec0, const double* gravity_W, double* dPsi3x9, double* dnu3);
/* measurement_noise_apply_suffstats_jax (measurement_noise_iw_jax.py:59-100) */
int gcs_meas_iw_apply(const double* nu3, const double* Psi3x9, const double* dPsi3x9, const double* dnu3,
                      double* nu_out, double* Psi_out, double* cert2);
int gcs_fibonacci_atlas(int32_t n_bins, double* dirs /*B*3*/);
int gcs_knn_table(int32_t n_bins, const double* dirs, int32_t k, int32_t* knn /*B*k*/);
int gcs_nearest_bins(int32_t n_bins, const double* dirs, int32_t n_query, const double* q /*n*3*/, int32_t* out);

/* ---------------------------------------------------------------- hypotheses (multi-GPU combine) */
/* Pack this hypothesis' contribution (weights pre-applied) for an RCCL sum all-reduce:
 * [w_iw dPsi 252 | w_iw dnu 7 | w_iw dPsi_meas 27 | w_iw dnu_meas 3 | w L 484 | w h 22 | w z 22 | w mu 22 | w |mu|^2 1] */
int gcs_hypothesis_payload(gcs_ctx* ctx, double w_iw, double w_bary, double* payload_host);
/* hypothesis_barycenter_projection (hypothesis.py:51-236) on host arrays, no context and no side
 * effects: weights floored at 0.0025 and renormalised, L = PSD(sum w L_k), h, z_lin = sum w (h, z).
 * cert6 = [psd_delta, floor_adjustment, ess = 1/sum w^2, support_frac, spread_proxy, cond] */
int gcs_hypothesis_barycenter(int32_t n_hyp, const double* L_stack /*n*484*/, const double* h_stack /*n*22*/,
                              const double* z_stack /*n*22*/, const double* weights /*n*/, double* L_out, double* h_out,
                              double* z_out, double* cert6);
/* process_noise_iw_apply_suffstats_jax (inverse_wishart_jax.py:126-185): state (nu7, Psi 7x36) <- apply
 * (dPsi, dnu); cert2 = [psd_delta, nu_delta].  process_noise_state_to_Q_jax (:35-68). */
int gcs_process_iw_apply(const double* nu7, const double* Psi7x36, const double* dPsi7x36, const double* dnu7,
                         double* nu_out, double* Psi_out, double* cert2);
int gcs_process_noise_Q(const double* nu7, const double* Psi7x36, double* Q22x22);
/* measurement_noise_mean_jax (IW mode, measurement_noise_iw_jax.py:38-56) of block idx (0 gyro, 1 accel, 2 lidar) */
int gcs_meas_iw_mode(const double* nu3, const double* Psi3x9, int32_t idx, double* Sigma3x3);
/* Runtime description of a context (RuntimeManifest, pipeline.py:1629-1793, for the bin path): JSON
 * with the library version, device, declared parameters (tau rule, K, cap, map mode, pushforward
 * form) and kernel set.  Writes at most len bytes (NUL-terminated); returns GCS_ERR_ARG if too short. */
int gcs_ctx_describe(gcs_ctx* ctx, char* buf, int32_t len);
/* Apply the summed payload: barycenter (PSD of L), process IW apply + Q rebuild and
 * measurement-noise IW apply (backend_node.py:2102-2119; both stored in ctx).
 * combined_out may be NULL; cert_out = [psd_delta, spread, iw_psd_delta, iw_nu_delta]. */
int gcs_hypothesis_combine(gcs_ctx* ctx, const double* payload_sum, int32_t scan_count, gcs_belief* combined_out,
                           double* cert_out);

/* The node's initial noise states (create_datasheet_process_noise_state,
 * structures/inverse_wishart_jax.py:42-80; create_datasheet_measurement_noise_state,
 * structures/measurement_noise_iw_jax.py:37-68): process nu[7], Psi[7*36]; measurement nu[3], Psi[3*9]. */
int gcs_datasheet_noise_states(double* nu7, double* Psi252, double* mnu3, double* mPsi27);

/* Context-free forms of the same payload (host numerics, no GPU): pack one hypothesis' contribution
 * (any stats pointer may be NULL = zeros) and apply a summed payload to explicit IW states. */
int gcs_payload_pack(const gcs_belief* b, const double* dPsi252, const double* dnu7, const double* meas_dPsi27,
                     const double* meas_dnu3, double w_iw, double w_bary, double* payload /*840*/);
int gcs_payload_apply(const double* payload_sum, int32_t scan_count, const double* X_anchor6, double stamp_sec,
                      const double* nu7, const double* Psi7x36, const double* meas_nu3, const double* meas_Psi3x9,
                      gcs_belief* combined_out /*may be NULL*/, double* nu_out, double* Psi_out, double* Q_out,
                      double* meas_nu_out, double* meas_Psi_out, double* cert4);

/* ---------------------------------------------------------------- RCCL (one rank per GPU) */
/* The per-scan hypothesis exchange (backend_node.py:1999-2119, hypothesis.py:92-115):
 * gcs_combine_allreduce packs this context's payload, sum-all-reduces it over the RCCL communicator
 * on the context stream (xGMI between MI355X GPUs), and applies the combine + IW updates, so every
 * rank holds bitwise-identical Q and IW states.  comm NULL = a single rank (no exchange).  The
 * communicator comes from gcs_rccl_comm_init with an id from gcs_rccl_get_unique_id on one rank,
 * broadcast by the launcher. */
#define GCS_RCCL_ID_BYTES 128
int gcs_rccl_get_unique_id(uint8_t* id /*GCS_RCCL_ID_BYTES*/);
int gcs_rccl_comm_init(int32_t device, int32_t n_ranks, int32_t rank, const uint8_t* id, void** comm);
int gcs_rccl_comm_destroy(void* comm);
/* Ranks the communicator holds (ncclCommCount) and this rank's index in it (ncclCommUserRank):
 * bench.py reports them so a multi-GPU line shows RCCL saw every rank. */
int gcs_rccl_comm_count(void* comm, int32_t* count, int32_t* user_rank);
/* In-place ncclBroadcast of `bytes` bytes of device memory from rank `root` on `stream` (NULL: the
 * device's null stream), then a stream synchronize: the live primitive map's per-scan update record
 * (gcslam.distributed.MapRecordChannel, ~0.5 MB at the reference sizes) from the lead to the ranks
 * that replay it (backend_node.py:2079-2083). */
int gcs_rccl_broadcast(void* comm, void* buf, int64_t bytes, int32_t root, void* stream);
/* gcs_scan then gcs_combine_allreduce in one call (the node's per-scan step, backend_node.py:2036-2119,
 * without a caller round trip between them); combine_ms (may be NULL): the combine's host wall time. */
int gcs_scan_combine(gcs_ctx* ctx, const gcs_scan_inputs* in, gcs_scan_outputs* out, void* comm, double w_iw,
                     double w_bary, int32_t scan_count, gcs_belief* combined_out, double* cert /*4*/,
                     double* combine_ms);
int gcs_combine_allreduce(gcs_ctx* ctx, void* comm, double w_iw, double w_bary, int32_t scan_count,
                          gcs_belief* combined_out /*may be NULL*/, double* cert4 /*may be NULL*/);


/* ---------------------------------------------------------------- one map for all hypotheses */
/* The reference node keeps ONE map: every hypothesis of a scan reads self.primitive_map and only
 * hypothesis 0's update is stored (backend_node.py:2036-2083).  With one hypothesis per GPU each
 * context holds a copy of that map:
 *   GCS_MAP_OWN (default)  every context updates its own map from its own scan (per-hypothesis maps,
 *                          no map traffic; declared);
 *   GCS_MAP_LEAD           hypothesis 0: updates its map and keeps the scan's map-update record
 *                          [deskew twist 6 | z_t 6 | pose covariance 6x6] (GCS_MAP_REC_LEN f64);
 *   GCS_MAP_FOLLOW         hypotheses 1..: gcs_scan skips its own pushforward, and gcs_map_follow
 *                          replays the lead's update on the same raw scan (point + bin stage at the
 *                          lead's twist, pushforward at the lead's z_t and covariance), so the map
 *                          stays bitwise the lead's.  No map rows move between GPUs: the record rides
 *                          the per-scan payload all-reduce (GCS_PAYLOAD_LEN + GCS_MAP_REC_LEN f64,
 *                          the lead's record plus zeros) when every rank's context is LEAD or FOLLOW.
 * A follower's scan s reads the map after the lead's scan s - 1 (declared lag: the reference's
 * sequential loop lets hypothesis k > 0 read hypothesis 0's update of the same scan). */
#define GCS_MAP_OWN 0
#define GCS_MAP_LEAD 1
#define GCS_MAP_FOLLOW 2
#define GCS_MAP_REC_LEN 48
int gcs_ctx_set_map_mode(gcs_ctx* ctx, int32_t mode);
/* the last gcs_scan's map-update record (any mode) */
int gcs_ctx_map_record(gcs_ctx* ctx, double* rec /*GCS_MAP_REC_LEN*/);
/* replay the lead's update of this scan (in: the scan's gcs_scan inputs; only the point stream,
 * the scan window and n_points are read); rec NULL = the record the last gcs_combine_allreduce
 * carried from the lead (a single rank, comm NULL: its own record -- bench.py --map-mode follow times
 * a follower's scan on one GPU that way) */
int gcs_map_follow(gcs_ctx* ctx, const gcs_scan_inputs* in, const double* rec /*GCS_MAP_REC_LEN or NULL*/);

/* ---------------------------------------------------------------- primitive path: LiDAR surfels */
/* extract_lidar_surfels (lidar_surfel_extraction.py:339-431) on the GPU: sentinel mask and weighted
 * centre, MA-hex 3D hash-grid cell of every point (ma_hex_web.py:221-303), the first max_occupants
 * points of each cell in index order (stable radix sort by cell), one weighted plane fit per cell
 * (3x3 eigh, Wishart-regularised covariance, kappa; :84-163), the valid cells in cell-id order
 * into n_surfel slots (:297-321) and the LiDAR slice of the MeasurementBatch in information form
 * (measurement_batch.py:298-331).  A surfel context owns the workspace for up to max_points points
 * on one GPU; calls on one context must be serialised. */
typedef struct gcs_surfel_ctx gcs_surfel_ctx;

typedef struct {
  int32_t n_surfel;                   /* lidar_surfel_extraction.py:46 (GC_N_SURFEL = 1024) */
  int32_t n_feat;                     /* :47 (GC_N_FEAT = 512): the LiDAR slice starts there */
  double voxel_size_m;                /* :48 */
  int32_t num_cells_1, num_cells_2, num_cells_z, max_occupants;  /* :50-53 (32, 32, 8, 32) */
  int32_t min_points_per_voxel;       /* :54 */
  double sensor_noise_var_per_axis;   /* :55 */
  double wishart_nu, wishart_psi_scale;          /* :56-57 */
  double kappa_main_scale, kappa_min, kappa_max; /* :58-60 */
  double eig_min;                     /* :61 */
  double eps_lift;                    /* :62 (GC_EPS_LIFT) */
  int32_t max_points;                 /* capacity of the context (points per call) */
  int32_t device;
} gcs_surfel_config;

/* Outputs: device pointers, each may be NULL (not written).  Row counts: n_surfel unless noted.
 * Slots past n_valid hold the reference's padding (positions / normals / kappas / weights /
 * timestamps 0, covariances I; batch rows 0, cell_ids -1). */
typedef struct {
  double* positions;     /* n_surfel x 3   surfel centroids (lidar_surfel_extraction.py:307) */
  double* covariances;   /* n_surfel x 9   Wishart-regularised Sigma */
  double* normals;       /* n_surfel x 3 */
  double* kappas;        /* n_surfel */
  double* weights;       /* n_surfel       sum of member weights */
  double* timestamps;    /* n_surfel */
  double* Lambdas;       /* n_surfel x 9   MeasurementBatch LiDAR slice: inv(Sigma + eps_lift I) */
  double* thetas;        /* n_surfel x 3   Lambda mu */
  double* etas;          /* n_surfel x 3 lobes x 3: lobe 0 = kappa n, others 0 */
  double* colors;        /* n_surfel x 3   grey from normal z (measurement_batch.py:262-269) */
  uint8_t* valid_mask;   /* n_surfel */
  int32_t* source_indices; /* n_surfel */
  int32_t* cell_ids;     /* n_surfel       MA-hex cell of each slot (-1 past n_valid) */
  int32_t* bucket;       /* n_cells x max_occupants point indices (-1 padding) */
  int32_t* count;        /* n_cells        occupancy clipped to max_occupants */
  int32_t* sources;      /* n_surfel       MeasurementBatch sources of the LiDAR slice: 1 on valid rows (the
                            rows past n_valid are not written) */
  /* host results */
  double center[3];      /* the weighted centre the cells are hashed around (:264-267) */
  int32_t n_valid;       /* surfels in the LiDAR slice */
  double cert[2];        /* SupportCert: ess_total = n_valid, support_frac = n_valid / n_surfel */
} gcs_surfel_outputs;

int gcs_surfel_config_defaults(gcs_surfel_config* cfg);
int gcs_surfel_ctx_create(const gcs_surfel_config* cfg, gcs_surfel_ctx** out);
int gcs_surfel_ctx_destroy(gcs_surfel_ctx* ctx);
const char* gcs_surfel_last_error(const gcs_surfel_ctx* ctx);
/* stream: a hipStream_t (NULL = the context's own); work on it is ordered after the caller's */
int gcs_surfel_ctx_set_stream(gcs_surfel_ctx* ctx, void* stream);
/* points: n x 3 f64, timestamps / weights: n f64 (device); n <= max_points.  Synchronises. */
int gcs_extract_lidar_surfels(gcs_surfel_ctx* ctx, const double* points_dev, const double* timestamps_dev,
                              const double* weights_dev, int32_t n, gcs_surfel_outputs* out);

/* ---------------------------------------------------------------- primitive path: camera splats */
/* The camera half of the node's per-scan batch (backend_node.py:1865-1925) on the GPU: LiDAR points
 * to the camera frame and the image (lidar_camera_depth_fusion.py:80-96), per visual feature the
 * LiDAR depth evidence along its pixel ray -- Route A, the robust depth sample of the points within
 * lidar_projection_radius_pix (:99-164), and Route B, the ray / plane intersection with the plane
 * of the nearest points (:242-386) -- the product of experts with the camera's depth
 * (splat_prep.py:37-134), the back-projection with its closed-form covariance (:450-489), the move
 * to the base frame (backend_node.py:1887-1918) and rows [0, n_feat) of the MeasurementBatch in
 * information form (camera_batch_utils.py:23-86, measurement_batch.py:165-259).  Route B's plane
 * fits are uniformly weighted (splat_prep_fused passes no point weights).  A context owns the
 * workspace for up to max_points points on one GPU; calls on one context must be serialised. */
typedef struct gcs_camsplat_ctx gcs_camsplat_ctx;

typedef struct {
  /* LidarCameraDepthFusionConfig (lidar_camera_depth_fusion.py:29-63), same names and defaults */
  double depth_fusion_weight_camera, depth_fusion_weight_lidar, gamma_lidar;
  double lidar_projection_radius_pix;
  int32_t lidar_plane_fit_min_points;
  double lidar_depth_base_sigma_m, lidar_incidence_sigma_scale, depth_var_min_m2;
  double point_support_n0, point_support_alpha, spread_mad_beta, repr_gamma;
  int32_t lidar_ray_plane_fit_max_points;   /* at most 64: one lane of a wave per fitted point */
  double plane_intersection_delta, plane_angle_sigmoid_alpha, plane_angle_sigmoid_t;
  double plane_planarity_sigmoid_beta, plane_planarity_rho0, plane_residual_exp_gamma, plane_fit_eps;
  double depth_min_m, depth_sigma_max_sq, depth_min_sigmoid_alpha_z;
  /* splat_prep_fused / feature_list_to_camera_batch arguments */
  double pixel_sigma;            /* splat_prep.py:43 (1.0) */
  double eps_lift;               /* GC_EPS_LIFT */
  int32_t n_feat, n_surfel;      /* the batch's budgets: the call writes rows [0, n_feat) */
  int32_t max_points;            /* capacity of the context (points per call) */
  int32_t max_candidates;        /* points within the radius of one feature held at once (<= 1024) */
  int32_t device;
} gcs_camsplat_config;

/* One call's inputs.  Pointers are device arrays (f64 unless noted); extrinsics, intrinsics and the
 * batch's timestamp are host values. */
typedef struct {
  const double* points_base;     /* n_points x 3, base frame (gcs_scan_begin's deskewed points) */
  int32_t n_points;
  double R_base_camera[9], t_base_camera[3];   /* p_base = R p_camera + t */
  double fx, fy, cx, cy;
  int32_t n_features;            /* M */
  const double *u, *v;           /* M pixel coordinates */
  const double *depth_Lambda_c, *depth_theta_c;   /* M: the camera's depth in natural form (0: none) */
  const double *xyz, *cov;       /* M x 3, M x 9: camera-frame splat, kept where fusion does not apply */
  const double *weight, *kappa_app;   /* M */
  const double* mu_app;          /* M x 3 (camera frame) */
  const uint8_t* has_mu;         /* M: 0 = the view direction xyz / |xyz| takes mu_app's place */
  const double* color;           /* M x 3 RGB */
  const uint8_t* has_color;      /* M: 0 = grey 0.5 */
  double timestamp_sec;
} gcs_camsplat_inputs;

/* Outputs: device pointers.  The batch arrays have n_feat rows (the camera slice) and are all written:
 * rows [0, n_camera_valid) from the first min(M, n_feat) features, the rest zeros.  The per-feature
 * diagnostics (M rows) may each be NULL. */
typedef struct {
  double* Lambdas;         /* n_feat x 9   inv(Sigma_base + eps_lift I) */
  double* thetas;          /* n_feat x 3 */
  double* etas;            /* n_feat x 3 lobes x 3: lobe 0 = kappa_app * direction */
  double* weights;         /* n_feat */
  int32_t* sources;        /* n_feat       0 = camera */
  int32_t* source_indices; /* n_feat */
  uint8_t* valid_mask;     /* n_feat */
  double* timestamps;      /* n_feat */
  double* colors;          /* n_feat x 3   clipped to [0, 1] */
  int32_t* n_pt;           /* M  points within the radius */
  double *z_med, *mad;     /* M  Route A's median depth and MAD (NaN below lidar_plane_fit_min_points) */
  double *Lambda_A, *theta_A, *Lambda_B, *theta_B;   /* M  lidar_depth_evidence's return_diag */
  double* z_f;             /* M  fused depth (0 where the input splat is kept) */
  uint8_t* fused;          /* M  1 = fused, 0 = the input splat kept (splat_prep.py:85-93) */
  /* host result */
  int32_t n_camera_valid;  /* min(M, n_feat) */
} gcs_camsplat_outputs;

int gcs_camsplat_config_defaults(gcs_camsplat_config* cfg);
int gcs_camsplat_ctx_create(const gcs_camsplat_config* cfg, gcs_camsplat_ctx** out);
int gcs_camsplat_ctx_destroy(gcs_camsplat_ctx* ctx);
const char* gcs_camsplat_last_error(const gcs_camsplat_ctx* ctx);
/* stream: a hipStream_t (NULL = the context's own); work on it is ordered after the caller's */
int gcs_camsplat_ctx_set_stream(gcs_camsplat_ctx* ctx, void* stream);
/* Synchronises.  GCS_ERR_STATE when a feature has more than max_candidates points within its radius
 * (the message names the first such feature): every batch row is then zero / invalid and
 * n_camera_valid 0 -- nothing is truncated silently. */
int gcs_camera_splats(gcs_camsplat_ctx* ctx, const gcs_camsplat_inputs* in, gcs_camsplat_outputs* out);
/* The same on the scan's own records -- the points splat_prep_fused sees in the node are the scan's
 * base-frame points, not the deskewed ones (backend_node.py:1872-1884): xyz_dev is what
 * gcs_scan_inputs.xyz_dev holds.  xyz_format 0: float32 x, y, z at bytes 0, 4, 8 of a point_step-byte
 * record (point_step >= 12, a multiple of 4); xyz_format 1: float64 at bytes 0, 8, 16 (point_step >= 24, a
 * multiple of 8).  in->points_base and in->n_points are ignored.  Widening float32 is exact: the results
 * are bit for bit those of gcs_camera_splats on the float64 array of the same values. */
int gcs_camera_splats_scan(gcs_camsplat_ctx* ctx, const gcs_camsplat_inputs* in, const void* xyz_dev,
                           int32_t point_step, int32_t xyz_format, int32_t n_points, gcs_camsplat_outputs* out);

/* ---------------------------------------------------------------- primitive path: visual features */
/* The visual feature node's per-keypoint numerics (src/visual_feature_node.cpp:493-652 on_rgbd, after
 * ORB) on the GPU, from a depth image and a keypoint list to the feature arrays gcs_camsplat_inputs
 * reads: the robust depth sample (:228-348: nearest, median3, median5, hex), the Student-t effective
 * variance (:350-369, :563-572), the 6-parameter quadratic surface fit with its normal, Gaussian
 * curvature and smallest Hessian eigenvalue (:401-491), the back-projection and its closed-form
 * covariance (:371-399), the medial-axis covariance inflation, the vMF kappa, the weights and the
 * colour (:546-641), and _feature_batch_to_list's renormalised mu_app (backend_node.py:1589-1650).
 * One wave64 per keypoint, one lane per window pixel, all f64; the median is an input value picked
 * by rank (element n / 2 of the sorted valid values, ties by lane) and the normal equations are
 * butterfly sums in a fixed order, so two calls agree bit for bit.  kp_u, kp_v, kp_response are
 * cv::KeyPoint's pt.x, pt.y, response: from any detector of the caller's, or from gcs_detect_keypoints
 * below, the library's own FAST-9 / Harris detector at pyramid level 0 (the pyramid, the orientation and the
 * descriptors are entries of their own further below; none of them claims parity with cv::ORB).
 * Declared where the node leaves it open: with n_keypoints > max_features the max_features largest
 * responses are kept (ties to the lower index, NaN last) and written in input order; a keypoint with
 * a non-finite u or v, or |u| or |v| > 1e9, is outside the image; a NaN response weighs 0.  A keypoint
 * without a valid depth still yields a feature (xyz 0, cov invalid_cov_inflate I, weight 0).
 * Calls on one context must be serialised. */
typedef struct gcs_visfeat_ctx gcs_visfeat_ctx;
#define GCS_VF_NEAREST 0
#define GCS_VF_MEDIAN3 1
#define GCS_VF_MEDIAN5 2
#define GCS_VF_HEX 3
#define GCS_VF_DEPTH_LINEAR 0
#define GCS_VF_DEPTH_QUADRATIC 1

typedef struct {
  /* the node's parameters (:70-103), same names and defaults */
  int32_t max_features;          /* 512: rows of every output array */
  int32_t depth_sample_mode;     /* GCS_VF_MEDIAN3 */
  int32_t depth_model;           /* GCS_VF_DEPTH_LINEAR */
  int32_t hex_radius;            /* 2; below 1 behaves as 1 (:303), at most 32 */
  int32_t quad_fit_radius;       /* 2; below 1 behaves as 1 (:407), at most 3: (2r + 1)^2 <= 49 lanes */
  int32_t quad_fit_min_points;   /* 6 */
  double pixel_sigma, depth_sigma0, depth_sigma_slope, min_depth_m, max_depth_m, depth_validity_slope;
  double response_soft_scale, depth_scale;
  double cov_reg_eps;            /* declared by the node, read nowhere in it */
  double invalid_cov_inflate;
  double quad_fit_lstsq_eps, student_t_nu, student_t_w_min, ma_tau, ma_delta_inflate;
  double kappa0, kappa_alpha, kappa_max, kappa_min;
  int32_t max_keypoints;         /* 4096: capacity of the context (keypoints per call), >= max_features */
  int32_t device;
} gcs_visfeat_config;

/* One frame.  Device pointers for gcs_visual_features, host pointers for gcs_visual_features_host. */
typedef struct {
  const void* depth;             /* height rows of width values, depth_pitch bytes apart */
  int32_t depth_format;          /* 0: float32, 1: uint16; metres = value * depth_scale */
  int64_t depth_pitch;           /* >= width * (4 or 2), a multiple of the value's size */
  int32_t width, height;
  const uint8_t* rgb;            /* rgb8, rows rgb_pitch (>= 3 width) bytes apart; NULL: no colour */
  int64_t rgb_pitch;
  double fx, fy, cx, cy;         /* camera_K (:103) */
  int32_t n_keypoints;           /* <= max_keypoints */
  const float *kp_u, *kp_v, *kp_response;   /* n_keypoints */
} gcs_visfeat_inputs;

/* Outputs: max_features rows each, rows [count, max_features) zeros (kp_index -1).  The twelve feature
 * arrays are gcs_camsplat_inputs' arrays; the diagnostics may each be NULL. */
typedef struct {
  double *u, *v;                 /* the keypoint's coordinates, widened */
  double* xyz;                   /* x 3, camera frame */
  double* cov;                   /* x 9 */
  double *weight, *kappa_app;
  double* mu_app;                /* x 3: the fit's normal / (|normal| + 1e-12); zeros without a fit */
  uint8_t* has_mu;               /* 1 exactly where the fit exists */
  double* color;                 /* x 3: rgb / 255 at the clamped, rounded (u, v); zeros without an image */
  uint8_t* has_color;            /* 1 when rgb was given */
  double *depth_Lambda_c, *depth_theta_c;   /* 1 / var_z_eff and z / var_z_eff (0 without a depth) */
  /* diagnostics */
  int32_t* kp_index;             /* the keypoint each row came from */
  uint8_t* z_valid;
  int32_t* n_depth;              /* valid values in the depth sample */
  int32_t* n_fit;                /* valid pixels in the fit window (0 where the depth is invalid) */
  double* z_m;                   /* the sampled depth (NaN where invalid) */
  double* z_var;                 /* the sample's own variance, NaN where the node has none */
  double* var_z_eff;
  double* beta;                  /* x 6: the fit's coefficients (NaN without a fit, as K, lam_min, w_ma) */
  double *K, *lam_min, *w_ma;
  /* host result */
  int32_t count;                 /* min(n_keypoints, max_features) */
} gcs_visfeat_outputs;

int gcs_visfeat_config_defaults(gcs_visfeat_config* cfg);
/* GCS_ERR_ARG, before any device call, for quad_fit_radius > 3, hex_radius > 32, max_features < 1,
 * max_keypoints < max_features or an unknown depth_sample_mode / depth_model. */
int gcs_visfeat_ctx_create(const gcs_visfeat_config* cfg, gcs_visfeat_ctx** out);
int gcs_visfeat_ctx_destroy(gcs_visfeat_ctx* ctx);
const char* gcs_visfeat_last_error(const gcs_visfeat_ctx* ctx);
/* stream: a hipStream_t, NULL being HIP's default stream, which is also what a new context queues on (the
 * call does not synchronise, so unlike the contexts above this one has no stream of its own to hide behind:
 * the work is ordered with the caller's work on the stream it names) */
int gcs_visfeat_ctx_set_stream(gcs_visfeat_ctx* ctx, void* stream);
/* Queues its kernels on the context's stream and returns: count is known on the host, nothing is waited
 * for.  The arrays are ready for work queued later on the same stream. */
int gcs_visual_features(gcs_visfeat_ctx* ctx, const gcs_visfeat_inputs* in, gcs_visfeat_outputs* out);
/* The same rows on the host (no device, no context): every pointer is a host array. */
int gcs_visual_features_host(const gcs_visfeat_config* cfg, const gcs_visfeat_inputs* in,
                             gcs_visfeat_outputs* out);

/* ---------------------------------------------------------------- primitive path: keypoint detector */
/* Keypoints from an 8-bit image on the GPU, in the form gcs_visfeat_inputs reads.  This detector is the
 * project's own.  It follows the published FAST / ORB recipe, but it claims no parity with cv::ORB: there
 * is no pyramid here (ORB's nlevels = 8, scaleFactor = 1.2: gcs_detect_keypoints_pyramid, below), and the
 * orientation and the descriptors are operators of their own (gcs_describe_keypoints, further below).  Everything is exact integer arithmetic except the last step of the response:
 *  1. grey: gray8 as it is; rgb8 as g = (4899 R + 9617 G + 1868 B + 8192) >> 14.
 *  2. FAST-9/16 score: the ring is the radius-3 Bresenham circle, clockwise from the top: (0,-3) (1,-3)
 *     (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3).
 *     With d_j = I(ring_j) - I(p), m(p) = max over the 16 arcs of 9 consecutive ring positions of
 *     max(min_arc d_j, min_arc -d_j); p (3 <= x < W - 3, 3 <= y < H - 3) is a corner when
 *     m(p) > fast_threshold and its score is then m(p); every other pixel's score is 0.
 *  3. suppression: a corner survives when its score is strictly greater than its 8 neighbours' scores
 *     (two adjacent corners of equal score both go); neighbours outside the border of 4. compete.
 *  4. border: survivors with edge_threshold <= x < W - edge_threshold, and the same in y, are kept; an
 *     image too small to hold one such pixel yields zero keypoints and is not an error.
 *  5. response: over the 7 x 7 block around the survivor, with Ix, Iy the 3 x 3 Sobel derivatives of the
 *     grey image as integers, a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy (int64);
 *     r = ((double)(a b - c c) - harris_k (double)((a + b)(a + b))) s^4, s = 1.0 / (4 * 7 * 255), every
 *     operation rounded on its own, s^4 formed as ((s s) s) s, the result rounded once to float32
 *     (ORB's Harris score with its scale: about 1e-4 .. 1e-2).
 *  6. selection: with more than max_keypoints survivors exactly the max_keypoints largest by (response
 *     descending, raster index y W + x ascending) are kept.  Output is always in raster order, kp_u = x,
 *     kp_v = y; rows [n_keypoints, max_keypoints) of the three arrays are NaN, which
 *     gcs_visual_features ranks last, weighs 0 and treats as outside the image, so a caller may chain
 *     with n_keypoints = max_keypoints and no wait.
 * No intermediate capacity exists that an image could overflow: the only buffers sized by the image are
 * per-pixel, and the selection is a radix select over the per-pixel key image.  No kernel reads outside
 * [0, W) x [0, H) of the input.  Calls on one context must be serialised. */
typedef struct gcs_keypoint_ctx gcs_keypoint_ctx;

typedef struct {
  int32_t fast_threshold;        /* 20 (ORB's fastThreshold); 0 .. 255 */
  int32_t edge_threshold;        /* 31 (ORB's edgeThreshold); >= 4 */
  int32_t max_keypoints;         /* 4096; 1 .. 65536 (gcs_visfeat_config.max_keypoints' range) */
  int32_t max_width, max_height; /* 1920 x 1080: capacity of the per-pixel workspace (at most 2^28 pixels) */
  double harris_k;               /* 0.04; finite */
  int32_t device;
} gcs_keypoint_config;

/* One image.  Device pointers for gcs_detect_keypoints, host pointers for gcs_detect_keypoints_host. */
typedef struct {
  const uint8_t* image;          /* height rows, pitch bytes apart */
  int32_t channels;              /* 1: gray8, 3: rgb8 */
  int64_t pitch;                 /* >= channels * width */
  int32_t width, height;         /* >= 1, at most the context's max_width, max_height */
} gcs_keypoint_inputs;

typedef struct {
  float *kp_u, *kp_v, *kp_response;   /* max_keypoints each */
  int32_t* counts;               /* 4: n_keypoints, n_survivors (after the border, before the cap), n_corners
                                    (pixels with a non-zero score), 0 */
} gcs_keypoint_outputs;

int gcs_keypoint_config_defaults(gcs_keypoint_config* cfg);
/* GCS_ERR_ARG, before any device call, for a config outside the ranges above. */
int gcs_keypoint_ctx_create(const gcs_keypoint_config* cfg, gcs_keypoint_ctx** out);
int gcs_keypoint_ctx_destroy(gcs_keypoint_ctx* ctx);
const char* gcs_keypoint_last_error(const gcs_keypoint_ctx* ctx);
/* stream: as gcs_visfeat_ctx_set_stream -- the context queues on the caller's stream and waits for nothing */
int gcs_keypoint_ctx_set_stream(gcs_keypoint_ctx* ctx, void* stream);
/* Queues its kernels on the context's stream and returns; counts is a device array like the others.
 * GCS_ERR_ARG, before any device call, for channels not 1 or 3, width or height < 1 or above the
 * context's capacity, pitch < channels * width, or a null array. */
int gcs_detect_keypoints(gcs_keypoint_ctx* ctx, const gcs_keypoint_inputs* in, gcs_keypoint_outputs* out);
/* The same steps on the host (no device, no context): every pointer is a host array. */
int gcs_detect_keypoints_host(const gcs_keypoint_config* cfg, const gcs_keypoint_inputs* in,
                              gcs_keypoint_outputs* out);

/* Keypoints over a scale pyramid: the detector above on n_levels images, each level with its own share of
 * max_keypoints, every keypoint in level-0 pixel coordinates (what ORB's nlevels = 8, scaleFactor = 1.2 adds
 * to the detector front; orientation and descriptors: gcs_describe_keypoints; no parity with cv::ORB).  The definition is
 * the project's own and is integer-exact wherever the one above is.  With W x H the input, L = n_levels,
 * K = max_keypoints and the scale factor the rational scale_num / scale_den (no pow, no floating-point
 * scale anywhere):
 *  P1. level sizes: with N = scale_num^l and D = scale_den^l, W_l = (2 W D + N) / (2 N) in integer division
 *      (W D / N rounded half up), H_l likewise.  A level with W_l < 1 or H_l < 1 has no pixels and yields no
 *      keypoints; that is not an error.
 *  P2. level images: level 0 is step 1's grey image.  Level l >= 1 is the exact pixel-area resample of level
 *      0 (not of level l - 1).  Per axis, in units of 1 / W_l of a source pixel, destination pixel x covers
 *      [x W, (x + 1) W) and source pixel j covers [j W_l, (j + 1) W_l); wx(x, j) is the integer length of
 *      their overlap (sum over j: W), wy the same with H and H_l, and
 *      I_l(x, y) = (sum_{j,i} wx(x, j) wy(y, i) I_0(j, i) + (W H) / 2) / (W H) in int64, integer division.
 *  P3. per level: steps 2-5 above on I_l at W_l x H_l, with the same fast_threshold, the same edge_threshold
 *      in that level's pixels and the same harris_k.
 *  P4. quotas: w_l = scale_den^l scale_num^(L - 1 - l); quota_l = (K w_l) / sum(w) (integer division) for
 *      l >= 1 and quota_0 = K - sum_{l >= 1} quota_l.  Quotas do not depend on the image and an unused share
 *      is not handed on.  Level l keeps its quota_l best by step 6's rule (response descending, raster index
 *      y W_l + x ascending, the same tie handling); a quota of 0 keeps nothing.
 *  P5. output: rows in (level ascending, raster index ascending) order;
 *      kp_u = (float)((double)((2 x + 1) W) / (double)(2 W_l) - 0.5), kp_v likewise with H: the integers are
 *      exact, the division and the subtraction are each rounded on their own, then once to float32 (at level
 *      0 this is x exactly).  kp_response is the level's own response, unscaled; kp_level the row's level.
 *      Rows [n_keypoints, max_keypoints) are NaN in the three float arrays and -1 in kp_level, so the chain
 *      into gcs_visual_features with n_keypoints = max_keypoints and no wait works as above.
 * With n_levels = 1 every byte equals gcs_detect_keypoints' with the same six fields; the level-0 rows equal
 * gcs_detect_keypoints with max_keypoints = quota_0.  The number of kernel launches of a call does not depend
 * on n_levels.  max_width x max_height is the capacity for level 0; the other levels' workspace follows from
 * it.  Calls on one context must be serialised. */
typedef struct gcs_keypoint_pyramid_ctx gcs_keypoint_pyramid_ctx;
#define GCS_KEYPOINT_MAX_LEVELS 8

typedef struct {
  int32_t fast_threshold;        /* the six fields of gcs_keypoint_config, same defaults and ranges */
  int32_t edge_threshold;
  int32_t max_keypoints;
  int32_t max_width, max_height;
  double harris_k;
  int32_t n_levels;              /* 8 (ORB's nlevels); 1 .. GCS_KEYPOINT_MAX_LEVELS */
  int32_t scale_num, scale_den;  /* 6 / 5 (ORB's scaleFactor 1.2); scale_den >= 1,
                                    scale_den < scale_num <= 2 scale_den, scale_num <= 64 */
  int32_t device;
} gcs_keypoint_pyramid_config;

typedef struct {
  float *kp_u, *kp_v, *kp_response;   /* max_keypoints each */
  int32_t* kp_level;             /* max_keypoints */
  int32_t* counts;               /* 4: n_keypoints, n_survivors, n_corners (each summed over the levels), n_levels */
  int32_t* level_counts;         /* GCS_KEYPOINT_MAX_LEVELS x 4: per level n_keypoints, n_survivors, n_corners,
                                    quota; rows of levels >= n_levels are zero */
} gcs_keypoint_pyramid_outputs;

int gcs_keypoint_pyramid_config_defaults(gcs_keypoint_pyramid_config* cfg);
/* GCS_ERR_ARG, before any device call, for a config outside the ranges above. */
int gcs_keypoint_pyramid_ctx_create(const gcs_keypoint_pyramid_config* cfg, gcs_keypoint_pyramid_ctx** out);
int gcs_keypoint_pyramid_ctx_destroy(gcs_keypoint_pyramid_ctx* ctx);
const char* gcs_keypoint_pyramid_last_error(const gcs_keypoint_pyramid_ctx* ctx);
int gcs_keypoint_pyramid_ctx_set_stream(gcs_keypoint_pyramid_ctx* ctx, void* stream);
/* Queues its kernels on the context's stream and returns; every output is a device array.  Refusals as
 * gcs_detect_keypoints'. */
int gcs_detect_keypoints_pyramid(gcs_keypoint_pyramid_ctx* ctx, const gcs_keypoint_inputs* in,
                                 gcs_keypoint_pyramid_outputs* out);
/* The same steps on the host (no device, no context): every pointer is a host array. */
int gcs_detect_keypoints_pyramid_host(const gcs_keypoint_pyramid_config* cfg, const gcs_keypoint_inputs* in,
                                      gcs_keypoint_pyramid_outputs* out);
/* W_l, H_l, quota_l of every level for a width x height image, on the host; rows of levels >= n_levels are
 * zero.  max_width and max_height do not bound width and height here. */
int gcs_keypoint_pyramid_layout(const gcs_keypoint_pyramid_config* cfg, int32_t width, int32_t height,
                                int32_t out[GCS_KEYPOINT_MAX_LEVELS][3]);

/* Keypoints spread over a grid of cells: the pyramid detector above with its per-level selection (the second
 * half of P4) replaced by a fair share among the cells of each level, and, on request, a level's unused quota
 * handed on (what cv::ORB's spreading of its keypoints over the image does for the map; the definition is
 * the project's own, integer-exact wherever the two above are, and claims no parity with cv::ORB).  Steps P1-P3
 * and the quotas of P4 are as above.  With e = edge_threshold, s_l the survivors of level l after step 4:
 *  G1. cells: level l's kept area e <= x < W_l - e, e <= y < H_l - e is cut into cells of cell_size x cell_size
 *      level pixels anchored at (e, e): cx = (x - e) / cell_size, cy likewise, n_cx = ceil((W_l - 2 e) /
 *      cell_size), n_cy likewise, cell id cy n_cx + cx.  The last column and row may be partial.  A level with
 *      W_l <= 2 e or H_l <= 2 e has no cells and no keypoints.  Step 3 leaves at most ceil(cell_size / 2)^2
 *      <= 1024 survivors in a cell.
 *  G2. budgets: b_l = min(quota_l, s_l).  With redistribute: spare = sum_l (quota_l - b_l); then for l = 0, 1,
 *      ... in this order give = min(spare, s_l - b_l), b_l += give, spare -= give.  So sum_l b_l =
 *      min(K, sum_l s_l), the finest levels filled first.
 *  G3. fair share: within a cell the survivors are ordered by (response descending, raster index y W_l + x
 *      ascending); survivor i has rank r_i = 1, 2, ... in its cell.  With n_c the survivors of cell c, the cap
 *      t_l is the largest t >= 0 with sum_c min(n_c, t) <= b_l, taken no larger than max_c n_c.  Every survivor
 *      with r_i <= t_l is kept; rem_l = b_l - sum_c min(n_c, t_l); of the survivors with r_i = t_l + 1 the rem_l
 *      best by (response descending, raster index ascending) over the whole level -- step 6's order and tie
 *      rule -- are kept as well.  Exactly b_l keypoints are kept, and with b_l at least the number of non-empty
 *      cells every non-empty cell keeps one.
 *  G4. output: as P5, rows in (level, raster index) order, rows [n_keypoints, max_keypoints) NaN and -1.
 * With redistribute = 0 and every level's kept area inside one cell, and whenever s_l <= quota_l on every
 * level, the rows, counts and the first four columns of level_counts equal gcs_detect_keypoints_pyramid's.
 * The number of kernel launches of a call depends neither on n_levels nor on the number of cells.  Calls on
 * one context must be serialised. */
typedef struct gcs_keypoint_grid_ctx gcs_keypoint_grid_ctx;

typedef struct {
  int32_t fast_threshold;        /* the ten fields of gcs_keypoint_pyramid_config, same defaults and ranges */
  int32_t edge_threshold;
  int32_t max_keypoints;
  int32_t max_width, max_height;
  double harris_k;
  int32_t n_levels;
  int32_t scale_num, scale_den;
  int32_t cell_size;             /* 32; 8 .. 64 level pixels */
  int32_t redistribute;          /* 1; 0: an unused share is not handed on, 1: G2's second half */
  int32_t device;
} gcs_keypoint_grid_config;

typedef struct {
  float *kp_u, *kp_v, *kp_response;   /* max_keypoints each */
  int32_t* kp_level;             /* max_keypoints */
  int32_t* counts;               /* 4: n_keypoints, n_survivors, n_corners (each summed over the levels), n_levels */
  int32_t* level_counts;         /* GCS_KEYPOINT_MAX_LEVELS x 6: per level n_keypoints, n_survivors, n_corners,
                                    quota_l, b_l, t_l; rows of levels >= n_levels are zero */
} gcs_keypoint_grid_outputs;

int gcs_keypoint_grid_config_defaults(gcs_keypoint_grid_config* cfg);
/* GCS_ERR_ARG, before any device call, for a config outside the ranges above. */
int gcs_keypoint_grid_ctx_create(const gcs_keypoint_grid_config* cfg, gcs_keypoint_grid_ctx** out);
int gcs_keypoint_grid_ctx_destroy(gcs_keypoint_grid_ctx* ctx);
const char* gcs_keypoint_grid_last_error(const gcs_keypoint_grid_ctx* ctx);
int gcs_keypoint_grid_ctx_set_stream(gcs_keypoint_grid_ctx* ctx, void* stream);
/* Queues its kernels on the context's stream and returns; every output is a device array.  Refusals as
 * gcs_detect_keypoints'. */
int gcs_detect_keypoints_grid(gcs_keypoint_grid_ctx* ctx, const gcs_keypoint_inputs* in,
                              gcs_keypoint_grid_outputs* out);
/* The same steps on the host (no device, no context): every pointer is a host array. */
int gcs_detect_keypoints_grid_host(const gcs_keypoint_grid_config* cfg, const gcs_keypoint_inputs* in,
                                   gcs_keypoint_grid_outputs* out);
/* W_l, H_l, quota_l, n_cx, n_cy of every level for a width x height image, on the host; rows of levels
 * >= n_levels are zero, and so are n_cx and n_cy of a level without cells. */
int gcs_keypoint_grid_layout(const gcs_keypoint_grid_config* cfg, int32_t width, int32_t height,
                             int32_t out[GCS_KEYPOINT_MAX_LEVELS][5]);

/* ---------------------------------------------------------------- primitive path: keypoint descriptors */
/* What ORB adds behind its detector -- an orientation per keypoint and a steered 256-bit BRIEF descriptor -- and
 * a brute-force Hamming matcher to read the descriptors with.  The operators are the project's own: the angle
 * bin, the 256 bits and every match output are defined in integer arithmetic, so device, host twin and a numpy
 * restatement agree as bytes.  The pattern is a fixed pseudo-random one, not ORB's learned rBRIEF pattern, and
 * no parity with cv::ORB is claimed.
 *  D1. level and level pixel: keypoint i is (kp_u[i], kp_v[i]) in level-0 pixels on level kp_level[i]; a null
 *      kp_level puts every keypoint on level 0 (gcs_detect_keypoints' rows).  With W_l x H_l = the level sizes
 *      of P1 (n_levels, scale_num, scale_den from the config) and the level's grey image that of P2 -- the same
 *      bytes the pyramid and grid detectors see -- the level pixel is x = floor((double(u) + 0.5) * W_l / W_0),
 *      y likewise, every operation rounded on its own; this inverts P5's coordinate map exactly for every
 *      keypoint a detector of this library emits.  A row is invalid when u or v is not finite, level is
 *      outside [0, n_levels), the level has no pixels, or x < 16, x >= W_l - 16, y < 16 or y >= H_l - 16.  An
 *      invalid row gets angle NaN, bin -1 and 32 zero bytes; the detectors' NaN / -1 padding rows are invalid,
 *      and a detector with edge_threshold >= 16 emits no invalid row.
 *  D2. moments: over the level pixels (dx, dy) with dx^2 + dy^2 <= 225 around (x, y), m10 = sum dx g,
 *      m01 = sum dy g, exact in int32.
 *  D3. angle bin: 32 bins of 11.25 degrees.  The direction table (C_k, S_k), k = 0..31, is scaled by 2^14:
 *      (C_k, S_k) for k = 0..7 = (16384, 0), (16069, 3196), (15137, 6270), (13623, 9102), (11585, 11585),
 *      (9102, 13623), (6270, 15137), (3196, 16069), i.e. round(2^14 cos) and round(2^14 sin) of 11.25 k degrees,
 *      and C_{k+8} = -S_k, S_{k+8} = C_k, so a quarter turn of the table is exact.  The bin is the k that
 *      maximises m10 C_k + m01 S_k in int64, ties to the lowest k; a flat patch has bin 0.
 *  D4. angle: kp_angle = (float)atan2((double)m01, (double)m10) in radians (0 for m10 = m01 = 0).  It is
 *      informative only: nothing is decided by it, and it may differ by one float32 ulp between builds.
 *  D5. pattern: 256 pairs of int8 points (ax, ay, bx, by), a != b, |a|^2 and |b|^2 <= 169, produced by
 *      tools/gen_brief_pattern.py (a stated 32-bit recurrence with a fixed seed, rejection-sampled on the disc)
 *      and reported by gcs_brief_pattern.  For bin k the steered point of p = (x, y) is p_k = (rnd((x C_k -
 *      y S_k) / 2^14), rnd((x S_k + y C_k) / 2^14)) with rnd rounding half away from zero, in integers; so
 *      p_{k+8} is exactly p_k turned by a quarter turn.  The steering is computed, not tabulated.
 *  D6. bits: B(p) is the 5 x 5 box sum of the level's grey image centred at (x, y) + p (at most 6375).  Bit i is
 *      1 when B(a_k,i) < B(b_k,i); it is stored in byte i / 8 at bit i % 8 of the keypoint's 32-byte row.  The
 *      reach is 14 + 2 = 16 level pixels, the margin of D1.
 *  D7. match: q is n_query x 32 bytes, t is n_train x 32 bytes, both 4-byte aligned; q_bin and t_bin are
 *      optional int32 arrays (kp_angle_bin of the describer): a row is valid when its value is >= 0, and a null
 *      array makes every row valid.  For every query row: idx = the valid train row of least Hamming distance,
 *      ties to the lowest index, -1 when there is none or the query is invalid; dist = that distance, 257 when
 *      idx is -1; dist2 = the least distance among the other valid train rows, 257 when there is none or the
 *      query is invalid.  All int32.  n_query = 0 and n_train = 0 are legal.  No floating point and no atomics
 *      are involved: the result is bitwise repeatable.
 *  D8. gate: optional per-row positions q_u, q_v, t_u, t_v (float32, level-0 pixels, as the detectors emit) and
 *      levels q_level, t_level (int32; a null level array puts every row on level 0).  The prediction q_pu, q_pv
 *      (float32) is where query row i is expected in the train image; a null prediction uses q_u, q_v.  With
 *      radius (float32, finite, >= 0) and max_level_diff (int32, >= 0), train row j is a candidate of query row
 *      i -- C(i, j) -- when both rows are valid in D7's sense, fabsf(t_u[j] - q_pu[i]) <= radius, the same for
 *      v, and |t_level[j] - q_level[i]| <= max_level_diff (in exact integers).  Each difference is one IEEE
 *      float32 subtraction, never contracted; a non-finite position or prediction makes every comparison false,
 *      so that row has no candidates.  Per query row idx, dist, dist2 are D7's taken over the candidates only --
 *      the minimum is over (distance, index), so ties go to the lowest index whatever order rows are visited in
 *      -- and -1 / 257 / 257 where there are none; n_cand is the number of candidates (int32).  C is defined
 *      once, from the query side: the backward search of train row j is over the query rows i with C(i, j), by
 *      (distance, lowest i), which makes the cross check symmetric even with a per-row prediction.
 *  D9. pairs: with max_distance (int32; 256 or more switches it off), ratio_num, ratio_den (int32 in [1, 2^20];
 *      ratio_den = 0 switches the test off) and cross_check (0 / 1), query row i is kept when idx[i] >= 0,
 *      dist <= max_distance, (int64)dist * ratio_den < (int64)ratio_num * dist2 and, with cross_check, the
 *      backward search of idx[i] returns i.  pair_a, pair_b, pair_dist (int32, n_query entries each) hold the
 *      kept rows' i, idx[i], dist[i] in ascending i; every entry past the count is -1 / -1 / 257; count is one
 *      int32 in device memory.  With a null gate C is "both rows valid".  No atomics order anything: the result
 *      is bitwise repeatable.
 * gcs_describe_keypoints queues two kernels whatever n_levels is (the packed resample of P2, then one wave per
 * keypoint) and makes no host synchronisation; the row count is the caller's n_keypoints, so it chains behind a
 * detector with n_keypoints = max_keypoints and the padding.  gcs_match_descriptors queues at most two kernels,
 * gcs_match_descriptors_gated two, gcs_match_pairs at most four and one memset (both directions' searches in one
 * launch, their merges in one, then the keep flags' counts per 256 rows and the stable compaction); neither makes
 * a host synchronisation.  Calls on one context must be serialised. */
typedef struct gcs_keypoint_desc_ctx gcs_keypoint_desc_ctx;
typedef struct gcs_match_ctx gcs_match_ctx;
#define GCS_DESC_BYTES 32
#define GCS_MATCH_NONE 257

typedef struct {
  int32_t n_levels;              /* 8, as gcs_keypoint_pyramid_config's, same ranges */
  int32_t scale_num, scale_den;  /* 6, 5 */
  int32_t max_width, max_height; /* 1920 x 1080: capacity of the packed workspace */
  int32_t max_keypoints;         /* 4096; 1 .. 65536: the largest n_keypoints of a call */
  int32_t device;
} gcs_keypoint_desc_config;

/* The keypoints of one call: device pointers for gcs_describe_keypoints, host pointers for the host twin. */
typedef struct {
  int32_t n_keypoints;           /* 0 .. max_keypoints */
  const float *kp_u, *kp_v;      /* n_keypoints each, level-0 pixels */
  const int32_t* kp_level;       /* n_keypoints, or null: every keypoint on level 0 */
} gcs_keypoint_desc_keypoints;

typedef struct {
  float* kp_angle;               /* n_keypoints, radians (D4); NaN on an invalid row */
  int32_t* kp_angle_bin;         /* n_keypoints, 0 .. 31 (D3); -1 on an invalid row */
  uint8_t* desc;                 /* n_keypoints x 32 (D6); zero on an invalid row */
} gcs_keypoint_desc_outputs;

int gcs_keypoint_desc_config_defaults(gcs_keypoint_desc_config* cfg);
/* GCS_ERR_ARG, before any device call, for a config outside the ranges above. */
int gcs_keypoint_desc_ctx_create(const gcs_keypoint_desc_config* cfg, gcs_keypoint_desc_ctx** out);
int gcs_keypoint_desc_ctx_destroy(gcs_keypoint_desc_ctx* ctx);
const char* gcs_keypoint_desc_last_error(const gcs_keypoint_desc_ctx* ctx);
int gcs_keypoint_desc_ctx_set_stream(gcs_keypoint_desc_ctx* ctx, void* stream);
/* Queues its kernels on the context's stream and returns.  GCS_ERR_ARG (last_error set) for an image as
 * gcs_detect_keypoints refuses it, n_keypoints outside [0, max_keypoints] or, with n_keypoints > 0, a null array
 * other than kp_level. */
int gcs_describe_keypoints(gcs_keypoint_desc_ctx* ctx, const gcs_keypoint_inputs* in,
                           const gcs_keypoint_desc_keypoints* kps, gcs_keypoint_desc_outputs* out);
/* The same steps on the host (no device, no context): every pointer is a host array. */
int gcs_describe_keypoints_host(const gcs_keypoint_desc_config* cfg, const gcs_keypoint_inputs* in,
                                const gcs_keypoint_desc_keypoints* kps, gcs_keypoint_desc_outputs* out);
/* The pattern of D5: 256 rows of ax, ay, bx, by. */
int gcs_brief_pattern(int8_t out[256][4]);

typedef struct {
  int32_t max_query, max_train;  /* 4096 each; 1 .. 1048576: the largest n_query and n_train of a call */
  int32_t device;
} gcs_match_config;

typedef struct {
  int32_t n_query, n_train;
  const uint8_t *q, *t;          /* n_query x 32 and n_train x 32 bytes, 4-byte aligned */
  const int32_t *q_bin, *t_bin;  /* n_query and n_train, or null (D7) */
} gcs_match_inputs;

typedef struct {
  int32_t *idx, *dist, *dist2;   /* n_query each (D7) */
} gcs_match_outputs;

int gcs_match_config_defaults(gcs_match_config* cfg);
int gcs_match_ctx_create(const gcs_match_config* cfg, gcs_match_ctx** out);
int gcs_match_ctx_destroy(gcs_match_ctx* ctx);
const char* gcs_match_last_error(const gcs_match_ctx* ctx);
int gcs_match_ctx_set_stream(gcs_match_ctx* ctx, void* stream);
/* Queues its kernels on the context's stream and returns.  GCS_ERR_ARG (last_error set) for a count below 0 or
 * above the context's capacity, a null or misaligned array that the counts make necessary. */
int gcs_match_descriptors(gcs_match_ctx* ctx, const gcs_match_inputs* in, gcs_match_outputs* out);
/* The same on the host; of the config only the capacities are looked at. */
int gcs_match_descriptors_host(const gcs_match_config* cfg, const gcs_match_inputs* in, gcs_match_outputs* out);

/* D8's gate: device pointers for the device entries, host pointers for the host twins. */
typedef struct {
  const float *q_u, *q_v;        /* n_query each; may be null when q_pu and q_pv are given */
  const int32_t* q_level;        /* n_query, or null: every query row on level 0 */
  const float *t_u, *t_v;        /* n_train each */
  const int32_t* t_level;        /* n_train, or null */
  const float *q_pu, *q_pv;      /* n_query each, or both null: the prediction is q_u, q_v */
  float radius;                  /* 16; finite, >= 0, level-0 pixels */
  int32_t max_level_diff;        /* 1; >= 0 */
} gcs_match_gate;

typedef struct {
  int32_t *idx, *dist, *dist2;   /* n_query each (D8) */
  int32_t* n_cand;               /* n_query, or null */
} gcs_match_gated_outputs;

/* D9's parameters. */
typedef struct {
  int32_t max_distance;          /* 64; 256 or more: off */
  int32_t ratio_num, ratio_den;  /* 4, 5; 1 .. 1048576 each; ratio_den = 0: off */
  int32_t cross_check;           /* 1 */
} gcs_match_filter;

typedef struct {
  int32_t *pair_a, *pair_b, *pair_dist;   /* n_query each (D9) */
  int32_t* count;                         /* one int32 */
} gcs_match_pair_outputs;

/* Null pointers, radius 16, max_level_diff 1. */
int gcs_match_gate_defaults(gcs_match_gate* gate);
/* 64, 4, 5, 1: the conveniences of gcslam.descriptors.match_descriptors. */
int gcs_match_filter_defaults(gcs_match_filter* filter);
/* D8 in one direction.  Queues its kernels on the context's stream and returns.  GCS_ERR_ARG (last_error set) for
 * what gcs_match_descriptors refuses, a null gate, a radius that is NaN, infinite or negative, a negative
 * max_level_diff, one of q_pu, q_pv without the other, or a null position array that the counts make necessary
 * (with n_query > 0 the prediction or q_u and q_v; with n_query > 0 and n_train > 0 also t_u and t_v).  The
 * context stays usable after a refusal. */
int gcs_match_descriptors_gated(gcs_match_ctx* ctx, const gcs_match_inputs* in, const gcs_match_gate* gate,
                                gcs_match_gated_outputs* out);
/* D8 + D9; a null gate is no gate.  Refuses in addition a null filter, ratio_num outside [1, 1048576], ratio_den
 * outside [0, 1048576] and a null output array (count is needed even with n_query = 0).  The workspace of
 * gcs_match_ctx_create covers the backward direction as well: a context serves gcs_match_pairs up to its full
 * max_query x max_train. */
int gcs_match_pairs(gcs_match_ctx* ctx, const gcs_match_inputs* in, const gcs_match_gate* gate,
                    const gcs_match_filter* filter, gcs_match_pair_outputs* out);
/* The same on the host; of the config only the capacities are looked at. */
int gcs_match_descriptors_gated_host(const gcs_match_config* cfg, const gcs_match_inputs* in, const gcs_match_gate* gate,
                                     gcs_match_gated_outputs* out);
int gcs_match_pairs_host(const gcs_match_config* cfg, const gcs_match_inputs* in, const gcs_match_gate* gate,
                         const gcs_match_filter* filter, gcs_match_pair_outputs* out);

/* ---------------------------------------------------------------- primitive path: map rendering */
/* The reference's output side (backend/rendering.py, common/bev_pushforward.py) on the GPU, reading
 * an AtlasMapView's rows: for every (view, row) -- one thread per row, looping over the views -- the BEV pushforward to pixels, the 2 x 2 adjugate inverse,
 * the binning radius 2 / sqrt(max(lambda_min(Sigma^-1), eps)), opacity from log det Sigma_3D,
 * one-lobe vMF shading and world-space fBm (gcs_render_prepare); per (view, tile) the overlapping
 * rows ordered by (distance^2 to the tile centre, row), the first max_splats_per_tile kept
 * (gcs_render_bin_tiles, splat_indices_for_tile :252-289); per (view, tile) the normalised EWA blend
 * of the listed rows in list order (gcs_render_tiles, render_tile_ewa :297-355).  gcs_render_view
 * queues all three and synchronises once.  Tiles cover the image from (0, 0) = top left; tile
 * (ty, tx) has origin (oy, ox) = (ty, tx) * tile_size and n_ty = ceil(height / tile_size),
 * n_tx = ceil(width / tile_size).  Calls on one context must be serialised. */
typedef struct gcs_render_ctx gcs_render_ctx;
#define GCS_RENDER_MAX_VIEWS 32
#define GCS_RENDER_MAX_CAP 1024

typedef struct {
  /* SplatRenderingConfig (rendering.py:28-44), same names and defaults */
  int32_t tile_size;             /* clamped to [1, 32] as the reference does */
  int32_t max_splats_per_tile;   /* 1 .. GCS_RENDER_MAX_CAP */
  int32_t fbm_octaves;           /* 0 .. 16 */
  double fbm_gain, opacity_gamma, logdet0, eps, ewa_log_clip, alpha_min;
  double vmf_intensity_scale, vmf_intensity_max, vmf_kappa_max;
  int32_t device;
} gcs_render_config;

/* gcs_render_prepare's inputs.  Row arrays: device for gcs_render_prepare / gcs_render_view, host for
 * gcs_render_prepare_host.  The per-view arrays are always host arrays. */
typedef struct {
  int32_t n_rows, n_views;       /* n_views <= GCS_RENDER_MAX_VIEWS */
  const double* positions;       /* n_rows x 3 */
  const double* covariances;     /* n_rows x 9 */
  const double* directions;      /* n_rows x 3 (normalised here) */
  const double* kappas;          /* n_rows */
  const double* colors;          /* n_rows x 3 */
  const uint8_t* valid_mask;     /* n_rows; NULL = every row valid */
  const double* intensity;       /* n_rows; NULL = no kappa modulation */
  const double* P_pix;           /* host, n_views x 6: the 2 x 3 map to pixels */
  const double* offsets;         /* host, n_views x 2: mu_px = P_pix p + offset */
  const double* view_dirs;       /* host, n_views x 3 (normalised here) */
  double fbm_modulate_scale;     /* > 0: colours carry (1 - s) + s fBm(world xy) */
  int64_t fbm_seed;
} gcs_render_prepare_inputs;

/* The 2-D record of every (view, row).  A row that is not valid, or whose record is not finite, has
 * radius -inf (no tile takes it) and zeros elsewhere; so has, with fbm_modulate_scale > 0, a row with
 * |x| or |y| >= 2^46 (the fBm lattice index has to fit an int64).  fbm may be NULL. */
typedef struct {
  double* means;                 /* n_views x n_rows x 2 pixels (x, y) */
  double* Sigmas_inv;            /* n_views x n_rows x 4 */
  double* radii;                 /* n_views x n_rows */
  double* alphas;                /* n_rows */
  double* colors;                /* n_views x n_rows x 3: clip(colour * shading, 0, 1), times the fBm factor */
  double* fbm;                   /* n_rows (written when fbm_modulate_scale > 0, else zeros) */
} gcs_render_splats;

int gcs_render_config_defaults(gcs_render_config* cfg);
int gcs_render_ctx_create(const gcs_render_config* cfg, gcs_render_ctx** out);
int gcs_render_ctx_destroy(gcs_render_ctx* ctx);
const char* gcs_render_last_error(const gcs_render_ctx* ctx);
/* stream: a hipStream_t (NULL = the context's own); work on it is ordered after the caller's */
int gcs_render_ctx_set_stream(gcs_render_ctx* ctx, void* stream);
/* Synchronises. */
int gcs_render_prepare(gcs_render_ctx* ctx, const gcs_render_prepare_inputs* in, gcs_render_splats* out);
/* The same rows on the host (no device, no context): every pointer is a host array. */
int gcs_render_prepare_host(const gcs_render_config* cfg, const gcs_render_prepare_inputs* in,
                            gcs_render_splats* out);
/* indices: n_views x n_ty x n_tx x max_splats_per_tile int32, padded with -1; counts: n_views x n_ty x
 * n_tx int32.  radii NULL: computed from Sigmas_inv (n_views x n_rows x 4).  Exact and bitwise
 * reproducible for any number of overlapping rows.  Synchronises. */
int gcs_render_bin_tiles(gcs_render_ctx* ctx, int32_t n_views, int32_t n_rows, int32_t width, int32_t height,
                         const double* means, const double* radii, const double* Sigmas_inv, int32_t* indices,
                         int32_t* counts);
/* alphas: n_rows, or n_views x n_rows with alphas_per_view != 0.  image_layout 0: out is n_views x n_ty x
 * n_tx x tile x tile x 3 (whole tiles); 1: out is n_views x height x width x 3 (the in-image part of the
 * edge tiles).  An index outside [0, n_rows) contributes nothing.  Synchronises. */
int gcs_render_tiles(gcs_render_ctx* ctx, int32_t n_views, int32_t n_rows, int32_t width, int32_t height,
                     const double* means, const double* Sigmas_inv, const double* alphas, int32_t alphas_per_view,
                     const double* colors, const int32_t* indices, const int32_t* counts, int32_t image_layout,
                     double* out);
/* prepare + bin + render in one call: images n_views x height x width x 3.  splats NULL (or any of its
 * pointers NULL): the record stays in the context's workspace.  Synchronises once. */
int gcs_render_view(gcs_render_ctx* ctx, const gcs_render_prepare_inputs* in, int32_t width, int32_t height,
                    gcs_render_splats* splats, int32_t* indices, int32_t* counts, double* images);

/* ---------------------------------------------------------------- primitive path: OT association */
/* associate_primitives_ot (primitive_association.py:239-553) on the GPU: per measurement the MA-hex
 * stencil pool (n_stencil x m_tile_view view entries) costed by ||x_i - x_j||^2 + beta H^2_vMF
 * (:152-197; 1e12 where the view entry is invalid or the stencil tile is not in the view), the
 * k_assoc cheapest by (cost, pool position) (lax.sort with num_keys=1 is stable on cost alone, :376),
 * the selected candidates' unmasked cost + recency (eps lambda dt) with the row minimum subtracted,
 * then k_sinkhorn fixed iterations of unbalanced Sinkhorn (:105-138) on one workgroup; the OTCert /
 * SupportCert / InfluenceCert scalars land in cert[] (GCS_ASSOC_CERT_* slots).  An association
 * context owns the workspace for up to max_meas rows, max_pool view entries and k_assoc <= max_k
 * (<= 32; max_meas <= 2048 / 1024 / 512 for max_k <= 8 / 16 / 32). */
/* slots CAND_*: the MapUpdateCert's candidate statistics (pipeline.py:879-905: distinct candidate tiles
 * and valid candidates per valid measurement, means over the valid rows and the counts' p95), computed
 * beside the Sinkhorn iterations */
#define GCS_ASSOC_CERT_LEN 21
enum {
  GCS_ASSOC_CERT_DEFECT_A = 0, GCS_ASSOC_CERT_DEFECT_B, GCS_ASSOC_CERT_MASS_TOTAL, GCS_ASSOC_CERT_SUM_A,
  GCS_ASSOC_CERT_SUM_B, GCS_ASSOC_CERT_SUM_M, GCS_ASSOC_CERT_SUM_NOVEL, GCS_ASSOC_CERT_P95_A, GCS_ASSOC_CERT_P95_B,
  GCS_ASSOC_CERT_NONZERO_A, GCS_ASSOC_CERT_NONZERO_B, GCS_ASSOC_CERT_B_RECENCY_P95, GCS_ASSOC_CERT_ESS,
  GCS_ASSOC_CERT_MASS_EPS_RATIO, GCS_ASSOC_CERT_TOTAL_COST, GCS_ASSOC_CERT_SUPPORT_FRAC, GCS_ASSOC_CERT_EXACT,
  GCS_ASSOC_CERT_MAP_VALID, GCS_ASSOC_CERT_CAND_TILES_MEAN, GCS_ASSOC_CERT_CAND_PRIMS_MEAN,
  GCS_ASSOC_CERT_CAND_PRIMS_P95
};
enum { GCS_ASSOC_A_UNIFORM = 0, GCS_ASSOC_A_WEIGHT = 1 };  /* MeasurementMassPolicy (:40-48) */
enum { GCS_ASSOC_B_UNIFORM = 0 };                          /* MapMassPolicy (:51-59): only UNIFORM runs */
typedef struct gcs_assoc_ctx gcs_assoc_ctx;

typedef struct {            /* AssociationConfig, primitive_association.py:206-236 */
  int32_t k_assoc, k_sinkhorn;                     /* GC_K_ASSOC = 8, GC_K_SINKHORN = 50 */
  double beta, epsilon, tau_a, tau_b;              /* 0.5, 0.1, 0.5, 0.5 */
  int32_t cost_subtract_row_min, cost_scale_by_median;  /* 1, 0 */
  int32_t a_policy, b_policy;                      /* GCS_ASSOC_A_*, GCS_ASSOC_B_* */
  double eps_mass;                                 /* AssociationConfig.eps_mass: marginals, b rows, ESS */
  double eps_lift, eps_mass_dir;                   /* operator arguments eps_lift / eps_mass: measurement
                                                      means and directions (:296-297) */
  double h_tile;                                   /* GC_H_TILE = 2.0 */
  int32_t r_stencil_tiles_xy, r_stencil_tiles_z;   /* 1, 0 */
  int64_t scan_seq;
  double recency_decay_lambda;                     /* 0.02 */
} gcs_assoc_config;

typedef struct {            /* MeasurementBatch (measurement_batch.py:68-135), device pointers */
  const double* Lambdas;    /* n_total x 9 */
  const double* thetas;     /* n_total x 3 */
  const double* etas;       /* n_total x n_lobes x 3 */
  const double* weights;    /* n_total */
  const uint8_t* valid_mask;/* n_total */
  int32_t n_total, n_lobes;
  int32_t n_valid;          /* n_camera_valid + n_lidar_valid (host count, :272) */
} gcs_assoc_meas;

typedef struct {            /* AtlasMapView (primitive_map.py:270-300), device pointers */
  const int64_t* tile_ids;  /* n_tiles, view order */
  int32_t n_tiles, m_tile_view;     /* view entries = n_tiles x m_tile_view */
  const double* positions;  /* entries x 3 */
  const double* directions; /* entries x 3 */
  const double* kappas;     /* entries */
  const uint8_t* valid_mask;/* entries */
  const int64_t* last_supported_scan_seq;  /* entries */
  const int64_t* candidate_tile_ids;       /* entries */
  const int32_t* candidate_slots;          /* entries */
} gcs_assoc_view;

typedef struct {            /* PrimitiveAssociationResult (:71-92): device pointers, n_total x k_assoc */
  double* responsibilities; /* required */
  int32_t* candidate_pool_indices;  /* may be NULL */
  int64_t* candidate_tile_ids;      /* may be NULL */
  int64_t* candidate_slots;         /* may be NULL */
  double* row_masses;       /* n_total, required */
  double* cost_matrix;      /* required */
  /* host results */
  double cert[GCS_ASSOC_CERT_LEN];
  int32_t exact;            /* 1: the empty case (no valid measurement or map entry, :272-287) */
  int32_t n_map_valid;
} gcs_assoc_outputs;

int gcs_assoc_config_defaults(gcs_assoc_config* cfg);
/* Host evaluation of the Sinkhorn's short log / exp / x^y (gcs_math.h log_short, exp_short,
 * pow_sinkhorn; the device runs the same code) for the accuracy test against numpy. */
int gcs_debug_short_log_exp(const double* x, int32_t n, double y, double* log_out, double* exp_out, double* pow_out);
/* Host evaluation of the table-driven log / exp of the Sinkhorn loop (gcs_math.h log_tab, exp_tab;
 * NaN outside their domains: positive normal x / |x| < 700), for the same accuracy test. */
int gcs_debug_tab_log_exp(const double* x, int32_t n, double* log_out, double* exp_out);
int gcs_assoc_ctx_create(int32_t max_meas, int32_t max_pool, int32_t max_k, int32_t device, gcs_assoc_ctx** out);
int gcs_assoc_ctx_destroy(gcs_assoc_ctx* ctx);
const char* gcs_assoc_last_error(const gcs_assoc_ctx* ctx);
/* stream: a hipStream_t (NULL = the context's own); work on it is ordered after the caller's */
int gcs_assoc_ctx_set_stream(gcs_assoc_ctx* ctx, void* stream);
/* Synchronises; unsupported policies return GCS_ERR_ARG with the reference's message. */
int gcs_associate_primitives_ot(gcs_assoc_ctx* ctx, const gcs_assoc_config* cfg, const gcs_assoc_meas* meas,
                                const gcs_assoc_view* view, gcs_assoc_outputs* out);

/* visual_pose_evidence (visual_pose_evidence.py:260-412): 22-D pose evidence from the association's
 * soft correspondences at z_lin_pose = [t, rotvec] -- WLS translation (L_t = sum_i (sum_k pi) Lambda_i,
 * h_t, cost; :104-148) and the vMF scatter rotation (S = sum pi sqrt(k_i k_m) mu_m mu_i^T, SVD,
 * det-fixed U V^T, so3_log of R_scatter R_pred^T, L_rot = diag(s + eps); :150-240) -- summed in a
 * fixed order over the first n_valid valid rows on the association context's stream; the 3x3 SVD
 * and so3_log on the host.  exact = 1: the empty case (L = eps I, h = 0; :293-318). */
typedef struct {
  double L_pose[GCS_D_Z * GCS_D_Z], h_pose[GCS_D_Z];
  double L_trans[9], h_trans[3], L_rot[9], h_rot[3];
  double total_weighted_cost, mean_transported_mass;
  double ess_total, support_frac;   /* SupportCert */
  int32_t n_associations, exact;
} gcs_vpe_outputs;
int gcs_visual_pose_evidence(gcs_assoc_ctx* ctx, const gcs_assoc_meas* meas, const gcs_assoc_view* view,
                             const double* responsibilities, const int32_t* candidate_pool_indices,
                             const double* row_masses, int32_t k_assoc, const double* z_lin_pose, double eps_lift,
                             double eps_mass, gcs_vpe_outputs* out);

/* ---------------------------------------------------------------- primitive path: the primitive map */
/* The AtlasMap's tile storage (FS/backend/structures/primitive_map.py:98-227) resident in HBM, and
 * its maintenance operators on the GPU:
 *   gcs_pmap_extract_view      extract_atlas_map_view (:356-450, top m_view slots by weight per tile,
 *                              _select_topk_slots_fixed :303-322; view core :474-498)
 *   gcs_pmap_insert_masked     primitive_map_insert_masked (:807-981; eviction targets by
 *                              _select_lowest_mass_slots_fixed :325-353), several tiles per call
 *   gcs_pmap_fuse              primitive_map_fuse (:992-1163), the pipeline's per-active-tile loop
 *                              (pipeline.py:1301-1327) in one call
 *   gcs_pmap_cull              primitive_map_cull (:1175-1304, weight threshold)
 *   gcs_pmap_forget            primitive_map_forget (:1314-1384)
 *   gcs_pmap_recency_inflate   primitive_map_recency_inflate (:1400-1484)
 *   gcs_pmap_merge_reduce      primitive_map_merge_reduce (:1501-2031) for tiles of <= max_merge slots
 * A map context holds max_tiles tiles of m_tile slots (tile storage index 0..max_tiles-1; the caller
 * maps MA-hex tile ids to storage indices, as the AtlasMap dict does).  Per field the storage is
 * [tile][slot][width] (the reference's array shapes).  Sorts are stable radix sorts on the
 * reference's single key (lax.sort with num_keys = 1; -0.0 == 0.0); scatter-adds accumulate in
 * input order; no floating-point atomics: bitwise reproducible.  Every call synchronises. */
typedef struct gcs_pmap gcs_pmap;
enum {  /* field codes for gcs_pmap_read / gcs_pmap_write: element type and width per slot */
  GCS_PM_LAMBDAS = 0,  /* f64 x 9 */
  GCS_PM_THETAS,       /* f64 x 3 */
  GCS_PM_ETAS,         /* f64 x n_lobes*3 */
  GCS_PM_WEIGHTS,      /* f64 */
  GCS_PM_TIMESTAMPS,   /* f64 */
  GCS_PM_CREATED,      /* f64 */
  GCS_PM_COLORS,       /* f64 x 3 */
  GCS_PM_CAM_MASS,     /* f64 */
  GCS_PM_LIDAR_MASS,   /* f64 */
  GCS_PM_RGB_ACCUM,    /* f64 x 3 */
  GCS_PM_RGB_DENOM,    /* f64 */
  GCS_PM_RGB,          /* f64 x 3 */
  GCS_PM_LAST_SUPPORTED, /* i64 */
  GCS_PM_LAST_UPDATE,  /* i64 */
  GCS_PM_IDS,          /* i64 */
  GCS_PM_VALID,        /* u8 */
  GCS_PM_NFIELDS
};

typedef struct {            /* AtlasMapView outputs (device pointers, n_tiles x m_view rows; any may be NULL) */
  double* positions;        /* x 3 */
  double* covariances;      /* x 9 */
  double* directions;       /* x 3 */
  double* kappas;
  double* weights;
  int64_t* primitive_ids;
  uint8_t* valid_mask;
  int64_t* last_supported_scan_seq;
  double* etas;             /* x n_lobes*3 */
  double* colors;           /* x 3 (the tile's rgb) */
  int32_t* candidate_slots;
  int64_t* candidate_tile_ids;
} gcs_pmap_view;

typedef struct {            /* one row per proposal / contribution (device pointers; optional ones may be NULL) */
  const double* Lambdas;    /* n x 9 (world frame) */
  const double* thetas;     /* n x 3 */
  const double* etas;       /* n x n_lobes*3 */
  const double* weights;    /* n */
  const double* responsibilities; /* n (fuse) */
  const uint8_t* valid;     /* n: fuse valid_mask / insert valid_new_mask */
  const double* colors;     /* n x 3, optional */
  const int32_t* sources;   /* n (0 camera, 1 LiDAR), optional */
  const int32_t* tile_pos;  /* fuse: n, index into the call's tile list (-1: no tile) */
  const int32_t* slots;     /* fuse: n, target slot */
  int32_t n;
} gcs_pmap_rows;

int gcs_pmap_create(int32_t m_tile, int32_t max_tiles, int32_t n_lobes, int32_t max_merge, int32_t device,
                    gcs_pmap** out);
int gcs_pmap_destroy(gcs_pmap* pm);
const char* gcs_pmap_last_error(const gcs_pmap* pm);
int gcs_pmap_set_stream(gcs_pmap* pm, void* stream);
/* create_empty_tile (:148-174) into storage index tile */
int gcs_pmap_clear_tile(gcs_pmap* pm, int32_t tile);
/* one field of one tile, host buffer of m_tile x width elements */
int gcs_pmap_read(gcs_pmap* pm, int32_t tile, int32_t field, void* host);
int gcs_pmap_write(gcs_pmap* pm, int32_t tile, int32_t field, const void* host);
/* Device-to-device copy of whole tiles (every field) from src storage slots to dst storage slots (maps of
 * the same m_tile, n_lobes and device; dst == src allowed): the working copy of a hypothesis that reads
 * the node's map but must not update it (backend_node.py:2062,2079-2083). */
int gcs_pmap_copy_tiles(gcs_pmap* dst, const int32_t* dst_tiles, const gcs_pmap* src, const int32_t* src_tiles,
                        int32_t n);
/* tiles: n host storage indices in view order (-1: a tile missing from the map, viewed as empty);
 * tile_ids: the n MA-hex ids written to candidate_tile_ids */
int gcs_pmap_extract_view(gcs_pmap* pm, const int32_t* tiles, const int64_t* tile_ids, int32_t n, int32_t m_view,
                          double eps_lift, double eps_mass, gcs_pmap_view* out);
/* primitive_map_insert_masked for n tiles, K proposals each (rows tile-major, rows.n = n K); ids from
 * next_global_id in tile order.  new_ids (device, n K, -1 where masked) may be NULL; n_inserted and
 * count (host, n each): proposals inserted and the tile's valid count afterwards. */
int gcs_pmap_insert_masked(gcs_pmap* pm, const int32_t* tiles, int32_t n, int32_t K, const gcs_pmap_rows* rows,
                           double timestamp, int64_t scan_seq, double recency_decay_lambda, int64_t next_global_id,
                           int64_t* new_ids, int32_t* n_inserted, int32_t* count);
/* primitive_map_fuse on each of the n tiles with the rows whose tile_pos names it (valid & tile
 * match, pipeline.py:1304-1305); every listed tile gets the call's timestamp at every row's slot and
 * its rgb rebuilt, as the reference's per-tile call does.  n_fused (host): unique row slots. */
int gcs_pmap_fuse(gcs_pmap* pm, const int32_t* tiles, int32_t n, const gcs_pmap_rows* rows, double timestamp,
                  int64_t scan_seq, double eps_mass, int32_t* n_fused);
/* per tile (host, n each): culled count, mass dropped, sum of all weights, valid count afterwards */
int gcs_pmap_cull(gcs_pmap* pm, const int32_t* tiles, int32_t n, double weight_threshold, int32_t* n_culled,
                  double* mass_dropped, double* weight_sum, int32_t* count);
int gcs_pmap_forget(gcs_pmap* pm, const int32_t* tiles, int32_t n, double forgetting_factor);
/* stats (host): [downscale total, cov inflation trace, valid count] over the n tiles */
int gcs_pmap_recency_inflate(gcs_pmap* pm, const int32_t* tiles, int32_t n, int64_t scan_seq,
                             double recency_decay_lambda, double min_scale, double* stats);
/* the whole tile's Bhattacharyya pairs (m_tile <= max_merge); pairs (host, 2 x max_pairs): the merged
 * (kept, removed) slots in selection order */
int gcs_pmap_merge_reduce(gcs_pmap* pm, int32_t tile, double merge_threshold, int32_t max_pairs, double eps_psd,
                          double eps_lift, int32_t* n_merged, int32_t* pairs, int32_t* count);

/* Map publishing and the splat export (FS/backend/map_publisher.py:131-242, backend_node.py:2371-2459):
 * the variable-length extract_primitive_map_view (primitive_map.py:501-577) of each listed tile,
 * concatenated in list order, optionally ordered newest first, as renderable rows and packed
 * PointCloud2 records.  Device pointers to `capacity` rows each; any may be NULL. */
typedef struct {
  double* positions;        /* x 3 */
  double* covariances;      /* x 9 */
  double* directions;       /* x 3 */
  double* kappas;
  double* lambda_world;     /* x 9: inv(covariance + eps_lift I), renderable_batch_from_view (:600-607) */
  double* weights;
  double* etas;             /* x n_lobes*3 */
  double* colors;           /* x 3 (the tile's rgb) */
  int64_t* primitive_ids;
  int64_t* last_supported_scan_seq;
  int64_t* tile_ids;        /* the row's source tile id */
  int32_t* slots;           /* ... and slot */
  double* timestamps;       /* the slot-local fields of the splat export */
  double* created_timestamps;
  double* cam_mass;
  double* lidar_mass;
  double* rgb_cam_accum;    /* x 3 */
  double* rgb_cam_denom;
  void* points;             /* 16-byte records x, y, z, intensity (float32); 16-byte aligned */
} gcs_pmap_export_out;
enum { GCS_PM_ORDER_CONCAT = 0, GCS_PM_ORDER_RECENCY = 1 };
/* tiles / tile_ids: n host storage indices and ids in list order; a tile the map lacks (-1) is skipped
 * (map_publisher.py:149-151), an id listed twice contributes twice.  Per tile the valid slots in slot
 * order, or, where max_primitives > 0 and the tile's valid count exceeds it, the first max_primitives of
 * the stable order of -weight (:541-545).  order 0: concatenation order; order 1: stable by
 * (-last_supported_scan_seq, primitive_id) over all 64 bits, np.lexsort((ids, -recency)); a valid slot
 * of a listed tile with recency INT64_MIN is refused (GCS_ERR_ARG: its negation overflows).
 * n_rows (host): the total row count; tile_rows (host, n; may be NULL): rows per listed tile.  If
 * n_rows exceeds capacity the call returns GCS_ERR_ARG with n_rows and tile_rows set and writes no row. */
int gcs_pmap_export(gcs_pmap* pm, const int32_t* tiles, const int64_t* tile_ids, int32_t n, int32_t max_primitives,
                    int32_t order, double eps_lift, double eps_mass, int32_t capacity, const gcs_pmap_export_out* out,
                    int32_t* n_rows, int32_t* tile_rows);

/* Step 12b of process_scan_single_hypothesis (pipeline.py:1232-1492): the map update at z_t from the
 * scan's MeasurementBatch and PrimitiveAssociationResult over the n active tiles (storage indices +
 * MA-hex ids, the association stencil's tiles): per association block (block_associations_for_fuse,
 * primitive_association.py:561-588) the world-frame rows fused into every active tile; the novelty
 * proposals (a - row mass)+ w of the measurements whose world mean falls in the tile, k_insert_tile
 * per tile by a stable rank, inserted masked (ids from *next_global_id, advanced); then cull, forget
 * and merge-reduce per tile (the merge only when m_tile <= merge_max_tile_size, else the reference's
 * budget cap).  counts (host, n): the tiles' valid counts afterwards. */
typedef struct {            /* PipelineConfig fields (pipeline.py:187-206) and operator epsilons */
  int32_t k_insert_tile;    /* GC_K_INSERT_TILE = 64 */
  int32_t block_size;       /* GC_ASSOC_BLOCK_SIZE = 256 */
  int32_t k_merge_pairs;    /* GC_K_MERGE_PAIRS_PER_TILE = 4 */
  int32_t merge_max_tile_size;  /* GC_PRIMITIVE_MERGE_MAX_TILE_SIZE = 2048 */
  double h_tile;            /* GC_H_TILE = 2.0 */
  double recency_decay_lambda;  /* 0.02 */
  double cull_threshold;    /* 1e-4 */
  double forgetting_factor; /* 0.995 */
  double merge_threshold;   /* 0.1 */
  double eps_lift, eps_mass, eps_psd;  /* 1e-9, 1e-12, 1e-12 */
} gcs_pmap_update_config;

typedef struct {            /* device pointers */
  const double* Lambdas;    /* MeasurementBatch: n_total x 9 (body frame) */
  const double* thetas;     /* n_total x 3 */
  const double* etas;       /* n_total x n_lobes x 3 */
  const double* weights;    /* n_total */
  const uint8_t* valid;     /* n_total */
  const double* colors;     /* n_total x 3, may be NULL */
  const int32_t* sources;   /* n_total, may be NULL (LiDAR) */
  int32_t n_total, n_lobes;
  const double* responsibilities;    /* PrimitiveAssociationResult: n_total x k_assoc */
  const int64_t* candidate_tile_ids; /* n_total x k_assoc */
  const int64_t* candidate_slots;    /* n_total x k_assoc */
  const double* row_masses;          /* n_total */
  int32_t k_assoc;
} gcs_pmap_update_inputs;

typedef struct {            /* MapUpdateCert counters (pipeline.py:1454-1487) */
  int32_t fused_count, insert_count_total, evicted_count, merged_count;
  double fused_mass_total, insert_mass_total, insert_mass_p95, evicted_mass_total;
} gcs_pmap_update_stats;

int gcs_pmap_map_update(gcs_pmap* pm, const int32_t* tiles, const int64_t* tile_ids, int32_t n, const double* z_t6,
                        double timestamp, int64_t scan_seq, int64_t* next_global_id,
                        const gcs_pmap_update_config* cfg, const gcs_pmap_update_inputs* in,
                        gcs_pmap_update_stats* stats, int32_t* counts);

/* ---------------------------------------------------------------- the live primitive path in one call */
/* process_scan_single_hypothesis's live primitive path (pipeline.py:316-1591: the map branch :778-926,
 * visual pose evidence :980-1010, step 12b :1232-1492) as one stream-ordered chain on the context's
 * stream:
 *   gcs_scan_begin -> the active and stencil MA-hex tiles around the predicted position
 *   (tiling.py:167-209) -> surfels of the deskewed points -> recency inflation of the active tiles the
 *   map holds -> the atlas view over the stencil (a tile the map lacks is viewed as empty) -> OT
 *   association -> visual pose evidence at z_lin_pose -> gcs_scan_finish (trigger / ESS sums of the
 *   surfel, recency, association and visual certificates, pipeline.py:1049-1056,1211) -> step 12b at
 *   z_t over the active tiles (new tiles take free storage slots in order, AtlasMap.index).
 * The same kernels on the same arguments as the per-operator entry points, bit for bit, with host
 * waits only where a host value feeds the next launch (begin, the surfel count, the pose evidence).
 * Step 12b is left queued: gcs_live_collect waits for it and returns its statistics; no other call
 * on the context or the map may come between the two.  Contexts: the surfel / association / map
 * contexts are switched to the gcs_ctx's stream.  Stencils of at most 64 tiles. */
#define GCS_LIVE_MAX_TILES 64
typedef struct {
  gcs_surfel_ctx* surfels;
  gcs_assoc_ctx* assoc;
  gcs_pmap* map;
  /* the AtlasMap's tile directory (primitive_map.py:182-227; AtlasMap.tiles / _free / _written) */
  int32_t n_tiles;
  const int64_t* tile_ids;       /* [n_tiles] MA-hex ids held */
  const int32_t* tile_slots;     /* [n_tiles] their storage indices */
  int32_t n_free;
  const int32_t* free_slots;     /* [n_free] free storage indices, in the order new tiles take them */
  const uint8_t* slot_written;   /* [max_tiles] 1: the slot may hold data (a new tile there is cleared) */
  int64_t next_global_id;
  /* tiling and operator parameters (PipelineConfig) */
  double h_tile;
  int32_t r_active_xy, r_active_z, r_stencil_xy, r_stencil_z;
  int32_t n_active_expected, n_stencil_expected;  /* N_ACTIVE_TILES / N_STENCIL_TILES (checked) */
  int64_t scan_seq;
  double recency_lambda, recency_min_scale;
  int32_t m_tile_view;
  double eps_lift, eps_mass;
  const gcs_assoc_config* assoc_cfg;          /* scan_seq / recency_decay_lambda as above */
  const gcs_pmap_update_config* update_cfg;
  double timestamp;                            /* scan_end_time: step 12b's timestamp */
  /* the scan's device buffers (caller-allocated; the surfels read points / timestamps / weights) */
  const double* points_dev;
  const double* timestamps_dev;
  const double* weights_dev;
  int32_t n_points;
  gcs_surfel_outputs* surfel_out;  /* device pointers: the batch's LiDAR slice + the extractor arrays */
  int32_t* lidar_sources_dev;      /* the batch's sources from the LiDAR slice start: 1 on valid rows */
  gcs_assoc_meas meas;             /* the whole MeasurementBatch; n_valid is set by the call (the camera count;
                                      the surfel count is added on the device) */
  const double* batch_colors;      /* n_total x 3 (step 12b) */
  const int32_t* batch_sources;    /* n_total (step 12b) */
  gcs_pmap_view* view;             /* n_stencil x m_tile_view rows */
  int64_t* view_tile_ids_dev;      /* n_stencil: AtlasMapView.tile_ids */
  gcs_assoc_outputs* assoc_out;
  gcs_vpe_outputs* vpe_out;
  void* zero_dev;                  /* zeroed on the stream before the surfels (the batch's arrays), may be NULL */
  int64_t zero_bytes;
} gcs_live_args;

typedef struct {
  int32_t n_active, n_stencil;
  int64_t active_ids[GCS_LIVE_MAX_TILES], stencil_ids[GCS_LIVE_MAX_TILES];
  int32_t active_slots[GCS_LIVE_MAX_TILES];        /* storage index of each active tile (step 12b) */
  int32_t n_present_active;                        /* active tiles the map held before the scan */
  int32_t n_created;                               /* new tiles, in creation order */
  int64_t created_ids[GCS_LIVE_MAX_TILES];
  int32_t created_slots[GCS_LIVE_MAX_TILES];
  double recency_stats[3];                         /* gcs_pmap_recency_inflate's stats */
  double trigger_sum, ess_sum;                     /* the gcs_lidar_evidence handed to the finish */
  double phase_us[12];  /* host clock since the call's entry: [0] begin returned, [1] surfels queued,
                           [3] recency / view / association / pose evidence queued, [4] the one wait for them
                           returned and their results collected, [5] finish returned, [6] step 12b queued;
                           [7] gcs_live_collect's wait (set by gcs_live_collect); [8] the camera slice queued
                           (gcs_live_scan_camera: form A ahead of the begin, form B ahead of the surfels);
                           [2], [9]-[11] unused (the surfel count is read on the device) */
  /* after gcs_live_collect */
  gcs_pmap_update_stats update;
  int32_t counts[GCS_LIVE_MAX_TILES];              /* valid counts of the active tiles */
  int64_t next_global_id;
} gcs_live_outputs;

/* in: the scan (NULL: gcs_scan_begin already ran on ctx and begin holds its outputs).  begin, out:
 * as gcs_scan_begin / gcs_scan_finish. */
int gcs_live_scan(gcs_ctx* ctx, const gcs_scan_inputs* in, gcs_scan_begin_outputs* begin, const gcs_live_args* a,
                  gcs_live_outputs* lo, gcs_scan_outputs* out);
int gcs_live_collect(gcs_ctx* ctx, gcs_live_outputs* lo);

/* The camera slice of the chain's batch (rows [0, n_feat) of a->meas's arrays), in one of two forms.
 * Form A (ctx != NULL): the slice is built in the chain, as the node builds it ahead of its hypothesis
 * loop (backend_node.py:1865-1925).  gcs_camera_splats_scan's kernels on the scan's records (xyz_dev /
 * point_step / xyz_format / n_points; in->points_base and in->n_points are ignored) are the first work
 * queued on the context's stream, ahead of gcs_scan_begin's host prologue -- they depend on nothing the
 * begin produces and run under its host work -- so a->zero_dev is zeroed ahead of them.  out's batch
 * pointers are row 0 of the batch's own arrays; its diagnostics may be NULL.
 * Form B (ctx == NULL): a slice built earlier by gcs_camera_splats.  The n_feat rows of src's nine batch
 * arrays are copied device to device into out's on the stream, after the zeroing; src->n_camera_valid is
 * the camera count.
 * Either way the association and the pose evidence see n_camera_valid + the surfel count rows; the
 * certificates' sums follow the per-operator path (the surfel certificate's ESS is the LiDAR count).
 * out->n_camera_valid is set when the call returns GCS_OK. */
typedef struct {
  gcs_camsplat_ctx* ctx;               /* form A; NULL: form B */
  const gcs_camsplat_inputs* in;       /* form A */
  const void* xyz_dev;                 /* form A: the scan's records (gcs_scan_inputs.xyz_dev) */
  int32_t point_step, xyz_format, n_points;
  const gcs_camsplat_outputs* src;     /* form B */
  int32_t n_feat;                      /* form B: rows of the camera slice */
  gcs_camsplat_outputs* out;           /* both: the batch's camera slice (and form A's diagnostics) */
} gcs_live_camera;

/* gcs_live_scan with a camera slice (cam == NULL: gcs_live_scan itself, bit for bit).  A feature over
 * max_candidates (form A) is found at the chain's one wait, before gcs_scan_finish: the call returns
 * GCS_ERR_STATE with gcs_camera_splats' message, the belief is not advanced and step 12b is not queued;
 * the map is as after the recency inflation and lo's created tiles are to be adopted -- what any failure
 * between the begin and the finish leaves (a failed launch or wait there returns at the same point). */
int gcs_live_scan_camera(gcs_ctx* ctx, const gcs_scan_inputs* in, gcs_scan_begin_outputs* begin,
                         const gcs_live_args* a, const gcs_live_camera* cam, gcs_live_outputs* lo,
                         gcs_scan_outputs* out);
/* the MA-hex tile ids of tiling.py:167-209 (ma_hex_stencil_tile_ids) around center; returns the count
 * (or GCS_ERR_ARG when it exceeds cap) */
int gcs_ma_hex_stencil(const double* center3, double h_tile, int32_t radius_xy, int32_t radius_z, int64_t* out,
                       int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GCSLAM_HIP_H */
