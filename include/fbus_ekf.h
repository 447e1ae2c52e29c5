/*
 * fbus_ekf.h -- C ABI of the MI355X-native batched error-state EKF.
 *
 * Drop-in boundary for ONE path of CASIA-RoboticFish/FBUS-EKF: the filter's
 * predict (ImuUpdate) and correct (MeasureUpdate) steps, batched over B
 * independent filters that live in device memory.  The reference exposes no
 * FFI of its own (predict/correct are private members / Matlab functions), so
 * each entry point cites the reference call contract it replaces.  Paths are
 * relative to the upstream repository.
 *
 * Conventions
 *   - one handle = one device, B filters, one dtype (32|64) and one error-state
 *     size (18 = reference, 15 = gravity block removed);
 *   - calls are stream-ordered and asynchronous until fbus_ekf_sync();
 *     a handle is not thread-safe;
 *   - every function returns FBUS_OK (0) or a negative/positive fbus_status;
 *     fbus_ekf_last_error() gives the text of the last failure on a handle;
 *   - "host" entry points take host pointers in the handle's dtype (float for
 *     32, double for 64) and stage them through library-owned device buffers;
 *     "_dev" entry points take device pointers and add no copies -- these are
 *     the hot path;
 *   - arrays are dense row-major: nominal B x 19 (p3 v3 q4[wxyz] ba3 bg3 g3),
 *     rot B x 9 (carried rotation matrix, see below), P B x N x N,
 *     accel/gyro B x 3, marker ids B x M (int32, -1 = absent),
 *     marker pos B x M x 3, marker quat B x M x 4 (wxyz);
 *   - there is NO CPU fallback: without a HIP device create() fails with
 *     FBUS_ERR_NO_DEVICE.
 */
#ifndef FBUS_EKF_H
#define FBUS_EKF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FBUS_MAX_MARKERS 32     /* marker-map entries                     */
#define FBUS_MAX_VISIBLE 16     /* markers per frame and filter (M)       */
#define FBUS_MAX_MARKER_ID 1023 /* ArUco ids handled by the id->slot table */

typedef struct fbus_ekf* fbus_ekf_t;

typedef enum fbus_status {
    FBUS_OK = 0,
    FBUS_ERR_INVALID = 1,       /* bad argument                          */
    FBUS_ERR_NO_DEVICE = 2,     /* no usable HIP device                  */
    FBUS_ERR_HIP = 3,           /* a HIP runtime call failed             */
    FBUS_ERR_UNSUPPORTED = 4,   /* dtype / nstate / mode not built       */
    FBUS_ERR_NOMEM = 5,
    FBUS_ERR_ABI = 6            /* caller built against another header version (see FBUS_ABI_VERSION) */
} fbus_status;

/* Which of the reference's two implementations is reproduced. */
enum { FBUS_DIALECT_MATLAB = 0,   /* matlab/ImuUpdate.m, MeasureUpdate.m             */
       FBUS_DIALECT_CPP = 1 };    /* C++/src/filter.cpp                              */
/* Measurement handling in correct(). */
enum { FBUS_MODE_NEAREST = 0,     /* reference: nearest marker (C++: + hysteresis), 7 rows */
       FBUS_MODE_STACKED = 1 };   /* extension: all visible markers, 7M rows, one linearisation point */
/* Stereo geometry of corner inputs (marker_pose, correct_corners). */
enum { FBUS_VIS_REFRACTIVE = 0,   /* flat-port Snell ray trace (vision.cpp:472-618)      */
       FBUS_VIS_PINHOLE = 1,      /* 6x4 DLT (vision.cpp:395-466)                        */
       FBUS_VIS_CORNERS3D = 2 };  /* corner positions given, no triangulation            */
/* Covariance correction form. */
enum { FBUS_COV_SIMPLE = 0,       /* (I-KH)P then symmetrise (MeasureUpdate.m:101-102)  */
       FBUS_COV_JOSEPH = 1 };     /* (I-KH)P(I-KH)' + K R K'                            */

/* Replaces: EkfParam (C++/include/common.hpp:32-54), the constants built in the
 * FILTER ctor (C++/include/filter.hpp:63-125), matlab/FBUS_EKF.m:32-39,83-112,
 * MarkerPoseServer (common.hpp:19-29 / matlab/GetMarkerMap.m), CameraInfo::T_SC
 * and RefractInfo (common.hpp:58-103). */
typedef struct fbus_params {
    int32_t dialect;            /* FBUS_DIALECT_*                                       */
    int32_t cov_form;           /* FBUS_COV_*                                           */
    double  q_diag[4];          /* process noise added to the v, theta, ba, bg diagonals (not scaled by dt) */
    double  r_pos, r_quat;      /* measurement noise: position rows, quaternion rows    */
    double  p0_diag[6];         /* initial covariance per block p v theta ba bg g (used by fbus_ekf_reset_cov) */
    double  T_SC_left[16];      /* left camera T_SC, row-major 4x4, RAW (the diag(-1,-1,1,1) flip is applied inside) */
    double  T_SC_right[16];     /* right camera T_SC, RAW (triangulation only)          */
    int32_t n_markers;
    int32_t marker_id[FBUS_MAX_MARKERS];
    double  marker_pos[FBUS_MAX_MARKERS][3];
    double  marker_rot[FBUS_MAX_MARKERS][9];    /* row-major rotation marker->world     */
    double  switch_thres;       /* C++ dialect marker hysteresis (paramconfig.yml:57)   */
    double  max_dist;           /* marker_max_dist (paramconfig.yml:56), init/reset only */
    double  n_air, n_glass, n_water;            /* flat-port refraction (paramconfig.yml:31-42) */
    double  d_air, d_glass;
    double  port_normal[3];
    double  marker_size;        /* side of the square marker [m] (vision.hpp:114: 0.28); corner-row model only */
    double  r_pix;              /* noise of one normalised image coordinate (pixel-row model only); default 1e-6 */
} fbus_params;

/* Fills prm with the reference's constants for the given dialect
 * (FBUS_EKF.m / paramconfig.yml / camerainfo1.yml / GetMarkerMap.m). */
int fbus_params_default(fbus_params* prm, int dialect);
/* Host-side check of a parameter set (no device needed): dialect / cov_form values, positive noise, marker count and ids in
 * range.  FBUS_OK, or FBUS_ERR_INVALID with the reason in msg (may be NULL).  fbus_ekf_create applies the same checks. */
int fbus_params_validate(const fbus_params* prm, char* msg, size_t msg_len);

/* ---- ABI version ---------------------------------------------------------- */
/* fbus_params is passed by pointer and has grown (round 2 added r_pix); fbus_ekf_set_stream(h, NULL) changed
 * meaning in round 2 (NULL is HIP's legacy default stream now, FBUS_STREAM_OWN the handle's own stream).  A caller built
 * against an older header must not run silently against a newer library: fbus_ekf_create below is a macro that hands
 * the caller's compile-time sizeof(fbus_params) and FBUS_ABI_VERSION to fbus_ekf_create_checked, which refuses a
 * mismatch with FBUS_ERR_ABI.  (Bindings that cannot use the macro -- ctypes, loadlibrary -- call
 * fbus_ekf_abi_version() / fbus_params_size() once after loading and compare; the Python mirror does.)
 *   8  fbus_ekf_set_gate, fbus_ekf_correct_nis[_dev], fbus_ekf_correct_pixels_nis[_dev], fbus_ekf_correct_corners_nis[_dev]
 *      (struct unchanged); added under 8 without a bump: fbus_ekf_set_noise[_dev], fbus_ekf_get_noise (per-filter noise; no
 *      existing meaning changed -- callers detect the feature by the symbol); likewise fbus_ekf_loglik_enable / _reset / _get /
 *      _get_dev (per-filter innovation log-likelihood sums; off by default, nothing routed differently until switched on) and
 *      fbus_ekf_group_fuse[_dev], fbus_ekf_group_collapse[_dev], fbus_ekf_group_mix[_dev] (hypothesis groups; new kernels, nothing
 *      existing changed);
 *      fbus_ekf_set_velocity_sensor, fbus_ekf_correct_velocity[_dev|_async|_nis|_nis_dev] (body-velocity update): added under 8
 *      without a bump;
 *      fbus_ekf_correct_rows[_dev|_nis|_nis_dev] (the general linearised measurement update: residual and Jacobian rows from the
 *      caller): added under 8 without a bump;
 *      fbus_ekf_nees[_dev] (NEES, error and log-density against a truth state; a read-only kernel): added under 8 without a bump;
 *      fbus_ekf_sample[_dev] (draws from every filter's own Gaussian N(estimate, P); a read-only kernel): added under 8 without a bump;
 *      fbus_ekf_project_markers[_dev] (predicted corner pixels, their innovation covariance and visibility; a read-only kernel): added
 *      under 8 without a bump
 *   7  fbus_ekf_frames_fused_traj_dev, fbus_ekf_frames_meas_fused_traj_dev, fbus_ekf_snapshot_dev (struct unchanged)
 *   6  round 6: fbus_ekf_*_async, fbus_ekf_async_inputs_consumed / _stats, fbus_ekf_host_register / _unregister (struct unchanged)
 *   5  round 5: fbus_ekf_frame_meas_fused_dev, fbus_ekf_frames_meas_fused_dev (struct unchanged)
 *   4  round 4: fbus_ekf_set_policy_batch, fbus_ekf_launch_info (struct unchanged)
 *   3  round 3: FBUS_ERR_ABI, create_checked, team kernels (fbus_ekf_set_team), fbus_ekf_gather
 *   2  round 2: r_pix in fbus_params, set_stream(NULL) = legacy default stream
 *   1  round 1 */
#define FBUS_ABI_VERSION 8
int fbus_ekf_abi_version(void);
size_t fbus_params_size(void);

/* ---- lifetime ------------------------------------------------------------- */
/* Replaces: FILTER::FILTER (filter.hpp:63-137) for a batch of filters.
 * dtype 32|64, nstate 15|18.  device = HIP ordinal. */
int fbus_ekf_create_checked(fbus_ekf_t* out, const fbus_params* prm, size_t params_size, int abi_version,
                            int batch, int device, int dtype, int nstate);
int fbus_ekf_create(fbus_ekf_t* out, const fbus_params* prm, int batch, int device, int dtype, int nstate);
#ifndef FBUS_EKF_NO_ABI_CHECK
#define fbus_ekf_create(out, prm, batch, device, dtype, nstate) \
    fbus_ekf_create_checked((out), (prm), sizeof(fbus_params), FBUS_ABI_VERSION, (batch), (device), (dtype), (nstate))
#endif
int fbus_ekf_destroy(fbus_ekf_t h);
/* Run all work of this handle on an existing hipStream_t (e.g. the caller's
 * framework stream).  hip_stream is the hipStream_t itself: NULL (0) is HIP's
 * legacy default stream, as everywhere in HIP -- a caller whose framework is
 * on the default stream passes 0 and gets launches ordered with its own work.
 * FBUS_STREAM_OWN restores the handle's own stream, which is non-blocking:
 * it is ordered against NO other stream, so a caller that stays on it orders
 * its device buffers itself (fbus_ekf_sync / device sync, or the two calls
 * below). */
#define FBUS_STREAM_OWN ((void*)(intptr_t)-1)
int fbus_ekf_set_stream(fbus_ekf_t h, void* hip_stream);
/* Waves per 64-filter tile ("team" kernels; no reference counterpart -- the reference runs one filter on one thread,
 * filter.cpp:190-250).  predict_roles governs predict / predict_n and the fused frame / frame window entry points (fp32): 0 (default):
 * chosen per launch from how much of the chip a one-wave launch would leave idle -- predict: 3 waves per tile up to a quarter of the
 * chip's SIMDs in tiles (16 384 filters on MI355X), predict_n and the fused entry points: 4 up to half (32 768); 1: always one wave
 * per tile; 2..4: always that many.  correct_roles governs fbus_ekf_correct_corners (stacked mode) and fbus_ekf_correct_pixels, whose
 * markers are divided among the waves of a tile (both record types): 0 = four waves up to a quarter of the chip, two up to half;
 * 1 = never; 2 = two; 3..4 = four.  The pose-row fbus_ekf_correct always runs one wave per tile (its team form was measured slower at
 * every batch size and removed in round 4).  Results agree to fp32 rounding whatever the choice (predict: the same arithmetic, 1 ulp
 * on a few covariance elements where the compiler fuses a different product; the folds: double-precision sums in a different
 * order), so a caller that compares runs BIT FOR BIT across batch sizes pins the value -- or, for shards of one job, names the job's
 * size with fbus_ekf_set_policy_batch. */
int fbus_ekf_set_team(fbus_ekf_t h, int predict_roles, int correct_roles);
/* (round 4) The batch the automatic kernel-FAMILY choice above is keyed on.  0 (default): this handle's own batch.  A job that is
 * cut into shards over several handles / GPUs (fbus::ShardedFilter, bench.py --total-batch) names the WHOLE job here, so that every
 * shard layout runs the same kernels and produces the same bits as the single-handle run (the team and the one-wave kernels agree
 * to fp32 rounding only).  No reference counterpart (one filter, one thread: filter.cpp:190-250). */
int fbus_ekf_set_policy_batch(fbus_ekf_t h, int total_filters);
/* What the launch policy of this handle is (decided at create from the device: CU count, cache sizes; environment overrides are
 * read there once -- no entry point reads the environment afterwards).  `arg`: K for FBUS_INFO_ROLES_PREDICT, M for
 * FBUS_INFO_ROLES_MEAS, else ignored. */
enum { FBUS_INFO_SIMDS = 0,            /* SIMDs of the device = CUs x 4 (FBUS_FAKE_SIMDS overrides it: tests)              */
       FBUS_INFO_ONE_ROUND_FILTERS = 1,/* filters of one wave per SIMD = SIMDs x 64                                         */
       FBUS_INFO_TWO_WAVE_MIN_B = 2,   /* from this many filters on the <= 256-register kernel forms run                   */
       FBUS_INFO_BIG_RECORDS_MB = 3,   /* records above this take the default cache policy in predict                      */
       FBUS_INFO_MALL_MB = 4, FBUS_INFO_L2_KB = 5,
       FBUS_INFO_POLICY_BATCH = 6,     /* see fbus_ekf_set_policy_batch                                                    */
       FBUS_INFO_ROLES_PREDICT = 7,    /* waves per tile the next predict (arg = 1) / predict_n (arg = K) would use       */
       FBUS_INFO_ROLES_MEAS = 8,       /* ... correct_corners (stacked) / correct_pixels with arg = M marker slots          */
       FBUS_INFO_TEAM_FRAMES = 9,      /* 1: the fused frame / frame window entry points use the team kernel              */
       FBUS_INFO_MEAS_SPLIT = 10,      /* (round 5) correct_pixels with arg = M: 0 = one wave applies the update, 2 / 4 = the update divided
                                          between a solver and an updater wave, that many waves per tile (fp32, square port) */
       FBUS_INFO_NOISE_RESIDENT = 11 };/* 1: with the noise table and the likelihood sums as they are now, the fused frame / frame window
                                          entry points take the resident kernels that read the table (table set, sums off, fp32 records,
                                          policy batch above half a chip); 0 otherwise, no table included.  What a single call can still
                                          exclude ((Joseph, nearest) pose rows, M = 0, FBUS_NO_FRAME_MEAS) is not part of the answer */
int fbus_ekf_launch_info(fbus_ekf_t h, int what, int arg, int* value);
/* Cross-stream ordering without a host sync (hipEventRecord + hipStreamWaitEvent):
 * wait_stream   -- work submitted to the handle's stream after this call starts
 *                  only when everything already submitted to other_stream is done
 *                  (inputs produced on the caller's stream);
 * signal_stream -- the reverse (outputs consumed on the caller's stream). */
int fbus_ekf_wait_stream(fbus_ekf_t h, void* other_stream);
int fbus_ekf_signal_stream(fbus_ekf_t h, void* other_stream);
int fbus_ekf_sync(fbus_ekf_t h);
const char* fbus_ekf_last_error(fbus_ekf_t h);
const char* fbus_status_string(int status);

/* ---- state I/O (also serves as checkpoint / resume) ------------------------ */
/* Replaces: direct member access to NominalState/ErrorState (common.hpp:205-247)
 * and the Matlab State struct (FBUS_EKF.m:74-85).  Any pointer may be NULL to
 * skip that part.  prev_id is the C++ dialect's preUsedMarkerID_ (filter.hpp). */
int fbus_ekf_set_state(fbus_ekf_t h, const void* nominal, const void* rot, const void* P, const int32_t* prev_id);
int fbus_ekf_get_state(fbus_ekf_t h, void* nominal, void* rot, void* P, int32_t* prev_id);
int fbus_ekf_set_state_dev(fbus_ekf_t h, const void* nominal, const void* rot, const void* P, const int32_t* prev_id);
int fbus_ekf_get_state_dev(fbus_ekf_t h, void* nominal, void* rot, void* P, int32_t* prev_id);
/* P <- diag(p0_diag) for every filter. */
int fbus_ekf_reset_cov(fbus_ekf_t h);
/* The packed device-resident records (what a multi-GPU gather ships): base
 * pointer, bytes per filter and total bytes.  Layout: DESIGN.md section 3. */
int fbus_ekf_records(fbus_ekf_t h, void** dev_ptr, size_t* bytes_per_filter, size_t* total_bytes);
/* ---- multi-GPU: one process (rank) per GPU, one handle per rank, ONE collective -------------------------------
 * No reference counterpart: the reference runs one filter on one CPU thread (filter.cpp:190-250).  Filters are independent, so
 * the ranks step their shards with no communication; the single exchange of the path is the gather of the packed records at the
 * end, over RCCL (xGMI inside a node).  RCCL is bound at first use (dlopen of librccl.so.1); the single-GPU path never needs it.
 *   comm_unique_id  rank 0 creates the 128-byte ncclUniqueId and hands it to the other ranks (any out-of-band channel);
 *   comm_init       every rank: ncclCommInitRank on the handle's device;
 *   comm_attach     alternatively adopt an existing ncclComm_t of the caller's (not destroyed by the library);
 *   gather          every rank's records into out_dev on every rank, on the handle's stream (asynchronous until
 *                   fbus_ekf_sync).  bytes_of_rank = NULL: all ranks hold the same number of bytes (ncclAllGather, rank k at
 *                   offset k * bytes); otherwise world entries (entry [rank] = this handle's fbus_ekf_records total): ragged
 *                   shards, rank k at the running offset (grouped ncclBroadcast). */
int fbus_ekf_comm_unique_id(void* id128);
int fbus_ekf_comm_init(fbus_ekf_t h, const void* id128, int rank, int world);
int fbus_ekf_comm_attach(fbus_ekf_t h, void* nccl_comm, int rank, int world);
int fbus_ekf_comm_destroy(fbus_ekf_t h);
int fbus_ekf_gather(fbus_ekf_t h, void* out_dev, const size_t* bytes_of_rank);
/* (round 4) ONE process that owns several devices (fbus::NodeFilter -- the closest thing to the reference's one stateful object,
 * filter.cpp:190-250, owning a whole node).  comm_init_all: ncclCommInitAll over the handles' devices, rank k = handles[k] (one handle
 * per device).  gather_group: the fbus_ekf_gather of all n ranks inside one RCCL group (out_dev[k] on handles[k]'s device).
 * copy_records: this handle's packed records to a buffer on any device of the process, on the handle's stream (hipMemcpyPeerAsync) --
 * the gather when the consumer sits on one device, or when the shards share a device; no communicator needed. */
int fbus_ekf_comm_init_all(fbus_ekf_t* handles, int n);
int fbus_ekf_gather_group(fbus_ekf_t* handles, int n, void* const* out_dev, const size_t* bytes_of_rank);
int fbus_ekf_copy_records(fbus_ekf_t h, void* dst, int dst_device);
/* Point the handle at caller-owned device storage of total_bytes (as reported
 * by fbus_ekf_records) so that a framework tensor can alias the records. */
int fbus_ekf_attach_records(fbus_ekf_t h, void* dev_ptr, size_t total_bytes);

/* ---- predict == ImuUpdate -------------------------------------------------- */
/* Replaces: State = ImuUpdate(State, accel, gyro, dt) (matlab/ImuUpdate.m:36) and
 * FILTER::UpdateCovariance + UpdateNominalState (filter.cpp:588-616,533-582) as
 * called per IMU sample from BatchImuProcessing (filter.cpp:505-516).
 * dt_per_filter = 0: dt points to ONE value; 1: B values. */
int fbus_ekf_predict(fbus_ekf_t h, const void* accel, const void* gyro, const void* dt, int dt_per_filter);
int fbus_ekf_predict_dev(fbus_ekf_t h, const void* accel, const void* gyro, const void* dt, int dt_per_filter);
/* K consecutive IMU samples in one launch (state stays in registers between
 * samples).  accel/gyro are K x B x 3, dt is K (dt_per_filter=0) or K x B.
 * Same arithmetic, same results as K fbus_ekf_predict calls. */
int fbus_ekf_predict_n(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter);
int fbus_ekf_predict_n_dev(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter);

/* ---- (round 6) the same host-pointer signatures WITHOUT the wait -------------- */
/* Replaces the same calls as fbus_ekf_predict / _predict_n / _correct / _correct_pixels, as the reference's caller issues them: one
 * call per IMU sample / camera frame that returns at once (FILTER::SetImuData hands the sample to the filter thread under a mutex,
 * filter.cpp:24-55; BatchImuProcessing then runs one predict per sample, :505-516; SetDetectionResult copies the detections,
 * :61-65).  Arguments, checks, arithmetic and results are those of the synchronous entry points; what differs:
 *   - every HOST array is taken by value at the call.  Pageable memory is copied into a pinned ring slot of the handle's by the
 *     calling thread -- the caller's buffer is free again on return.  Memory that is already pinned (hipHostMalloc, hipHostRegister,
 *     fbus_ekf_host_register below; pieces of >= 4 KiB) is transferred IN PLACE and must stay unchanged until
 *     fbus_ekf_async_inputs_consumed() or fbus_ekf_sync() returns;
 *   - nothing waits for the device: the H2D copy runs on a copy stream, the kernel on the handle's stream behind it, so the copy of
 *     call i + 1 overlaps the kernel of call i.  The ring has 8 slots; the ninth call in flight waits for the first one's kernel
 *     (back-pressure; counted by fbus_ekf_async_stats);
 *   - completion and device-side errors surface at fbus_ekf_sync() or at any host-pointer result (fbus_ekf_get_state,
 *     fbus_ekf_get_applied), which are unchanged.  Not capturable into a HIP graph (FBUS_ERR_INVALID between graph_begin / _end).
 * Measured (tools/host_api_rate.py). */
int fbus_ekf_predict_async(fbus_ekf_t h, const void* accel, const void* gyro, const void* dt, int dt_per_filter);
int fbus_ekf_predict_n_async(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter);
int fbus_ekf_correct_async(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip);
int fbus_ekf_correct_pixels_async(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right /* may be NULL */,
                                  const uint8_t* skip);
/* every H2D copy issued so far has completed: pinned input arrays handed to the _async calls may be rewritten (cheaper than
 * fbus_ekf_sync: does not wait for the kernels) */
int fbus_ekf_async_inputs_consumed(fbus_ekf_t h);
/* counters since create: _async calls, calls that had to wait for a ring slot, input pieces transferred in place (any may be NULL) */
int fbus_ekf_async_stats(fbus_ekf_t h, int64_t* calls, int64_t* waits, int64_t* direct_pieces);
/* page-lock / release a host range for in-place transfers (hipHostRegister / hipHostUnregister for callers without HIP headers) */
int fbus_ekf_host_register(void* ptr, size_t bytes);
int fbus_ekf_host_unregister(void* ptr);

/* ---- correct == MeasureUpdate ---------------------------------------------- */
/* Replaces: State = MeasureUpdate(State, visionMeas[8xM], markerMap, cameraInfo)
 * (matlab/MeasureUpdate.m:37) and FILTER::ObservationUpdate (filter.cpp:622-754)
 * fed by SetDetectionResult (filter.cpp:61-65).  ids B x M (-1 = slot unused),
 * pos B x M x 3, quat B x M x 4.  skip (B bytes, may be NULL): non-zero = leave
 * that filter untouched.  Filters with no usable marker are left untouched
 * (the reference's silent early return, filter.cpp:671-673). */
int fbus_ekf_correct(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat,
                     int mode, const uint8_t* skip);
int fbus_ekf_correct_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat,
                         int mode, const uint8_t* skip);
/* 1 where the last correct() applied an update, 0 where it returned early. */
int fbus_ekf_get_applied(fbus_ekf_t h, uint8_t* applied_host);

/* ---- correct from stereo corners (north-star extension; NO reference counterpart) ------------ */
/* The per-corner measurement model BASELINE.json's north_star describes, in the form SURVEY.md section 0.1 (B2)
 * fixes: the marker's four corners are triangulated on the device (flat-port refractive or pin-hole, the
 * arithmetic of fbus_ekf_marker_pose: vision.cpp:472-618 / :395-466) and each corner position is a 3-row
 * measurement h_k = R_IL R'(P_m + R_m c_k - p - R P_IL), c_k = corner k in the marker frame of
 * VISION::ComputeMarkerPose (vision.cpp:736-759), noise r_pos per row: 12 rows per marker, Jacobians of the
 * reference's position rows (MeasureUpdate.m:72-73), same gain / injection / covariance algebra as correct().
 * left/right: B x M x 8 normalised corner coordinates (FBUS_VIS_REFRACTIVE / FBUS_VIS_PINHOLE), or
 * left = B x M x 12 corner positions (FBUS_VIS_CORNERS3D).  mode as in correct() (nearest = by corner 0).
 * The reference has nothing to compare this with: it is validated against the fp64 oracle only. */
int fbus_ekf_correct_corners(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right,
                             int geometry, int mode, const uint8_t* skip);
int fbus_ekf_correct_corners_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right,
                                 int geometry, int mode, const uint8_t* skip);

/* ---- one camera frame: K predicts then one correct -------------------------- */
/* Replaces one iteration of the frame loop (matlab/FBUS_EKF.m:175-196;
 * filter.cpp:232-235): enqueues K per-sample predict launches followed by one
 * correct launch without returning to the caller in between.  Device pointers. */
int fbus_ekf_frame_dev(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter,
                       int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip);

/* Same frame in ONE launch: the records stay in registers between the K predicts and the correct
 * (one HBM round trip per frame instead of one per EKF step).  Same arithmetic and results as
 * fbus_ekf_frame_dev.  M = 0: predicts only. */
int fbus_ekf_frame_fused_dev(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter,
                             int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip);

/* (round 5) The same frame with the NORTH STAR's MeasureUpdate -- correct() from corner pixels (FBUS_MEAS_PIXELS: the rows of
 * fbus_ekf_correct_pixels_dev; right may be NULL = left camera; geometry and mode are ignored) or from stereo corners
 * (FBUS_MEAS_CORNERS: fbus_ekf_correct_corners_dev with its geometry and mode) -- in place of the pose rows: K predicts
 * (matlab/ImuUpdate.m:36-82 ; filter.cpp:505-516) and the update (matlab/MeasureUpdate.m:84-102 with the reprojection rows of the
 * flat-port model, vision.cpp:496-599 run forward) in ONE launch, the record resident in registers / LDS in between.  Same
 * arithmetic as K fbus_ekf_predict_dev calls + one fbus_ekf_correct_pixels_dev / _corners_dev call, and equal results TO FP32
 * ROUNDING (the single-step gate of tests/util.py: which product of an a b + c d becomes an FMA differs between the specialised
 * kernels); bit-equal are the update alone (K = 0) to the per-call update and a window to its sequence of frames.  Where the one
 * launch is taken and where the frame runs as fbus_ekf_predict_n_dev + the per-call update: the route table, DESIGN.md 5.1 (rows
 * "pixels, corners").  M = 0: predicts only.  left / right: 16-byte aligned. */
enum { FBUS_MEAS_PIXELS = 0, FBUS_MEAS_CORNERS = 1 };
int fbus_ekf_frame_meas_fused_dev(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter,
                                  int kind, int M, const int32_t* ids, const void* left, const void* right, int geometry, int mode,
                                  const uint8_t* skip);

/* (round 5) A WINDOW of such frames in ONE launch (offline replay of a recorded stretch of corners.txt through the north star's model: the
 * frame loop of matlab/FBUS_EKF.m:151-210 with the reprojection / corner rows): nframes times { kcount[f] predicts, the update }, the
 * records resident from the first load to the last store.  Same arithmetic and results as nframes calls of
 * fbus_ekf_frame_meas_fused_dev (bit-equal where that takes its resident kernel; elsewhere this entry point runs frame by frame).
 *   kcount HOST array, nframes entries (<= FBUS_MAX_WINDOW_FRAMES), each 0..255;  accel, gyro [sum kcount][B][3], dt [sum kcount] or [..][B]
 *   ids [nframes][B][M], left / right [nframes][B][M][8] ([..][12] corner positions for FBUS_VIS_CORNERS3D), skip [nframes][B] or NULL
 * fbus_ekf_get_applied afterwards reports the LAST frame of the window. */
int fbus_ekf_frames_meas_fused_dev(fbus_ekf_t h, int nframes, const int32_t* kcount, const void* accel, const void* gyro, const void* dt,
                                   int dt_per_filter, int kind, int M, const int32_t* ids, const void* left, const void* right, int geometry,
                                   int mode, const uint8_t* skip);

/* A WINDOW of camera frames in ONE launch (offline replay of a recorded stretch: the frame loop of
 * matlab/FBUS_EKF.m:151-210 / FilterThreadFunction, filter.cpp:229-235): nframes times { kcount[f] predicts, one
 * correct } with the records resident in registers from the first load to the last store.  Same arithmetic and
 * results as nframes calls of fbus_ekf_frame_fused_dev.
 *   kcount  HOST array, nframes entries (<= FBUS_MAX_WINDOW_FRAMES), each 0..255: IMU samples in front of frame f
 *   accel, gyro  [sum kcount][B][3], dt [sum kcount] or [sum kcount][B] (dt_per_filter)       device
 *   ids [nframes][B][M], pos [nframes][B][M][3], quat [nframes][B][M][4], skip [nframes][B] or NULL   device
 * fbus_ekf_get_applied afterwards reports the LAST frame of the window. */
#define FBUS_MAX_WINDOW_FRAMES 64
int fbus_ekf_frames_fused_dev(fbus_ekf_t h, int nframes, const int32_t* kcount, const void* accel, const void* gyro,
                              const void* dt, int dt_per_filter, int M, const int32_t* ids, const void* pos,
                              const void* quat, int mode, const uint8_t* skip);

/* The two windows above WITH THEIR TRAJECTORY: one state per camera frame, the reference's product -- matlab/FBUS_EKF.m:201-204 appends
 * ekfState (p, v, q, ba, bg, g) to EKFResults after every frame, C++/src/filter.cpp:238-248 one fusion.txt row.  Arguments before the
 * three outputs: those of the twin, with the same checks (all made before the first launch).  Outputs, device memory, each may be NULL
 * (not written):
 *   out_nominal  [nframes][B][19] in the handle's dtype, the get_state order p3 v3 q4(wxyz) ba3 bg3 g3
 *   out_pdiag    [nframes][B][N]  the diagonal of P
 *   out_applied  [nframes][B]     1 where frame f's update ran: what fbus_ekf_get_applied would report after frame f alone
 * Row f is the state after frame f's update (after its predicts where the update did not run: skip, no usable marker, M = 0).  The
 * records, fbus_ekf_get_applied and every other effect are bit-identical to the twin's on the same inputs; with all three outputs NULL
 * the call IS the twin.  Row f equals what fbus_ekf_get_state (nominal, diag P) / fbus_ekf_get_applied report after the same frame run
 * alone, bit for bit wherever the twin's window equals its frames bit for bit.  The one-wave resident window kernels write the rows
 * from their registers; every other route (fp64 records, Joseph + nearest, team / small launches, nframes == 1 for the pixel / corner
 * rows) already runs frame by frame and adds fbus_ekf_snapshot_dev's kernel behind each frame.
 * The outputs must not overlap the records (FBUS_ERR_INVALID) nor any input array (not checked). */
int fbus_ekf_frames_fused_traj_dev(fbus_ekf_t h, int nframes, const int32_t* kcount, const void* accel, const void* gyro,
                                   const void* dt, int dt_per_filter, int M, const int32_t* ids, const void* pos,
                                   const void* quat, int mode, const uint8_t* skip,
                                   void* out_nominal, void* out_pdiag, uint8_t* out_applied);
int fbus_ekf_frames_meas_fused_traj_dev(fbus_ekf_t h, int nframes, const int32_t* kcount, const void* accel, const void* gyro,
                                        const void* dt, int dt_per_filter, int kind, int M, const int32_t* ids, const void* left,
                                        const void* right, int geometry, int mode, const uint8_t* skip,
                                        void* out_nominal, void* out_pdiag, uint8_t* out_applied);
/* The pose and its sigma of every filter from the current records, without the full covariance of fbus_ekf_get_state_dev: nominal
 * B x 19 (get_state order), pdiag B x N = diag(P), applied B (= fbus_ekf_get_applied).  Device pointers, each may be NULL;
 * stream-ordered.  Equal to get_state's nominal and diag(P) bit for bit (the same index map).  Outputs must not overlap the records. */
int fbus_ekf_snapshot_dev(fbus_ekf_t h, void* nominal, void* pdiag, uint8_t* applied);

/* ---- initialisation / reset (the callers' side of the path) ------------------- */
/* Replaces: InitGravityAndGyrobias (matlab/InitGravityAndGyrobias.m:36-40) /
 * FILTER::InitializeGravityAndBias (filter.cpp:256-285).  accel, gyro: T x B x 3.
 * Writes g = (0, 0, -|mean accel|) and bg = mean gyro of every filter. */
int fbus_ekf_init_gravity_bias(fbus_ekf_t h, int T, const void* accel, const void* gyro);
int fbus_ekf_init_gravity_bias_dev(fbus_ekf_t h, int T, const void* accel, const void* gyro);
/* Replaces: InitPositionAndQuaternion (matlab/InitPositionAndQuaternion.m:38-80) /
 * FILTER::InitializePose (filter.cpp:291-399) [FBUS_POSE_INIT: p, q, R from the nearest
 * marker, g = (9.8, 0, 0)] and ResetState (matlab/ResetState.m:37-80) /
 * FILTER::ResetSystemState (filter.cpp:405-477) [FBUS_POSE_RESET: p, q, v = 0, ba = 0;
 * Matlab dialect also refreshes R, C++ dialect also zeroes bg and leaves R stale].
 * mask (B bytes, may be NULL = all): non-zero selects the filters to (re)initialise.
 * C++ dialect: markers farther than params.max_dist are refused (filter.cpp:343-347).
 * fbus_ekf_get_applied() tells which filters were changed. */
enum { FBUS_POSE_INIT = 0, FBUS_POSE_RESET = 1 };
int fbus_ekf_pose_init(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int what,
                       const uint8_t* mask);
int fbus_ekf_pose_init_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int what,
                           const uint8_t* mask);
/* Replaces: ComputeVisionOnlyResults (matlab/ComputeVisionOnlyResults.m:39-79) /
 * positionOnlyVisual, quaternionOnlyVisual (filter.cpp:449-456).  out_pose: B x 7 (p3, q4 wxyz);
 * the state is not touched. */
int fbus_ekf_vision_only_pose(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat,
                              void* out_pose);
int fbus_ekf_vision_only_pose_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat,
                                  void* out_pose);
/* Replaces: the IMU pre-filter of FILTER::SetImuData (filter.cpp:36-47):
 * y[t] = 0.9 y[t-1] + 0.1 x[t] per filter, in place on T x B x 3 accel / gyro arrays; the last
 * filtered sample is carried in the handle to the next call (restart != 0 forgets it: the next
 * sample passes through, as the first buffered sample does in the reference). */
int fbus_ekf_imu_ema(fbus_ekf_t h, int T, void* accel, void* gyro, int restart);
int fbus_ekf_imu_ema_dev(fbus_ekf_t h, int T, void* accel, void* gyro, int restart);

/* ---- marker pose from stereo corners (the step in front of correct) --------- */
/* Replaces: VISION::RefractionTriangulation (C++/src/vision.cpp:472-618) or
 * VISION::NormalTriangulation (:395-466) followed by VISION::ComputeMarkerPose
 * (:624-759), for n markers at once (n = B x M when the output feeds correct()).
 * geometry FBUS_VIS_REFRACTIVE / FBUS_VIS_PINHOLE: left/right are n x 8 undistorted
 * normalised image coordinates of the four corners (x0 y0 .. x3 y3, the corners.txt
 * layout written at vision.cpp:111-119).  FBUS_VIS_CORNERS3D: `left` is n x 12 corner
 * positions in the left camera frame (the alternative log at vision.cpp:120-124) and
 * `right` is ignored.  Outputs: pos n x 3, quat n x 4 (wxyz) -- exactly the arrays
 * correct() takes -- and, if not NULL, corners3d n x 12.  Uses the handle's
 * T_SC_left/right and refraction constants, dtype and stream. */
int fbus_ekf_marker_pose(fbus_ekf_t h, int n, int geometry, const void* left, const void* right,
                         void* pos, void* quat, void* corners3d);
int fbus_ekf_marker_pose_dev(fbus_ekf_t h, int n, int geometry, const void* left, const void* right,
                             void* pos, void* quat, void* corners3d);

/* ---- HIP graphs -------------------------------------------------------------- */
/* Capture any sequence of *_dev calls on this handle once (between graph_begin and graph_end: the calls are
 * recorded, not executed; no host-pointer entry points, no sync, no timing inside) and replay it with ONE
 * launch.  The captured launches keep the device pointers they were given: replay reads the same input
 * buffers (refill them in place between replays).  For launch-bound inner loops: small batches, long runs of
 * per-step launches.  New: the reference runs one filter on one CPU thread and has nothing comparable. */
int fbus_ekf_graph_begin(fbus_ekf_t h);
int fbus_ekf_graph_end(fbus_ekf_t h, int* graph_id);
int fbus_ekf_graph_launch(fbus_ekf_t h, int graph_id);
int fbus_ekf_graph_destroy(fbus_ekf_t h, int graph_id);

/* ---- measurement support (bench / profiling) -------------------------------- */
enum { FBUS_KERNEL_PREDICT = 0, FBUS_KERNEL_CORRECT = 1, FBUS_KERNEL_PREDICT_N = 2, FBUS_KERNEL_MARKER_POSE = 3,
       FBUS_KERNEL_FRAME = 4, FBUS_KERNEL_CORRECT_CORNERS = 5, FBUS_KERNEL_COUNT = 6 };
/* When enabled (on >= 1), launches of the listed kernels are bracketed by HIP events on
 * the handle's stream; read() synchronises and returns the summed device time and launch
 * count since the last reset.  fbus_ekf_frame_dev uses ONE pair around its run of K
 * back-to-back predict launches (a pair per launch costs ~8 us of stream time and reads
 * ~3 us long) and brackets only every `on`-th frame (on = 1: every frame). */
int fbus_ekf_timing_enable(fbus_ekf_t h, int on);
int fbus_ekf_timing_reset(fbus_ekf_t h);
int fbus_ekf_timing_read(fbus_ekf_t h, int kernel, double* total_ms, int64_t* launches);

/* ---- correct() from corner PIXELS: the north star's reprojection rows ------------ */
/* No reference counterpart (the reference has only the back-projection VISION::RefractionTriangulation,
 * vision.cpp:472-618).  Measurement = the normalised image points of the four corners of every visible marker in the left
 * camera (right == NULL: 2 rows per corner, 128 rows at 16 markers) or in both cameras (4 rows per corner).
 * h = pi(X_k(x)): X_k = R_IL R'(P_m + R_m c_k - p - R P_IL) the corner in the left camera frame (the geometry of
 * MeasureUpdate.m:67,72-73 with the corner in place of the marker origin), pi = the flat-port forward projection
 * (air -> glass -> water, the inverse of the ray construction of vision.cpp:505-552, in the plane of the port normal and the
 * point: a closed-form thin-port start taken twice, then ONE Halley step in double -- two for fp64 records --; no iteration).
 * Per-corner Jacobian rows (2 x N) = d pi/dX (closed form) x [ -R_IL R' | R_IL [R'(c_w - p)]x ];
 * all rows of all visible markers at one linearisation point, folded into the 6x6 information matrix; the update is the one-shot
 * form  P(J,:) <- G P(J,:),  P_rr -= x_a' S^-1 x_c  (symmetric by construction, nothing cancels on the rows the measurement
 * shrinks).  fbus_params::cov_form DOES NOT APPLY to this entry point nor to fbus_ekf_correct_corners: FBUS_COV_JOSEPH selects
 * nothing here (the one-shot form already has what Joseph's form is chosen for); it governs fbus_ekf_correct only.  The one form
 * is checked against BOTH forms of the oracle -- (I - K H) P, MeasureUpdate.m:101-102, and Joseph's (I - K H) P (I - K H)' + K R K',
 * what north_star names: fp64 records 1e-9, fp32 the standard gates (tests/test_pixels_gpu.py::test_correct_pixels_matches_the_oracle,
 * tests/test_vision_gpu.py::test_correct_from_stereo_corners_matches_oracle).
 * left / right must be 16-byte aligned (any allocation is): the slots are fetched with 16-byte loads, FBUS_ERR_INVALID otherwise.
 * ids (B, M), left / right (B, M, 8) = x0 y0 .. x3 y3 (the column layout of corners.txt, vision.cpp:111-119). */
int fbus_ekf_correct_pixels(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right /* may be NULL */,
                            const uint8_t* skip);
int fbus_ekf_correct_pixels_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right,
                                const uint8_t* skip);

/* ---- NIS output and chi-square gating of the measurement updates ---------------------------------------------------
 * fbus_ekf_correct (the pose rows), fbus_ekf_correct_pixels and fbus_ekf_correct_corners with, per filter, the normalised innovation squared of the rows the update applies, evaluated at the prior,
 *     nis = r' S^-1 r,   S = H P H' + R      (the matrix MeasureUpdate.m:84 inverts; filter.cpp:709-712 solves with LDLT)
 * and its dof = the number of rows that carry a residual:
 *   pixel rows   2 per projection the fold gives non-zero weight (in front of the port and inside its field of view, marker in the
 *                map): at most 8 per marker for the left camera, 16 for stereo;
 *   corner rows  3 per corner of each used marker (12 per marker; nearest mode: the chosen marker only);
 *   pose rows    3 per used marker in the Matlab dialect (its quaternion residual is zeroed, MeasureUpdate.m:88: those rows enter S
 *                but carry no residual), 7 in the C++ dialect; nearest mode: the chosen marker only.
 * A filter that is skipped or has no usable marker reports nis = 0, dof = 0 and is left untouched, as by the twin.  No S is formed:
 * with Lam = H_J' R^-1 H_J, b = H_J' R^-1 r (the 6 x 6 fold the update already builds) and m = (I + P_JJ Lam)^-T b,
 *     nis = sum res^2 / r - b' P_JJ m          (S^-1 r = R^-1 (r - H dx), dx_J = P_JJ m), in double for both record types;
 * the pose rows:  nis = sum w res^2 - b' (P_JJ^-1 + Lam)^-1 b, through P_JJ = C C' and the Cholesky factor of I + C' Lam C.
 * GATE: fbus_ekf_set_gate stores a table thr[0 .. n-1] indexed by dof.  With a table, a filter whose update would run is left
 * untouched when nis > thr[dof]: its record stays bit-identical (the C++ dialect's previous-marker id included), applied = 0, and
 * nis / dof are still reported.  The decision is made after the 6 x 6 stage, in front of the first store.  +inf entries never
 * reject; NaN or negative entries are refused (FBUS_ERR_INVALID, table unchanged), as are n > FBUS_GATE_MAX_DOF + 1 entries.
 * n = 0 or thresholds = NULL: no gate.  A call whose largest possible dof (M x 8 x cameras; corners: 12, or 12 M stacked; pose: 3 / 7,
 * or 3 M / 7 M stacked) has no
 * entry (>= n) fails with FBUS_ERR_INVALID before anything is launched.  set_gate copies the table into handle-owned device
 * memory in order on the handle's stream and waits for the copy; it is refused between graph_begin and graph_end; a captured
 * _nis_dev call reads the table that is current when the graph is replayed (entries past the current n read as +inf).
 * The existing entry points ignore the table.
 * nis: B values in the handle's dtype, dof: B int32; either may be NULL; host pointers for the host forms, device pointers for
 * _dev.  Arguments, checks and alignment rules are those of each twin.  With no table, records and applied equal the twin's bit for
 * bit on the route the twin takes for one wave per tile.  The pixel / corner forms always run that route; on small launches
 * (fewer tiles than half the chip's SIMDs, unless fbus_ekf_set_team(h, ., 1)) the twins divide the markers among 2-4 waves per tile
 * and add their sums in another order, and the two agree to rounding (the single-step gate).  The pose form takes the twin's
 * kernel choice except the fp32 row-split kernel of stacked, simple-form launches of more than one wave per SIMD (> 65 536 filters
 * on a 256-CU part), where it keeps the one-wave kernel: a different pass order, equal to rounding.  One pose route is not bit-identical
 * even so: fp64 records, C++ dialect, stacked mode -- the covariance is, the nominal state differs from the twin's in the last bits
 * (measured <= 2e-15 absolute; the single-step gate holds). */
#define FBUS_GATE_MAX_DOF 256      /* largest dof: 16 markers x 4 corners x 2 cameras x 2 rows; a full table has 257 entries */
int fbus_ekf_set_gate(fbus_ekf_t h, int n, const double* thresholds /* host, n entries; n = 0 or NULL: no gate */);
int fbus_ekf_correct_nis(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode,
                         const uint8_t* skip, void* nis, int32_t* dof);
int fbus_ekf_correct_nis_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode,
                             const uint8_t* skip, void* nis, int32_t* dof);
int fbus_ekf_correct_pixels_nis(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right,
                                const uint8_t* skip, void* nis, int32_t* dof);
int fbus_ekf_correct_pixels_nis_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right,
                                    const uint8_t* skip, void* nis, int32_t* dof);
int fbus_ekf_correct_corners_nis(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, int geometry,
                                 int mode, const uint8_t* skip, void* nis, int32_t* dof);
int fbus_ekf_correct_corners_nis_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, int geometry,
                                     int mode, const uint8_t* skip, void* nis, int32_t* dof);

/* ---- per-filter process and measurement noise -------------------------------------------------------------------------
 * Every filter of a handle takes q_diag, r_pos, r_quat and r_pix from fbus_params until a table is set.  fbus_ekf_set_noise
 * gives each filter its own: a B x FBUS_NOISE_COLS table, row-major, fp64 for both record types, columns
 *     q_v q_theta q_ba q_bg r_pos r_quat r_pix      (= fbus_params q_diag[0..3], r_pos, r_quat, r_pix)
 * Filter b then runs the arithmetic of a handle whose fbus_params hold row b's values: the kernels convert each entry to the record
 * type as the handle converts fbus_params ((T)q on the device equals the host's (T)prm.q_diag[i]; 1 / r_pix and 1 / r_pos are formed
 * from the same double).  The NIS forms use the filter's own R in S = H P H' + R.  What stays shared: the gate table (indexed by dof),
 * switch_thres, p0_diag (fbus_ekf_set_state takes per-filter P), the camera, port and marker constants.
 * STORAGE: the handle owns one device buffer, allocated at the first set_noise and kept until destroy, holding the table as fields
 * [FBUS_NOISE_COLS][B] in double; later calls rewrite the same buffer in place.  A captured graph (fbus_ekf_graph_*) that ran with a
 * table therefore sees the values current at its replay.  A graph captured without a table keeps the kernels it captured (it reads
 * fbus_params as they were at capture).  set_noise / set_noise_dev / get_noise are refused between graph_begin and graph_end.
 * ROUTES with a table: the one-wave-per-tile kernels only.  The team forms (fbus_ekf_set_team is ignored while a table is set, and
 * fbus_ekf_launch_info reports ROLES_* = 1, TEAM_FRAMES = 0, MEAS_SPLIT = 0) and the divided pixel update are bypassed.
 * fbus_ekf_frame*_fused_dev and the windows take resident kernels that read the table where an untabled handle of the same policy
 * batch runs the one-wave resident kernels: fp32 records, likelihood sums off, policy batch above half a chip
 * (FBUS_INFO_NOISE_RESIDENT; not (Joseph, nearest) pose rows, M = 0, FBUS_NO_FRAME_MEAS, as without a table).  Filter b of such a window
 * equals, bit for bit, the untabled resident window of a handle with row b's values in fbus_params, and the window equals its fused frames
 * bit for bit (the single-frame entry points launch the same kernels with one frame); it equals the per-call sequence to fp32 rounding,
 * as every untabled window does.  Elsewhere (at or below half a chip, the sums on, fp64 records) they run frame by frame, bit-equal to
 * predict_n + the per-call update (trajectory rows from the snapshot kernel).  The plain updates run the NIS kernels with no outputs and no gate: records equal a handle with the row's
 * values in fbus_params on its one-wave route bit for bit, except fp64 C++-dialect stacked pose updates (nominal state within ~2e-15,
 * see the NIS section above).
 * fbus_ekf_set_noise     host table; every entry must be finite, q >= 0 and r > 0 (as fbus_params_validate).  A bad entry returns
 *                        FBUS_ERR_INVALID with its row and column in fbus_ekf_last_error and leaves the previous table (or none) in
 *                        force.  Copied in order on the handle's stream; returns after the copy.  NULL: no table (back to fbus_params).
 * fbus_ekf_set_noise_dev device table, stream-ordered on the handle's stream (the caller keeps it alive until the stream has passed the
 *                        call).  Like every _dev entry point it does NOT inspect the values: the caller validates them (the Python
 *                        mirror does, with torch).  NULL: no table.
 * fbus_ekf_get_noise     the current table into a host B x FBUS_NOISE_COLS array (waits for the stream); FBUS_ERR_INVALID when no table
 *                        is set. */
#define FBUS_NOISE_COLS 7   /* q_v q_theta q_ba q_bg r_pos r_quat r_pix -- the fbus_params fields of the same names */
int fbus_ekf_set_noise(fbus_ekf_t h, const double* table);      /* host, B x 7 row-major; NULL = no table (back to fbus_params) */
int fbus_ekf_set_noise_dev(fbus_ekf_t h, const double* table);  /* device, B x 7 row-major, stream-ordered; NULL = no table      */
int fbus_ekf_get_noise(fbus_ekf_t h, double* table);            /* host, B x 7; FBUS_ERR_INVALID when no table is set          */

/* ---- per-filter innovation log-likelihood (the evidence of a noise hypothesis) -------------------------------------------
 * NIS cannot rank noise hypotheses: it falls as R or the prior grow.  The quantity that can is the Gaussian log-likelihood of each
 * applied update's innovation,
 *     ll = -1/2 ( r' S^-1 r + log det S + rows ln 2 pi ),      S = H P H' + R,
 * summed over a run.  The handle owns a per-filter accumulator, fed by EVERY measurement update it launches while accumulation is on
 * (correct*, correct*_nis*, host-pointer, _dev and _async forms, frame*, frames*, captured graphs):
 *   * an update that is applied:        ll += -1/2 (nis + log det S + rows ln 2 pi),  rows += rows of S,  applied += 1
 *   * an update the gate rejects:       rejected += 1, nothing else
 *   * a skipped filter, or one with no usable marker (dof = 0): nothing
 * all in double for both record types (nis is the double the NIS kernels hold before its cast to the record type; log det S =
 * log det R + log det(I + P_JJ Lam) from the Cholesky pivots the update has anyway, R from the filter's own table row when a noise
 * table is set).  `rows` is the row count of S.  It equals the reported dof everywhere EXCEPT the Matlab dialect's pose rows: there the
 * quaternion residual is zeroed but its four rows stay in S (MeasureUpdate.m:84-88), so rows = 7 and dof = 3 per used marker, and
 * log det R counts all seven.
 * STORAGE: one device buffer, allocated at the first enable(h, 1) and neither moved nor freed before fbus_ekf_destroy, so a captured
 * graph accumulates at every replay.  A graph captured while accumulation was on keeps its kernels: it goes on accumulating after
 * enable(h, 0).  enable and get are refused between graph_begin and graph_end; reset and get_dev are stream-ordered and may be captured.
 * ROUTES while on: as with a noise table (above) -- the one-wave-per-tile kernels only, fbus_ekf_set_team ignored, fbus_ekf_launch_info
 * reports ROLES_* = 1, TEAM_FRAMES = 0, MEAS_SPLIT = 0, the fused frame and window entry points run frame by frame (predict_n + the
 * per-call update).  The updates run the tabled kernels; without a noise table the handle writes fbus_params' own values into its table
 * buffer (fbus_ekf_get_noise still answers "no table", predict keeps its untabled kernels), so records, applied, nis and dof equal the
 * same call with accumulation off on its one-wave route bit for bit, except fp64 C++-dialect stacked pose updates (nominal state within
 * ~2e-15, as with a table).  Off (the default) nothing is routed differently.
 * fbus_ekf_loglik_enable   on != 0: accumulate from the next launch on (first time: allocate and zero); on == 0: stop, keep the sums
 * fbus_ekf_loglik_reset    zero the sums, stream-ordered on the handle's stream
 * fbus_ekf_loglik_get      the sums into host arrays of B entries each (any may be NULL); waits for the stream
 * fbus_ekf_loglik_get_dev  the same into device arrays, stream-ordered
 * All four return FBUS_ERR_INVALID (1) for a NULL handle; get / get_dev / reset before the first enable(h, 1) are FBUS_ERR_INVALID with
 * a fbus_ekf_last_error text. */
int fbus_ekf_loglik_enable(fbus_ekf_t h, int on);
int fbus_ekf_loglik_reset(fbus_ekf_t h);
int fbus_ekf_loglik_get(fbus_ekf_t h, double* ll, int64_t* rows, int32_t* applied, int32_t* rejected);
int fbus_ekf_loglik_get_dev(fbus_ekf_t h, double* ll, int64_t* rows, int32_t* applied, int32_t* rejected);

/* ---- hypothesis groups: evidence-weighted fusion, collapse and IMM mixing (NO reference counterpart) ---------------------------
 * The reference runs one filter on one thread (C++/src/filter.cpp:190-250) and has no bank of hypotheses; these three calls are what a
 * multiple-model bank does with the evidence above.  Group j holds the G consecutive filters j G .. j G + G - 1 (the layout a noise
 * grid of G hypotheses has when G divides B), 2 <= G <= FBUS_GROUP_MAX, B % G == 0, any G in that range (a 3 x 3 grid is G = 9).
 * Groups are per handle.
 *
 * fbus_ekf_group_fuse: per-filter log-weights -> weights, the best member, and the moment-matched state and covariance of each group.
 *   logw     [B] double; NULL = the handle's likelihood sums `ll` (the accumulator never moves: a captured call reads the sums current at
 *            its replay; FBUS_ERR_INVALID before the first fbus_ekf_loglik_enable(h, 1))
 *   weight   [B] double            best  [B/G] int32 (member index 0..G-1, or -1)
 *   nominal  [B/G][19], P [B/G][N][N], pdiag [B/G][N] in the handle's dtype and in fbus_ekf_get_state's order
 *   Every output may be NULL (not written).  Members i = 0..G-1 of one group, in member order throughout:
 *   1. member i is usable iff logw[i] is finite (NaN, +inf, -inf exclude it).  No usable member: weight = 0 for the whole group,
 *      best = -1, and nominal, P, pdiag are member 0's own values, copied.
 *   2. m = the largest usable logw; e_i = exp(logw_i - m), s = sum e_i, w_i = e_i / s in double; an excluded member gets exactly 0;
 *      best = the smallest i with logw_i == m.
 *   3. The chart is the best member's nominal state x*.  delta_i in R^N, error-state order p v theta ba bg [g]: plain differences
 *      against x* except delta_theta_i = Log(conj(q*) (x) q_i): d = conj(q*) (x) q_i, negated if d_w < 0, n = |d_vec|,
 *      delta_theta = (2 atan2(n, d_w) / n) d_vec (0 when n == 0) -- the inverse of the injection q <- normalize(q (x) dq(dtheta))
 *      (matlab/MeasureUpdate.m:92-98).  d and delta_theta are formed in double for both record types.
 *   4. mu = sum w_i delta_i.  The fused nominal is x* + mu on p, v, ba, bg (and g for N = 18; g of the best member for N = 15) and
 *      q = normalize(q* (x) dq(mu_theta)).
 *   5. Pbar = sum w_i (P_i + (delta_i - mu)(delta_i - mu)'), symmetric by construction; pdiag is its diagonal.  Each P_i stays in its
 *      own member's tangent space: the first-order transport of P_i to the chart x* is omitted, as in standard IMM mixing.
 *   6. A member with weight exactly 0 is skipped by a select, not multiplied by 0: a diverged hypothesis (NaN in its record, logw NaN
 *      or -inf) does not poison its group.
 *   7. The records, the applied flags, the likelihood sums and the noise table are not touched.
 *   8. Every sum runs in member order: two calls on the same inputs give bit-identical outputs whatever the batch size.
 *
 * fbus_ekf_group_collapse: for every group with src[j] in 0..G-1, every member's whole packed record (nominal state, carried rotation,
 *   packed covariance, prev_id) becomes member src[j]'s record, bit for bit.  Any other src[j] -- negative is the documented way to
 *   skip a group, and `best` of group_fuse is -1 for a group without a usable member, so it can be passed straight in -- leaves the
 *   group's bytes alone; the device form inspects nothing and the kernel never forms an address from such a value.  NOT copied: the
 *   applied flags, the likelihood sums, the noise table and the carried IMU-EMA sample.
 *
 * fbus_ekf_group_mix: the mixing step of the interacting-multiple-model (IMM) estimator, in place: between two stretches of
 *   measurements every member of a group is re-initialised from a mixture of all members, weighted by the model probabilities and a
 *   model-transition matrix.  collapse is its degenerate case (every column of the mixing matrix one-hot on one source), fuse its
 *   rank-one case (every target gets the same mixture).
 *   logw     [B] double, log model probabilities up to a per-group constant; NULL = the handle's likelihood sums, by the rule and with
 *            the error of fuse
 *   trans    [G][G] double, row-major: trans[i][j] = Pi_ij, the probability that model i is followed by model j; one matrix for all
 *            groups of the call (a device pointer in the _dev form, a host pointer in the host form)
 *   weight   [B] double, may be NULL: mu_i, steps 1-2 of fuse
 *   logc     [B] double, may be NULL: log c_j, the predicted model probability -- the caller adds the next stretch's `ll` to it to get
 *            the next logw
 *   Members i (sources) and j (targets) of one group, in member order throughout:
 *   1. mu_i as in steps 1-2 of fuse: usable iff logw_i is finite, exactly 0 otherwise.  No usable member: no record of the group
 *      changes, weight = 0 and logc = -inf for all its members.
 *   2. c_j = sum_i Pi_ij mu_i and W_ij = Pi_ij mu_i / c_j, in double.  c_j == 0 (in the device form, which inspects nothing: anything
 *      but c_j > 0): target j keeps its bytes and logc_j = -inf.
 *   3. The chart is the record of the best member, x* (fuse's `best`); delta_i exactly as in step 3 of fuse, in double with atan2;
 *      m_j = sum_i W_ij delta_i.
 *   4. Target j's new nominal state is x* with m_j injected by the update's own injection (MeasureUpdate.m:92-98), as in step 4 of
 *      fuse.  Its carried rotation is the chart member's, bit for bit: mixing is an injection into x*, and the measurement update leaves
 *      the carried rotation alone.  A target whose own record was NaN is thereby wholly re-seeded.  For N = 15, g is the chart's.
 *   5. P0_j = sum_i W_ij (P_i + (delta_i - m_j)(delta_i - m_j)'), stored packed (symmetric by construction) and rounded once to the
 *      record type.  No transport between tangent spaces, as in step 5 of fuse.
 *   6. A source with W_ij exactly 0 is skipped, not multiplied by 0 (mu_i = 0 and Pi_ij = 0 alike: a NaN record behind it cannot
 *      reach target j).  A target with W_jj == 1 exactly keeps its bytes: Pi = I changes nothing, bit for bit.
 *   7. Written in place: the nominal state, the carried rotation and the packed covariance of every rewritten target.  Each member keeps
 *      its own prev_id.  The applied flags, the likelihood sums, the noise table and the carried IMU-EMA sample are not touched.
 *   8. Every sum runs in member order: the results do not depend on the batch size or on the group's place in it, and two runs are
 *      bit-identical.
 *   The cycle this enables, all on the device:  logc = log prior;  loop { loglik_reset; a window of frames; logw = logc + ll;
 *   group_fuse(G, logw) -> the output estimate;  group_mix(G, trans, logw) -> weight, logc }.
 *
 * The _dev forms take device pointers, are stream-ordered on the handle's stream and may be captured in a graph; the host forms stage
 * their arrays and wait.  All checks are made before anything is launched: a NULL handle is FBUS_ERR_INVALID; G out of range or
 * B % G != 0, an output that overlaps the records (the rule of fbus_ekf_snapshot_dev), src == NULL, trans == NULL, in the host form of
 * collapse an entry >= G, and in the host form of mix a trans entry that is not finite or is negative or a row sum further than 1e-9
 * from 1 (the text names the row) are FBUS_ERR_INVALID with a fbus_ekf_last_error text; the _dev form of mix inspects nothing.
 * Added under ABI 8 without a bump: detect the feature by symbol. */
#define FBUS_GROUP_MAX 64
int fbus_ekf_group_fuse_dev(fbus_ekf_t h, int G, const double* logw, double* weight, int32_t* best, void* nominal, void* P, void* pdiag);
int fbus_ekf_group_fuse(fbus_ekf_t h, int G, const double* logw, double* weight, int32_t* best, void* nominal, void* P, void* pdiag);
int fbus_ekf_group_collapse_dev(fbus_ekf_t h, int G, const int32_t* src);
int fbus_ekf_group_collapse(fbus_ekf_t h, int G, const int32_t* src);
int fbus_ekf_group_mix_dev(fbus_ekf_t h, int G, const double* logw, const double* trans, double* weight, double* logc);
int fbus_ekf_group_mix(fbus_ekf_t h, int G, const double* logw, const double* trans, double* weight, double* logc);

/* ---- depth (pressure) sensor update (NO reference counterpart) ---------------------------------------------------------------
 * The reference names three sensors -- `namespace FBUSEKF // Underwater Vision IMU Depth EKF` (C++/include/common.hpp:16) -- and
 * implements two: it has no depth update to follow, so the model is stated here.  predict is the IMU, correct* are vision and need
 * a marker in view; this is the one absolute measurement a vehicle has between sightings: one scalar row per filter.
 *
 * The sensor, per handle, set once:
 *   fbus_ekf_set_depth_sensor(h, axis, offset, lever)
 *     axis    world-frame direction along which the reading grows; normalised by the host in double.  A zero or non-finite axis is
 *             FBUS_ERR_INVALID with the reason in fbus_ekf_last_error (the previous sensor, or none, stays).
 *     offset  the reading at the world origin (finite)
 *     lever   the sensor's position in the IMU frame; NULL = 0
 *   The three go to the kernel BY VALUE as doubles: a captured graph keeps the values it was captured with, whatever is set later.
 *   Refused between graph_begin and graph_end.  Until it has been called every correct_depth* form returns FBUS_ERR_INVALID with a
 *   fbus_ekf_last_error text that names fbus_ekf_set_depth_sensor: there is no silent default axis.
 *
 * The row.  R = the record's CARRIED rotation (the possibly stale, not re-orthonormalised one the pose rows use), error convention
 * of the injection q <- q (x) dq(dtheta) (MeasureUpdate.m:92-98), error-state order p v theta ba bg [g]:
 *     h(x)  = axis . (p + R lever) + offset
 *     H_p   = axis'                      (columns 0..2)
 *     H_th  = (lever x (R' axis))'       (columns 6..8)           every other column 0
 *     res   = z - h(x)         S = H P H' + var         u = P H'  (reads the p and theta columns of P only)
 *     dx    = u res / S  -> the update's own injection;   P <- P - u u' / S
 * For one row the reference's literal (I - K H) P, its Joseph form and P - u u' / S are the same matrix: the kernel has the one
 * symmetric form for both settings of fbus_params::cov_form, and does not read the dialect.  The carried rotation and prev_id are
 * not written (MeasureUpdate writes neither).
 *
 *   z              [B] readings in the handle's dtype
 *   var            the reading's variance, ALWAYS double (as the noise table): 1 value (var_per_filter = 0) or [B] (var_per_filter = 1);
 *                  filter b with var[b] runs bit for bit what a handle with the scalar var[b] runs
 *   skip           [B] bytes, nonzero = leave the filter alone; may be NULL
 *   nis, dof       (_nis forms) [B] in the handle's dtype / int32; each may be NULL
 * A filter is LEFT UNTOUCHED -- record bytes unchanged, applied = 0, nis = 0, dof = 0, likelihood sums unchanged -- when it is
 * skipped, when z[b] is not finite, or when its var is not a finite number > 0: a per-lane decision, a bad input of one filter
 * never reaches another.  Otherwise nis = res^2 / S, dof = 1, and the update is APPLIED IFF S > 0 and nis <= thr[1] of the handle's
 * gate table (fbus_ekf_set_gate; +inf without one or with a shorter one); both comparisons are false for a NaN -- the rule of
 * fbus_ekf_correct_velocity and fbus_ekf_correct_rows below, S being the one pivot: a record of NaN (nis is NaN) and a record whose
 * covariance makes S <= 0 are not applied.  The decision is made before the first store, in EVERY form.  A lane that is not applied
 * keeps its record and reports applied = 0, its nis (possibly NaN) and dof = 1.  While fbus_ekf_loglik_enable is on, an applied update
 * adds -1/2 (nis + ln S + ln 2 pi) to ll, 1 to rows and 1 to applied; one that is not applied adds 1 to rejected alone.  The innovation, h, S,
 * 1 / S, nis and ll are formed in double for both record types -- and so are u = P H', the gain and the covariance pass: with fp32
 * records every covariance element is P - u u' / S in double, rounded ONCE to the record (as in fbus_ekf_correct_velocity), because
 * the update of a grown prior subtracts nearly equal numbers along its row (a 1 m prior beside var = 1e-4 leaves the fp32 pass 2e-3
 * of the posterior variance, the double pass the rounding of the record, 1e-4).  fp64 records do the pass in the record type.
 * fbus_ekf_get_applied reports the flags of the last update, as after correct*.
 * One kernel, one wave per 64-filter tile at every batch size: fbus_ekf_set_team, the policy batch, a noise table and the
 * likelihood switch do not change the route, and the plain, _nis and likelihood-on calls are the same code object -- records and
 * applied are bit-equal between all five forms.
 * The argument check runs before anything is staged, in this order: NULL handle (FBUS_ERR_INVALID, no text), sensor not set,
 * NULL z / var, var_per_filter not 0 or 1 -- the last three with the entry point's name in fbus_ekf_last_error.
 * _dev: device pointers, stream-ordered, capturable.  _async: host pointers through the pinned ring (the rules of
 * fbus_ekf_predict_async).  Added under ABI 8 without a bump: detect the feature by symbol. */
int fbus_ekf_set_depth_sensor(fbus_ekf_t h, const double axis[3], double offset, const double lever[3] /* may be NULL */);
int fbus_ekf_correct_depth(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip);
int fbus_ekf_correct_depth_dev(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip);
int fbus_ekf_correct_depth_async(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip);
int fbus_ekf_correct_depth_nis(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip,
                               void* nis, int32_t* dof);
int fbus_ekf_correct_depth_nis_dev(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip,
                                   void* nis, int32_t* dof);

/* ---- body-velocity (DVL) update (NO reference counterpart) -----------------------------------------------------------------------
 * The reference has no velocity update, so the model is stated here, as it is for depth.  Between marker sightings the depth row
 * holds one axis of position and nothing measures velocity: the horizontal axes of p, all of v and the accelerometer bias free-run on
 * the integrated accelerometer.  A Doppler velocity log measures the velocity of the vehicle over ground in the instrument's own
 * frame; a zero-velocity update (ZUPT) of a vehicle sitting on the bottom is the same measurement with z = 0.
 *
 * The sensor, per handle, set once:
 *   fbus_ekf_set_velocity_sensor(h, mount, lever)
 *     mount   const double[9], row-major: the rotation C from the IMU frame to the instrument frame; NULL = identity.  Refused
 *             (FBUS_ERR_INVALID, text in fbus_ekf_last_error, previous sensor kept) when an entry is not finite or
 *             max |C C' - I| > 1e-6.
 *     lever   const double[3], the instrument's position in the IMU frame; NULL = 0.  Must be finite.
 *   Both go to the kernel BY VALUE as doubles: a captured graph keeps what it was captured with.  Refused between graph_begin and
 *   graph_end.  Until it has been called every correct_velocity* form returns FBUS_ERR_INVALID with a fbus_ekf_last_error text that
 *   names fbus_ekf_set_velocity_sensor: there is no silent default.
 *
 * The rows.  R = the record's CARRIED rotation, the one the pose rows and the depth row use; error convention of the injection
 * q <- q (x) dq(dtheta) (MeasureUpdate.m:92-98); error-state order p v theta ba bg [g]; w = gyro - bg:
 *     h(x)  = C (R' v + w x lever)                      3 rows
 *     H_v   = C R'            (columns 3..5)
 *     H_th  = C [R' v]x       (columns 6..8)
 *     H_bg  = C [lever]x      (columns 12..14)          every other column 0
 *     res = z - h     S = H P H' + diag(var)     U = P H' (N x 3)
 *     dx = U S^-1 res -> the update's own injection      P <- P - U S^-1 U'
 * Processing the three rows one after another AT THE ONE linearisation point gives the same dx, P, nis and log det S as the joint
 * solve: u = P h_k, s_k = h_k . u + var_k, r_k = res_k - h_k . dx, dx += u r_k / s_k, P -= u u' / s_k; nis = sum r_k^2 / s_k and
 * ln det S = sum ln s_k.  Either form may be the kernel's; the s_k are the squares of the Cholesky pivots of S, so "pivot" below
 * means the same number in both forms.
 *
 *   z              [B][3] in the handle's dtype
 *   gyro           [B][3] in the handle's dtype, the raw rate sample that predict takes; may be NULL: the w x lever term is then
 *                  dropped from h and H_bg = 0 -- the columns 12..14 are then EXACTLY untouched by H
 *   var            ALWAYS double, as for depth: 3 values (var_per_filter = 0) or [B][3] (var_per_filter = 1); filter b under
 *                  var[b][:] runs bit for bit what a handle under those three scalars runs
 *   skip           [B] bytes, nonzero = leave the filter alone; may be NULL
 *   nis, dof       (_nis forms) [B] in the handle's dtype / int32; each may be NULL
 * A filter is LEFT UNTOUCHED -- record bytes unchanged, applied = 0, nis = 0, dof = 0, likelihood sums unchanged -- when it is
 * skipped, when a component of z is not finite, when a component of gyro is not finite (only when gyro is given), or when one of
 * its three variances is not a finite number > 0.
 * Otherwise dof = 3, and the update is APPLIED IFF all three pivots are > 0 and nis <= thr[3] of the handle's gate table
 * (fbus_ekf_set_gate; +inf without one or with a shorter one); both comparisons are false for a NaN.  The decision is made before
 * the first store, in every form.  A lane that is not applied keeps its record and reports applied = 0, its nis (res' S^-1 res also
 * where a pivot is negative, for both record types; NaN for a record of NaN) and
 * dof = 3; while fbus_ekf_loglik_enable is on it adds 1 to rejected alone.  An applied lane adds -1/2 (nis + ln det S + 3 ln 2 pi)
 * to ll, 3 to rows and 1 to applied.
 * h, res, S, the pivots, nis and ll are formed in double for both record types; H is rounded once to the record type.  U and the
 * covariance pass run in double for BOTH record types, and an fp32 record's covariance elements are rounded once, when they are stored:
 * an update that takes the velocity variance from a loose prior down to the instrument's subtracts numbers that agree in their leading
 * digits, and in fp32 arithmetic the posterior would keep only eps32 x prior / posterior of its own size.  dx is formed in the record type.  The carried rotation and prev_id are not written; cov_form and the dialect are not
 * read; for N = 15, g is left alone.  fbus_ekf_get_applied reports the flags of the last update, as after correct*.
 * One kernel, one wave per 64-filter tile at every batch size: fbus_ekf_set_team, the policy batch, a noise table and the
 * likelihood switch do not change the route, and the plain, _nis and likelihood-on calls are the same code object -- records and
 * applied are bit-equal between all five forms.  Not available inside the frame windows.
 * The argument check runs before anything is staged, in this order: NULL handle (FBUS_ERR_INVALID, no text), sensor not set,
 * NULL z / var, var_per_filter not 0 or 1 -- the last three with the entry point's name in fbus_ekf_last_error.
 * _dev: device pointers, stream-ordered, capturable.  _async: host pointers through the pinned ring (the rules of
 * fbus_ekf_predict_async).  Added under ABI 8 without a bump: detect the feature by symbol. */
int fbus_ekf_set_velocity_sensor(fbus_ekf_t h, const double mount[9] /* may be NULL */, const double lever[3] /* may be NULL */);
int fbus_ekf_correct_velocity(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter, const uint8_t* skip);
int fbus_ekf_correct_velocity_dev(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter,
                                  const uint8_t* skip);
int fbus_ekf_correct_velocity_async(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter,
                                    const uint8_t* skip);
int fbus_ekf_correct_velocity_nis(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter,
                                  const uint8_t* skip, void* nis, int32_t* dof);
int fbus_ekf_correct_velocity_nis_dev(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter,
                                      const uint8_t* skip, void* nis, int32_t* dof);

/* ---- the general linearised measurement update (NO reference counterpart) ------------------------------------------------------
 * Depth and body velocity are built in; a compass, an acoustic position fix, a range to a beacon and whatever else a vehicle carries
 * are not, and do not need to be: the caller forms the innovation and the Jacobian rows of its sensor, the library does the gain, the
 * injection, the covariance, the NIS, the gate and the likelihood on the packed records.  (fbus_ekf.rows in the Python package has
 * three such sensors ready made: position_fix, direction, range_to.)
 *
 *   m              1..FBUS_ROWS_MAX rows per filter, the same for every filter of the call
 *   res            [B][m] in the handle's dtype: the innovation z - h(x) at the current record, formed by the caller
 *   H              [B][m][N] in the handle's dtype, N the handle's nstate (18 or 15); columns in the error-state order
 *                  p v theta ba bg [g]; row k is d h_k / d dx under the injection's convention q <- q (x) dq(dtheta)
 *                  (MeasureUpdate.m:92-98), i.e. R_true ~ R (I + [dtheta]x)
 *                  res and H need only the natural alignment of the element type
 *   var            ALWAYS double, as for depth and velocity: m values (var_per_filter = 0) or [B][m] (var_per_filter = 1); filter b
 *                  under var[b][:] runs bit for bit what a handle under those m scalars runs
 *   skip           [B] bytes, nonzero = leave the filter alone; may be NULL
 *   nis, dof       (_nis forms) [B] in the handle's dtype / int32; each may be NULL
 *
 * The linearisation point is the caller's business: fbus_ekf_get_state_dev(h, nominal, rot, NULL, NULL) gives the nominal state and
 * the CARRIED rotation -- the possibly stale, not re-orthonormalised one that every built-in update (pose, depth, velocity)
 * linearises with.  A caller may form h and H with that rotation or with the rotation of the quaternion; the kernel reads neither
 * R, the dialect nor fbus_params::cov_form.
 *
 *     S = H P H' + diag(var)      U = P H' (N x m)      dx = U S^-1 res -> the update's own injection      P <- P - U S^-1 U'
 * The m rows may be processed one after another at the one linearisation point, with the orthogonalised rows of
 * fbus_ekf_correct_velocity above: the pivots s_k are the squares of the Cholesky pivots of S, nis = sum r_k^2 / s_k
 * = res' S^-1 res and ln det S = sum ln s_k, exactly as defined there.
 *
 * A filter is LEFT UNTOUCHED -- record bytes unchanged, applied = 0, nis = 0, dof = 0, likelihood sums unchanged -- when it is
 * skipped, when one of its m residuals is not finite, when one of its m variances is not a finite number > 0, or when one of its
 * m N entries of H is not finite: a per-lane decision, a bad input of one filter never reaches another.
 * Otherwise dof = m, and the update is APPLIED IFF all m pivots are > 0 and nis <= thr[m] of the handle's gate table
 * (fbus_ekf_set_gate; +inf without one); both comparisons are false for a NaN.  The decision is made before the first store, in
 * every form.  A lane that is not applied keeps its record and reports applied = 0, its nis (as for the velocity update: finite where
 * a pivot is negative, NaN for a record of NaN) and dof = m; while
 * fbus_ekf_loglik_enable is on it adds 1 to rejected alone.  An applied lane adds -1/2 (nis + ln det S + m ln 2 pi) to ll, m to rows
 * and 1 to applied.  A gate table of n <= m entries has no thr[m]: EVERY form then fails with FBUS_ERR_INVALID before anything is
 * launched (the rule of the _nis updates).
 * An all-zero row of H is legal: its pivot is var_k, it adds res_k^2 / var_k to nis and moves nothing.
 * Not written: the carried rotation and prev_id; for N = 15, g is left alone.  fbus_ekf_get_applied reports the flags of the last
 * update, as after correct*.
 * Precision, as fbus_ekf_correct_velocity: S, the pivots, the orthogonalised residuals, nis and ll are formed in double for both
 * record types; H is used as given, in the record type.  U and the covariance pass run in double for BOTH record types, and an
 * fp32 record's covariance elements are rounded once, when they are stored; dx is formed in the record type.  (fp64 records take
 * the sequential rows in the record type, which is double.)
 * One kernel family, one wave per 64-filter tile at every batch size: fbus_ekf_set_team, the policy batch, a noise table and the
 * likelihood switch do not change the route, and the plain, _nis and likelihood-on calls are the same code object -- records and
 * applied are bit-equal between all four forms.  Not available inside the frame windows.
 * The argument check runs before anything is staged, in this order: NULL handle (FBUS_ERR_INVALID, no text), m outside
 * 1..FBUS_ROWS_MAX, NULL res / H / var, var_per_filter not 0 or 1, a gate table that does not reach thr[m] -- the last four with
 * the entry point's name in fbus_ekf_last_error.
 * _dev: device pointers, stream-ordered, capturable.  The host forms stage their arrays, launch and wait; they are refused between
 * graph_begin and graph_end.  There is NO _async form: res and H are functions of the device-resident state, so a host array of
 * them implies the very round trip (state to the host, rows back) that the async forms exist to avoid -- a caller with that need
 * forms its rows on the device and calls _dev.
 * Why FBUS_ROWS_MAX is 3: for fp32 records the joint form keeps m N doubles beside the covariance, and the velocity kernel's budget
 * at m = 3 is 442 of the 512 registers; pose-sized stacks are what fbus_ekf_correct* is for.  A sensor with more rows calls twice
 * and relinearises in between, which is ordinary sequential EKF practice.
 * Added under ABI 8 without a bump: detect the feature by symbol. */
#define FBUS_ROWS_MAX 3
int fbus_ekf_correct_rows(fbus_ekf_t h, int m, const void* res, const void* H, const double* var, int var_per_filter, const uint8_t* skip);
int fbus_ekf_correct_rows_dev(fbus_ekf_t h, int m, const void* res, const void* H, const double* var, int var_per_filter,
                              const uint8_t* skip);
int fbus_ekf_correct_rows_nis(fbus_ekf_t h, int m, const void* res, const void* H, const double* var, int var_per_filter,
                              const uint8_t* skip, void* nis, int32_t* dof);
int fbus_ekf_correct_rows_nis_dev(fbus_ekf_t h, int m, const void* res, const void* H, const double* var, int var_per_filter,
                                  const uint8_t* skip, void* nis, int32_t* dof);

/* ---- per-marker chi-square screening of a frame's marker slots ----------------------------------------------------------------
 * The reference drops single detections in front of the update (VISION::RejectInvalidMarker, C++/src/vision.cpp:825-853, called once
 * per image at :73: a marker whose apparent motion exceeds markerMoveVelThres loses isComputePose, the rest of the frame goes on to
 * SetDetectionResult).  The gate of the _nis forms judges the WHOLE stacked frame of a filter; this call judges every marker slot on
 * its own -- the individual-compatibility test -- and writes a screened copy of ids with -1 in the rejected slots.  -1 means
 * "absent" in every update, so the existing updates take that copy unchanged, and their whole-frame gate remains the joint test of
 * the survivors.  Nothing but the four outputs is written.
 *
 *   kind           FBUS_SCREEN_POSE / FBUS_SCREEN_PIXELS / FBUS_SCREEN_CORNERS: the update whose rows are judged
 *   ids            [B][M] int32, M in 1..FBUS_MAX_VISIBLE
 *   a, b           the two measurement arrays of the kind's update, with that update's shapes and alignment rules --
 *                  POSE: pos [B][M][3], quat [B][M][4];  PIXELS: left, right [B][M][8] each, right == NULL: the left camera only;
 *                  CORNERS: left, right as fbus_ekf_correct_corners takes them under `geometry`
 *   geometry       CORNERS only (FBUS_VIS_*); ignored for the other two kinds
 *   skip           [B] bytes, nonzero = the filter is not screened; may be NULL
 *   ids_out        [B][M] int32; may be the same pointer as ids (in place); any other overlap is the caller's error
 *   nis, dof       [B][M] in the handle's dtype / int32
 *   kept           [B] int32
 *   Every output may be NULL, in which case it is not written.
 *
 * For filter b and slot m:
 * 1. The slot is JUDGED iff the filter is not skipped and the slot is one the kind's stacked update would fold: its id is in the
 *    marker map and, for pixels, at least one of its projections has non-zero weight (lies in the port's view).  An unjudged slot
 *    gets nis = 0, dof = 0 and ids_out = ids: -1 and unknown ids pass through as they are.
 * 2. nis_m and dof_m are exactly what the kind's _nis entry point defines for a stacked frame that holds slot m alone, evaluated at
 *    the current record: pixels 2 per weighted projection (at most 8 per marker for the left camera, 16 for stereo); corners 12; pose
 *    3 in the Matlab dialect (all 7 rows in S, the quaternion residual zeroed) and 7 in the C++ dialect.  Formed in double for both
 *    record types from the 6 x 6 quantities Lam_m, b_m (the fold's information matrix and vector) and P_JJ (the p / theta block):
 *        nis_m = w sum res^2 - b_m' (P_JJ^-1 + Lam_m)^-1 b_m  =  r_m' (H_m P H_m' + R_m)^-1 r_m
 * 3. R comes from the filter's own row when a noise table is set (r_pix, r_pos, r_quat of fbus_ekf_set_noise), otherwise from
 *    fbus_params.
 * 4. The slot is KEPT iff nis_m <= thr[dof_m], thr = the handle's gate table (fbus_ekf_set_gate); without a table, or past its end
 *    at a replay, thr is +inf.  The decision is made on the double, before the cast: a NaN nis_m (a non-finite detection) is
 *    dropped even without a table.  A record whose p, q, R or P_JJ holds a non-finite value makes EVERY slot of the filter whose id
 *    is in the map judged with nis = NaN, hence dropped; no other filter is touched.  A dropped slot gets ids_out = -1; its nis and
 *    dof are still reported.
 *    kept[b] = the number of slots of filter b whose ids_out is an id of the marker map (what a stacked update of the screened ids
 *    folds); 0 for a skipped filter.
 * 5. With a gate table of n entries, a call whose largest possible per-marker dof (8 x cameras for pixels, 12 for corners, 3 / 7
 *    for pose) has no entry fails with FBUS_ERR_INVALID before anything is launched, as the _nis forms do.
 * 6. Nothing else is written: the records stay byte-identical, and so do the applied flags, the likelihood sums, the noise table,
 *    prev_id and the carried EMA sample.  The nearest-mode rules (the 10 m limit, the hysteresis, switch_thres) are NOT applied: the
 *    screen is mode-agnostic, a nearest-mode update afterwards chooses among the survivors.
 * 7. The argument check runs before anything is staged, in this order: NULL handle (FBUS_ERR_INVALID, no text); then kind, M
 *    (1..FBUS_MAX_VISIBLE), NULL ids / a, an unknown geometry (CORNERS; FBUS_ERR_UNSUPPORTED), a NULL b where the kind needs it (POSE;
 *    CORNERS unless FBUS_VIS_CORNERS3D), alignment (_dev, PIXELS / CORNERS: 16 bytes), r_pix <= 0 (PIXELS), the table size -- each
 *    with the entry point's name in fbus_ekf_last_error.
 * 8. _dev: device pointers, stream-ordered, capturable; a captured call reads the gate table current at its replay (the _nis_dev
 *    rule).  The host form stages, launches, waits and copies back; it is refused between graph_begin and graph_end.
 * One kernel family, one wave per 64-filter tile at every batch size: fbus_ekf_set_team, the policy batch and the likelihood switch
 * do not change the route.  Not available inside the frame windows (a window's later frames would have to be screened at states
 * that do not exist yet) and without an _async form.  Added under ABI 8 without a bump: detect the feature by symbol. */
enum { FBUS_SCREEN_POSE = 0, FBUS_SCREEN_PIXELS = 1, FBUS_SCREEN_CORNERS = 2 };
int fbus_ekf_screen_markers_dev(fbus_ekf_t h, int kind, int M, const int32_t* ids, const void* a, const void* b, int geometry,
                                const uint8_t* skip, int32_t* ids_out, void* nis, int32_t* dof, int32_t* kept);
int fbus_ekf_screen_markers(fbus_ekf_t h, int kind, int M, const int32_t* ids, const void* a, const void* b, int geometry,
                            const uint8_t* skip, int32_t* ids_out, void* nis, int32_t* dof, int32_t* kept);

/* ---- consistency against a truth state: NEES, error and log-density ---------------------------------------------------------------
 * NIS, the gate, the screen and the likelihood sums judge a filter from its innovations.  This call judges it against a KNOWN state --
 * a simulator's or a motion-capture truth, or any reference state (a consensus of a bank, another build's result): with
 * delta = truth (-) estimate, the normalised estimation error squared delta' P^-1 delta of the whole state and of each block, the
 * error itself, and the log-density of the truth under N(estimate, P).  The reference has no counterpart (it runs one filter and is
 * judged off line), so the model is stated here.  Nothing but the three outputs is written.
 *
 *   truth   [B][19] double for both record types (as var and the noise table are), in the order of fbus_ekf_get_state:
 *           p3 v3 q4(wxyz) ba3 bg3 g3.  For N = 15 the last three are ignored.
 *   skip    [B] bytes, nonzero = the filter is not judged; may be NULL
 *   nees    [B][FBUS_NEES_COLS] double
 *   err     [B][N] double, error-state order p v theta ba bg [g]
 *   lnp     [B] double
 *   Every output may be NULL, in which case it is not written.  A call with all three NULL is legal and launches nothing.
 *
 * For filter b:
 * 1. delta is exactly step 3 of fbus_ekf_group_fuse with the estimate as the chart x*: on p, v, ba, bg (and g for N = 18) the plain
 *    difference (double)truth - (double)record, one exact subtraction; delta_theta = Log(conj(q) (x) q_true) with that step's sign rule
 *    and atan2 form, in double for both record types.  q_true is first normalised in double (q / sqrt(w^2 + x^2 + y^2 + z^2)); q is the
 *    record's nominal quaternion, the carried rotation is not read.  err is delta as formed, NaNs included.
 * 2. Column c of nees belongs to an index set J_c of the error state and is delta_J' (P_JJ)^-1 delta_J = |L^-1 delta_J|^2 with
 *    L L' = P_JJ the Cholesky factorisation of that marginal, in double:
 *        FBUS_NEES_FULL   all N states                          dof N
 *        FBUS_NEES_POSE   {0, 1, 2, 6, 7, 8} (p and theta)      dof 6
 *        FBUS_NEES_P, _V, _THETA, _BA, _BG, _G   the 3 x 3 marginals {0..2}, {3..5}, {6..8}, {9..11}, {12..14}, {15..17}, dof 3 each
 *    For N = 15 column FBUS_NEES_G is written as 0.  The dofs are fixed and are not an output.  (The elimination order is free: the
 *    leading k entries of L^-1 delta depend on the leading k x k block only, so a factorisation in the order p, theta, v, ... yields P
 *    and POSE as prefix sums.  This definition, not the order, is the contract.)
 * 3. lnp = -1/2 (nees_FULL + ln det P + N ln 2 pi), ln det P = the sum of the logs of the squared pivots L_ii^2 of the full
 *    factorisation: the log-density of the truth under the estimate, a proper score for comparing tunings when truth is known.
 * 4. A skipped filter gets 0 in every output.  Otherwise a column is NaN iff one of its delta components is not finite or one of its
 *    block's pivots is not > 0 (the comparison is false for NaN); lnp is NaN iff FULL is.  Columns are independent of each other: a NaN
 *    in the record's bg makes BG and FULL (and lnp) NaN and leaves P, V, THETA, BA, G and POSE as they are; a zero or non-finite
 *    q_true makes every column that contains theta (THETA, POSE, FULL) and err's theta entries NaN.  A bad filter never reaches another.
 * 5. Nothing else is written: the records stay byte-identical, and so do the applied flags, the likelihood sums, the noise table,
 *    prev_id and the carried EMA sample.  An output that overlaps the records is refused with FBUS_ERR_INVALID (the rule of
 *    fbus_ekf_snapshot_dev).
 * 6. The argument check runs before anything is staged, in this order: NULL handle (FBUS_ERR_INVALID, no text); NULL truth; an
 *    output that overlaps the records -- the last two with the entry point's name in fbus_ekf_last_error.
 * 7. _dev: device pointers, stream-ordered, capturable; a captured call reads the truth array current at its replay.  nees should be
 *    16-byte aligned (any allocation is).  The host form stages, launches, waits and copies back; it is refused between graph_begin
 *    and graph_end.
 * One kernel family, one wave per 64-filter tile at every batch size: fbus_ekf_set_team, the policy batch, the noise table and the
 * likelihood switch do not change the route, and two calls on the same inputs are bit-identical whatever the batch size or the
 * filter's position in it.  Without an _async form.  Added under ABI 8 without a bump: detect the feature by symbol. */
#define FBUS_NEES_COLS 8
enum { FBUS_NEES_FULL = 0, FBUS_NEES_POSE = 1, FBUS_NEES_P = 2, FBUS_NEES_V = 3, FBUS_NEES_THETA = 4,
       FBUS_NEES_BA = 5, FBUS_NEES_BG = 6, FBUS_NEES_G = 7 };
int fbus_ekf_nees_dev(fbus_ekf_t h, const double* truth, const uint8_t* skip, double* nees, double* err, double* lnp);
int fbus_ekf_nees    (fbus_ekf_t h, const double* truth, const uint8_t* skip, double* nees, double* err, double* lnp);

/* ---- draws from every filter's own Gaussian: the inverse of NEES ----------------------------------------------------------------------
 * fbus_ekf_nees judges a known state against N(estimate, P); this call DRAWS states from it: truth states for a calibration run, start
 * states for a Monte-Carlo run against one truth, the sigma points of every filter, a particle cloud around each member of a bank --
 * without moving a covariance to the host.  The reference has no counterpart, so the model is stated here.  Nothing but the two outputs
 * is written.
 *
 *   S       1..FBUS_SAMPLE_MAX draws per filter in one call: one factorisation serves S products
 *   xi      [S][B][N] double for both record types (as truth and var are): the standard-normal coordinates -- or sigma-point
 *           coordinates -- of the draws, IN THE FACTORISATION ORDER p, theta, v, ba, bg, [g].  They are not inspected: a non-finite
 *           entry gives non-finite entries in that row of that filter and nowhere else.
 *   skip    [B] bytes, nonzero = the filter is not drawn; may be NULL
 *   state   [S][B][19] double, in the order of fbus_ekf_get_state: p3 v3 q4(wxyz) ba3 bg3 g3.  Row [s] is a ready truth array for
 *           fbus_ekf_nees, or -- cast to the record type -- a nominal array for fbus_ekf_set_state.
 *   drawn   [B] bytes
 *   Either output may be NULL, in which case it is not written.  A call with both NULL is legal and launches nothing.
 *
 * For filter b:
 * 1. L is the lower Cholesky factor of Pi P Pi', formed in double for both record types, Pi the permutation (0,1,2, 6,7,8, 3,4,5,
 *    9..N-1) that brings the error state p v theta ba bg [g] into the order p theta v ba bg [g].  The draw is delta = Pi' L xi_s, in
 *    error-state order.  (As in the NEES section the definition is the contract, not the elimination code.  In this order xi's leading
 *    3 and 6 coordinates alone decide delta_p and delta_(p, theta): fed back to fbus_ekf_nees as truth, a row returns
 *    FULL = |xi|^2, POSE = |xi(0..5)|^2, P = |xi(0..2)|^2 and err = delta, up to rounding.)
 * 2. On p, v, ba, bg (and g for N = 18): (double)record + delta, one addition per component.
 * 3. The quaternion, in double: q_out = normalize(q (x) dq(delta_theta)), dq = (cos(|delta_theta| / 2), sin(|delta_theta| / 2) /
 *    |delta_theta| delta_theta), and (1, 0, 0, 0) when |delta_theta| = 0 -- the injection of the measurement updates
 *    (MeasureUpdate.m:92-98) and so the exact inverse of the Log of fbus_ekf_group_fuse's step 3 for |delta_theta| < pi.  q is the
 *    record's nominal quaternion as stored; the carried rotation is not read.
 * 4. For N = 15, g is the record's g.
 * 5. drawn = 1 iff the filter is not skipped and all N pivots L_ii^2 are > 0 (the comparison is false for NaN).  Otherwise drawn = 0
 *    and EVERY row of that filter is its own nominal state, converted to double and otherwise unchanged (a draw with delta = 0, without
 *    the renormalisation).  A bad filter never reaches another.
 * 6. Nothing else is written: the records stay byte-identical, and so do the applied flags, the likelihood sums, the noise table,
 *    prev_id and the carried EMA sample.
 * 7. An output that overlaps the records is refused with FBUS_ERR_INVALID (the rule of fbus_ekf_snapshot_dev).
 * 8. The argument check runs before anything is staged, in this order: NULL handle (FBUS_ERR_INVALID, no text); S out of range; NULL
 *    xi; an output that overlaps the records -- the last three with the entry point's name in fbus_ekf_last_error.
 * 9. _dev: device pointers, stream-ordered, capturable; a captured call reads the xi current at its replay.  The host form stages,
 *    launches, waits and copies back; it is refused between graph_begin and graph_end.
 * One kernel family, one wave per 64-filter tile at every batch size: fbus_ekf_set_team, the policy batch, the noise table and the
 * likelihood switch do not change the route, and two calls on the same inputs are bit-identical whatever the batch size or the
 * filter's position in it.  Without an _async form.  Added under ABI 8 without a bump: detect the feature by symbol. */
#define FBUS_SAMPLE_MAX 256
int fbus_ekf_sample_dev(fbus_ekf_t h, int S, const double* xi, const uint8_t* skip, double* state, uint8_t* drawn);
int fbus_ekf_sample    (fbus_ekf_t h, int S, const double* xi, const uint8_t* skip, double* state, uint8_t* drawn);

/* ---- predicted corner pixels with their innovation covariance: the measurement model as an output ---------------------------------------
 * fbus_ekf_correct_pixels, the frame entry points and fbus_ekf_screen_markers evaluate h(x) -- map corner -> port -> image point -- and
 * its Jacobian inside their folds and never hand it out.  This call does: where the four corners of a marker of the map appear in the
 * left (and right) image given each filter's state, how uncertain that prediction is, and which corners are in view at all.  Uses: a
 * search window for the detector (the reference's front end searches the whole image and rejects detections by apparent motion,
 * C++/src/vision.cpp:825-853); pixels of a truth state for a Monte-Carlo run that stays on the device (fbus_ekf_sample -> a handle that
 * holds the truths -> this call -> fbus_ekf_correct_pixels_dev on another handle -> fbus_ekf_nees_dev); the per-corner mask behind a dof.
 *
 *   ids       [B][M] int32, M in 1..FBUS_MAX_VISIBLE, with the meaning every update gives it: -1 or an id outside the map = absent
 *   cameras   1 = left camera only, 2 = stereo.  With 1, right and cov_right are not written and may be anything, and bits 4..7 of view
 *             are 0
 *   skip      [B] bytes, nonzero = the filter produces zeros; may be NULL
 *   left, right          [B][M][8] in the handle's dtype: x0 y0 .. x3 y3 of corners.txt -- bit for bit the arrays
 *                        fbus_ekf_correct_pixels_dev takes
 *   cov_left, cov_right  [B][M][4][3] double: (S_uu, S_uv, S_vv) per corner
 *   view      [B][M] bytes: bit k is set when left corner k is in view, bit 4 + k when right corner k is
 *   Every output may be NULL, in which case it is not written.  A call with all outputs NULL is legal and launches nothing.
 *
 * For filter b, a slot whose id is in the map, camera c and corner k:
 * 1. X = M_c (R'(c_w - p) - pil) + t_c with R the record's CARRIED rotation, pil = R'(R P_IL) taken literally, c_w = P_m + R_m c_k,
 *    c_k = (0,0,0), (0,s,0), (s,s,0), (s,0,0), s = marker_size; M_c, t_c take the IMU frame into camera c's refraction frame.  This is
 *    the h of fbus_ekf_correct_pixels, not a new model.
 * 2. The corner is in view iff z_w = n.X - d_air - d_glass > 0 and |X - (n.X) n|^2 < klim z_w^2, klim = 0.81 a1^2 / (1 - a1^2),
 *    a1 = n_air / n_water: in front of the port and inside 0.9 of its field of view.  Both comparisons are false for NaN.
 * 3. uv = pi(X), the forward projection of the update at the update's precision (a closed-form start in fp32, then one Halley step of
 *    the port equation in double for fp32 records, two for fp64), rounded once to the handle's dtype when stored.
 * 4. S = H P_JJ H' + r_pix I_2 in double for both record types; H: the 2 x 6 Jacobian rows (p and theta columns) of that projection,
 *    [ -(R a)' | (a x R'(c_w - p))' ] with a' = d pi / d X M_c, in image coordinates (u, v); r_pix: the filter's own row when a noise
 *    table is set (the rule of fbus_ekf_screen_markers, item 3).
 * 5. A projection that is not in view gets 0 in its coordinates and covariance and a clear bit; so does every projection of a slot
 *    whose id is not in the map, and of a skipped filter.  Every slot is written: the caller needs no memset.
 * 6. Nothing else is written: the records stay byte-identical, and so do the applied flags, the likelihood sums, the noise table,
 *    prev_id and the carried EMA sample.
 * 7. The argument check runs before anything is staged, in this order, each but the first with the entry point's name in
 *    fbus_ekf_last_error: NULL handle (FBUS_ERR_INVALID, no text); M out of range; NULL ids; cameras not 1 or 2; (_dev) left / right /
 *    cov_left / cov_right not 16-byte aligned; r_pix <= 0; an output that overlaps the records (the rule of fbus_ekf_snapshot_dev).
 * 8. _dev: device pointers, stream-ordered, capturable.  The host form stages, launches, waits and copies back; it is refused between
 *    graph_begin and graph_end.  Without an _async form.
 * 9. One kernel family, one wave per 64-filter tile at every batch size: fbus_ekf_set_team, the policy batch, the noise table (beyond
 *    r_pix) and the likelihood switch do not change the route, and two calls on the same inputs are bit-identical whatever the batch
 *    size or the filter's position in it.
 * Added under ABI 8 without a bump: detect the feature by symbol. */
int fbus_ekf_project_markers_dev(fbus_ekf_t h, int M, const int32_t* ids, int cameras, const uint8_t* skip, void* left, void* right,
                                 double* cov_left, double* cov_right, uint8_t* view);
int fbus_ekf_project_markers    (fbus_ekf_t h, int M, const int32_t* ids, int cameras, const uint8_t* skip, void* left, void* right,
                                 double* cov_left, double* cov_right, uint8_t* view);

/* ---- L0 helpers on the device (unit-test hook) -------------------------------- */
/* Evaluates ONE of the device inline helpers the kernels are built from for n independent inputs -- what
 * matlab/quaternion_*.m, vector_to_crossmat.m, axisangle_to_quaternion.m and C++/include/matrix_math.hpp:26-99
 * compute -- so that each helper can be tested against the oracle's restatement on its own, not only through
 * predict/correct.  a, b, out: HOST arrays of the handle's scalar type, n rows each.
 *   FBUS_L0_QUAT_MUL         a (n,4) (x) b (n,4) -> out (n,4)     quaternion_add.m:22-28 / Eigen Quaterniond::operator*
 *   FBUS_L0_QUAT_TO_ROTMAT_M a (n,4)             -> out (n,9)     quaternion_to_rotmat.m:22-33
 *   FBUS_L0_QUAT_TO_ROTMAT_E a (n,4)             -> out (n,9)     Eigen toRotationMatrix (filter.cpp:542,562,564)
 *   FBUS_L0_QUAT_NORMALIZE   a (n,4)             -> out (n,4)     quaternion_normalize.m:22-24
 *   FBUS_L0_EXPM_SO3_NEG     a (n,3) = w, b (n,1) = dt -> out (n,9) = expm(-[w]x dt)   ImuUpdate.m:68 (closed form of predict_nominal)
 *   FBUS_L0_DTHETA_TO_QUAT   a (n,3) = dtheta    -> out (n,4)     axisangle_to_quaternion.m:22-29 as used by the injection (MeasureUpdate.m:94)
 *   FBUS_L0_SINCOS_HALF      a (n,1) = x         -> out (n,4) = sin x, cos x, sin x/2, cos x/2 (the polynomial / library switch) */
enum { FBUS_L0_QUAT_MUL = 0, FBUS_L0_QUAT_TO_ROTMAT_M = 1, FBUS_L0_QUAT_TO_ROTMAT_E = 2, FBUS_L0_QUAT_NORMALIZE = 3,
       FBUS_L0_EXPM_SO3_NEG = 4, FBUS_L0_DTHETA_TO_QUAT = 5, FBUS_L0_SINCOS_HALF = 6 };
int fbus_ekf_l0_eval(fbus_ekf_t h, int op, int n, const void* a, const void* b, void* out);

#ifdef __cplusplus
}
#endif
#endif /* FBUS_EKF_H */
