// ekf_launch.hpp -- host-callable launchers of every kernel of the library, and the argument types that cross from the host unit to them.
//
// The library is built from several translation units so that the kernels compile in parallel (and a kernel under
// work rebuilds in seconds): kernels_tu.hip (the predict / update / frame families) and small_tu.hip (state I/O, hypothesis groups,
// sensor updates, screening, reports) are compiled once per (scalar type, state size, family) with
// -DFBUS_TU_T / -DFBUS_TU_N / -DFBUS_TU_FAMILY and hold the explicit instantiations of the function templates
// declared here (both dialects); small_tu.hip is compiled once more for the kernels that depend on neither.  fbus_ekf.hip (handle,
// C ABI) holds no kernel and launches none: it only sees these declarations.  A type named in a launcher's signature is declared
// here, in namespace fbus: a launcher that names a type of an anonymous namespace has internal linkage and never reaches the linker.
//
// A launcher whose kernel takes a trailing parameter pack takes the same pack (`X... x`) and hands it on: one launcher and one
// kernel choice per kernel, whatever the pack.  The packs that are instantiated (each in a unit of its own, listed at the top of
// kernels_tu.hip; any other pack links as an undefined symbol):
//   launch_predict_k                                          ()  (NoiseIn)
//   launch_correct_k, launch_pixels2_k, launch_corners2_k     ()  (NisOut<T>)  (NisOut<T>, NoiseIn)  (NisOut<T>, NoiseIn, LikOut)
//   launch_frames_k, launch_frame_meas_k                      ()  (TrajOut<T>)  (TrajOut<T>, NoiseIn)
// NisOut<T>{nis, dof, thr}: nis [B] in T and dof [B] on the device (each may be null), thr: the handle's gate table on the device (null
// for the pixel / corner updates, a table of +inf for the pose update: no gate; its length was checked against the largest dof).
// NoiseIn{noise, B}: the handle's table [FBUS_NOISE_COLS][B] (fbus_ekf_set_noise).  LikOut{lik, B}: the handle's sums [4][B] (ll, rows,
// applied, rejected as doubles; fbus_ekf_loglik_enable).  TrajOut<T>{nominal, pdiag, applied}: frame f's trajectory row [f][B][.] goes
// to each non-null output.  With a pack the updates run one wave per tile.  (TrajOut<T>, NoiseIn): the resident windows of a tabled handle
// (fp32); its windows without trajectory outputs pass three null pointers, its fused single frames F = 1.
#pragma once
#include "ekf_device.hpp"
#include "vision_device.hpp"

#include <hip/hip_runtime.h>

namespace fbus {

// What the launchers need to know about the device and the process, decided ONCE per handle (fbus_ekf_create: device properties +
// environment overrides) -- nothing below reads the environment.
struct LaunchPolicy {
    int simds = 1024;               // SIMDs of the device (CUs x 4): one wave per SIMD = `simds` 64-filter tiles
    int two_wave_min_b = 1024 * 64 + 1;   // from this many filters on a launch has more waves than SIMDs: the <= 256-register forms
    bool meas_vec = true;           // measurement inputs of correct as 16-byte loads where legal
    int policy_b = 0;               // fbus_ekf_set_policy_batch: the batch the kernel-FORM choice is keyed on (0 = the launch's own B)
    // the <= 256-register forms (row-split correct, parked predict_n, frame2_kernel): chosen by the JOB's size, not the shard's, so
    // that every shard layout of one job runs the same instruction streams (the forms agree to 1 ulp only)
    bool two_wave(int B) const { return (policy_b > 0 ? policy_b : B) >= two_wave_min_b; }
};

// K == 1: the streamed per-call kernel (`policy`: 0 = nt loads and stores, 1 = default-policy loads, 2 = default loads
// and stores); K > 1: predict_n, K samples per launch with the record resident in registers
template <typename T, int N, int D, typename... X>
void launch_predict_k(hipStream_t s, T* recs, int B, int K, int policy, const T* accel, const T* gyro, const T* dt,
                      int dt_stride, const DevConst<T>& dc, const LaunchPolicy& lp, X... x);

// (with a pack fp32 never runs the row-split form)
template <typename T, int N, int D, typename... X>
void launch_correct_k(hipStream_t s, T* recs, int B, int M, const int* ids, const T* pos, const T* quat, int mode,
                      bool joseph, const unsigned char* skip, unsigned char* applied, const DevConst<T>& dc, const LaunchPolicy& lp, X... x);

template <typename T, int N, int D>
void launch_frame_k(hipStream_t s, T* recs, int B, int K, const T* accel, const T* gyro, const T* dt, int dt_stride,
                    int M, const int* ids, const T* pos, const T* quat, int mode, bool joseph,
                    const unsigned char* skip, unsigned char* applied, const DevConst<T>& dc, const LaunchPolicy& lp);
// a window of F frames in one launch (fp32; not (Joseph, nearest)); kcount: F host bytes
template <typename T, int N, int D, typename... X>
void launch_frames_k(hipStream_t s, T* recs, int B, int F, const unsigned char* kcount, const T* accel, const T* gyro,
                     const T* dt, int dt_stride, int M, const int* ids, const T* pos, const T* quat, int mode, bool joseph,
                     const unsigned char* skip, unsigned char* applied, const DevConst<T>& dc, X... x);

// ---- team kernels (ekf_team.hpp): several waves per 64-filter tile, fp32 only -------------------------------------------
// roles: waves per tile (predict 2..4, predict_n always 4); policy as in launch_predict_k
template <typename T, int N, int D>
void launch_predict_team_k(hipStream_t s, T* recs, int B, int K, int roles, int policy, const T* accel, const T* gyro,
                           const T* dt, int dt_stride, const DevConst<T>& dc);
template <typename T, int N, int D>
void launch_frames_team_k(hipStream_t s, T* recs, int B, int F, const unsigned char* kcount, const T* accel, const T* gyro,
                          const T* dt, int dt_stride, int M, const int* ids, const T* pos, const T* quat, int mode,
                          const unsigned char* skip, unsigned char* applied, const DevConst<T>& dc);

// ---- correct() from corner pixels, round-4 kernel (ekf_meas.hpp) ---------------------------------------------------------
constexpr int MKC_STRIDE = 10;      // doubles per map slot: corner 0 in the world (3), marker x axis (3), y axis (3), pad

// constants of the pixel fold (double; kernel argument)
struct MeasConst {
    double P_IL[3];
    double McL[9], McR[9], tR[3];   // a corner at t_I (IMU frame, t_I = R'(c_w - p) - P_IL) in the refraction frame of the left / right
                                    // camera:  XL = McL t_I,  XR = McR t_I + tR   (McL = F R_IL: vision.cpp:597-599 undone;
                                    // McR = R_RL^-1 McL, tR = -R_RL^-1 P_LR: vision.cpp:555-556 inverted)
    double nML[3], nMR[3];          // n' McL, n' McR
    double NI[6];                   // R_IL' R_IL (symmetric: 00 01 02 11 12 22): the N' of a corner's three position rows
    double n[3];                    // port normal
    double a0, a1, d_air, d_glass;  // n_air / n_glass, n_air / n_water
    double klim;                    // (round 6) (0.9 a1)^2 / (1 - a1^2): the field-of-view test of the fold (a division per marker when left to the kernel)
    double MiTL[9], adjL[9];        // (round 6) McL^-T and adj(McL) = det(McL) McL^-1: the camera-frame fold of the left-only kernels
                                    // (ekf_meas.hpp::pixel_fold_marker<..., CF = true>, PixAcc::to_imu_frame)
    float st[8];                    // (round 6) constants of the fp32 start of the port equation (ekf_meas.hpp::port_start_f32):
                                    // a1, a1^2, 1 - a1^2, 1 - a0^2, d_air, d_glass a0, (d_air + d_glass a0) / a1, 0
    const double* mkc;              // [FBUS_MAX_MARKERS][MKC_STRIDE]
};
// roles: waves per 64-filter tile (1, 2 or 4: the markers of a filter divided among them; with a pack always 1); right == nullptr: left
// camera only; r_pix: ignored with a NoiseIn.
// The kernel does not depend on the dialect (the pixel rows have no quaternion part); D only keeps the instantiation macro uniform.
template <typename T, int N, int D, typename... X>
void launch_pixels2_k(hipStream_t s, T* recs, int B, int M, const int* ids, const T* left, const T* right, int roles, double size,
                      double r_pix, const unsigned char* skip, unsigned char* applied, const short* id2slot, const MeasConst& mc, X... x);
// (round 5) the same update with the TAIL divided between the waves of a tile (ekf_meas_split.hpp): roles = 2 or 4 waves per tile
// (launches below half / a quarter of the chip's SIMDs in tiles).  fp32 records, square port only -- the caller checks.
template <typename T, int N, int D>
void launch_pixels_split_k(hipStream_t s, T* recs, int B, int M, const int* ids, const T* left, const T* right, int roles, double size,
                           double r_pix, const unsigned char* skip, unsigned char* applied, const short* id2slot, const MeasConst& mc);
// correct() from stereo corners, round-4 kernel: nearest marker (roles forced to 1) or stacked; dialect: hysteresis of the nearest mode;
// roles and r_pos as launch_pixels2_k's roles and r_pix
template <typename T, int N, int D, typename... X>
void launch_corners2_k(hipStream_t s, T* recs, int B, int M, const int* ids, const T* left, const T* right, int geometry, int mode,
                       int roles, double size, double r_pos, double switch_thres, const unsigned char* skip, unsigned char* applied,
                       const short* id2slot, const MeasConst& mc, const VisConst<double>& vc, const VisConst<T>& vct, X... x);

// ---- one camera frame with the north star's MeasureUpdate in one launch (ekf_meas.hpp::frame_meas_kernel; fp32) -----------------
// kind: corner pixels (geometry / mode ignored; right == nullptr: left camera) or stereo corners (geometry, mode as correct_corners)
enum { MEAS_PIXELS = 0, MEAS_CORNERS = 1 };
// F = 1: one frame of kcount[0] predicts; F > 1: a window of F frames in one launch (kcount: F host bytes; measurements [F][B][M]...);
// with a pack the window form only (F = 1 included); with a NoiseIn qd and r_meas are ignored
template <typename T, int N, int D, typename... X>
void launch_frame_meas_k(hipStream_t s, T* recs, int B, int F, const unsigned char* kcount, const T* accel, const T* gyro, const T* dt, int dt_stride, int kind,
                         int M, const int* ids, const T* left, const T* right, int geometry, int mode, double size, double r_meas,
                         double switch_thres, const unsigned char* skip, unsigned char* applied, const short* id2slot,
                         const MeasConst& mc, const VisConst<double>& vc, const VisConst<T>& vct, const T* qd, X... x);

// ---- record I/O and initialisation (ekf_kernels.hpp; family "state") -----------------------------------------------------------------------
// one wave per 64-filter tile (pack, unpack, snapshot, reset_cov) / one thread per filter (the two initialisations)
template <typename T, int N>
void launch_pack_k(hipStream_t s, T* recs, int B, const T* nominal, const T* rot, const T* P, const int* prev);
template <typename T, int N>
void launch_unpack_k(hipStream_t s, const T* recs, int B, T* nominal, T* rot, T* P, int* prev);
// p0: the six variances of fbus_params::p0_diag
template <typename T, int N>
void launch_reset_cov_k(hipStream_t s, T* recs, int B, const double* p0);
template <typename T, int N>
void launch_snapshot_k(hipStream_t s, const T* recs, int B, const unsigned char* d_applied, T* nominal, T* pdiag, unsigned char* applied);
template <typename T, int N>
void launch_init_gravity_bias_k(hipStream_t s, T* recs, int B, int Tn, const T* accel, const T* gyro);
template <typename T, int N, int D>
void launch_pose_init_k(hipStream_t s, T* recs, int B, int M, const int* ids, const T* pos, const T* quat, int what, double max_dist,
                        const unsigned char* mask, T* out7, unsigned char* applied, const DevConst<T>& dc);

// ---- hypothesis groups (ekf_group.hpp; family "group"): one wave per floor(64 / G) whole groups ---------------------------------------------
// P == nullptr: the diagonal alone (the kernel without the dense covariance)
template <typename T, int N>
void launch_group_fuse_k(hipStream_t s, const T* recs, size_t rec_bytes, int B, int G, const double* logw, double* weight, int* best,
                         T* nominal, T* P, T* pdiag);
template <typename T, int N>
void launch_group_collapse_k(hipStream_t s, T* recs, size_t rec_bytes, int B, int G, const int* src);
template <typename T, int N>
void launch_group_mix_k(hipStream_t s, T* recs, size_t rec_bytes, int B, int G, const double* logw, const double* trans, double* weight,
                        double* logc);

// ---- the streamed sensor updates (ekf_depth.hpp, ekf_velocity.hpp, ekf_rows.hpp; family "sensor"): one wave per tile ------------------------
// the depth sensor, by value (fbus_ekf_set_depth_sensor): unit axis, reading at the world origin, lever arm in the IMU frame
struct DepthSensor { double axis[3], offset, lever[3]; };
// the velocity sensor, by value (fbus_ekf_set_velocity_sensor): the rotation IMU frame -> instrument frame (row-major), the instrument's
// position in the IMU frame
struct VelocitySensor { double C[9], lever[3]; };
// thr: the gate table; nis, dof, lik: each may be null
template <typename T, int N>
void launch_depth_k(hipStream_t s, T* recs, int B, const T* z, const double* var, int var_stride, const unsigned char* skip,
                    unsigned char* applied, const DepthSensor& ds, const double* thr, T* nis, int* dof, double* lik);
template <typename T, int N>
void launch_velocity_k(hipStream_t s, T* recs, int B, const T* z, const T* gyro, const double* var, int var_stride,
                       const unsigned char* skip, unsigned char* applied, const VelocitySensor& vs, const double* thr, T* nis, int* dof,
                       double* lik);
// m = 1..3 rows per filter: picks the instantiation
template <typename T, int N>
void launch_rows_k(hipStream_t s, T* recs, int B, int m, const T* res, const T* H, const double* var, int var_stride,
                   const unsigned char* skip, unsigned char* applied, const double* thr, T* nis, int* dof, double* lik);

// ---- per-marker screening (ekf_screen.hpp; family "screen"): one wave per tile -------------------------------------------------------------
enum { SCREEN_PIX_LEFT = 0, SCREEN_PIX_STEREO = 1, SCREEN_CORNERS = 2 };
// where the verdicts go: ids_out [B][M], nis [B][M] in T, dof [B][M], kept [B]; each may be null.  thr: the handle's gate table
template <typename T> struct ScreenOut { int* ids; T* nis; int* dof; int* kept; const double* thr; };
template <typename T, int N, int KIND>
void launch_screen_meas_k(hipStream_t st, const T* recs, int B, int M, const int* ids, const T* a, const T* bb, int geometry, bool square_port,
                          double size, double r_meas, const double* noise, const unsigned char* skip, const short* id2slot,
                          const MeasConst& mc, const VisConst<double>& vc, const VisConst<T>& vct, const ScreenOut<T>& out);
template <typename T, int N, int DIALECT>
void launch_screen_pose_k(hipStream_t st, const T* recs, int B, int M, const int* ids, const T* pos, const T* quat, const double* noise,
                          const unsigned char* skip, const DevConst<T>& dc, const ScreenOut<T>& out);

// ---- predicted corner pixels (ekf_project.hpp; family "screen"): one wave per tile ----------------------------------------------------------
// left, right [B][M][8] in T, cov_left, cov_right [B][M][4][3], view [B][M]; each may be null (CAM = 1: right and cov_right are not read)
template <typename T> struct ProjectOut { T* left; T* right; double* cov_left; double* cov_right; unsigned char* view; };
// CAM: 1 = left camera, 2 = stereo; r_pix: ignored with a noise table
template <typename T, int N, int CAM>
void launch_project_k(hipStream_t st, const T* recs, int B, int M, const int* ids, bool square_port, double size, double r_pix,
                      const double* noise, const unsigned char* skip, const short* id2slot, const MeasConst& mc, const ProjectOut<T>& out);

// ---- NEES and draws (ekf_nees.hpp, ekf_sample.hpp; family "report"): one wave per tile ------------------------------------------------------
struct NeesOut { double* nees; double* err; double* lnp; };     // [B][FBUS_NEES_COLS], [B][N], [B]; each may be null
struct SampleOut { double* state; unsigned char* drawn; };      // [S][B][19], [B]; each may be null
template <typename T, int N>
void launch_nees_k(hipStream_t st, const T* recs, int B, const double* truth, const unsigned char* skip, const NeesOut& out);
template <typename T, int N>
void launch_sample_k(hipStream_t st, const T* recs, int B, int S, const double* xi, const unsigned char* skip, const SampleOut& out);

// ---- the kernels that depend on neither the state size nor the dialect (small_tu.hip, built once; unit "common") -----------------------------
template <typename T>
void launch_marker_pose_k(hipStream_t s, int n, int geometry, const T* left, const T* right, T* pos, T* quat, T* corners3d,
                          const VisConst<double>& vc);
template <typename T>
void launch_imu_ema_k(hipStream_t s, int B, int Tn, T* accel, T* gyro, T* carry, int have_carry);
template <typename T>
void launch_l0_eval_k(hipStream_t s, int op, int n, const T* a, const T* b, T* out);
// B x FBUS_NOISE_COLS row-major -> fields [FBUS_NOISE_COLS][B] (fbus_ekf_set_noise_dev)
void launch_noise_fields_k(hipStream_t s, const double* rows, double* fields, int B);
// one row (q_v, q_theta, q_ba, q_bg, r_pos, r_quat, r_pix) into every filter's fields
void launch_noise_own_row_k(hipStream_t s, double* fields, int B, const double* row);
// the sums [4][B] as doubles -> the caller's typed arrays (fbus_ekf_loglik_get*; each may be null)
void launch_lik_export_k(hipStream_t s, const double* acc, int B, double* ll, int64_t* rows, int32_t* applied, int32_t* rejected);

}  // namespace fbus
