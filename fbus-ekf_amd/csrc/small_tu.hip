// small_tu.hip -- the small kernel families, each for one (scalar type, state size), and the kernels that depend on neither.
// Compiled once per (type, N, family) row of build.py's FAMILIES table with -DFBUS_TU_T=float|double  -DFBUS_TU_N=18|15  -DFBUS_TU_FAMILY=n,
// with build.py's base flags alone (no per-family scheduler flag), fp32 and fp64 records alike:
//  21 state   pack, unpack, reset_cov, snapshot, init_gravity_bias, pose_init (ekf_kernels.hpp)
//  22 group   hypothesis groups: fuse, collapse, mix (ekf_group.hpp)
//  23 sensor  the streamed sensor updates: depth, velocity, rows, and the steps they share (ekf_depth.hpp, ekf_velocity.hpp, ekf_rows.hpp
//             over ekf_sensor.hpp)
//  24 screen  per-marker screening: pixel / corner rows and pose rows (ekf_screen.hpp); predicted corner pixels with their innovation
//             covariance (ekf_project.hpp)
//  25 report  NEES against a truth state and draws from every filter's Gaussian: one record stream and one column step (ekf_nees.hpp,
//             ekf_sample.hpp)
// and once with -DFBUS_TU_FAMILY=26 alone (unit "common"):
//  26 common  marker_pose, imu_ema, l0_eval for float and double (ekf_kernels.hpp); the noise-table and likelihood-export helpers (below)
// Each family includes the headers of its kernels and no other: a kernel header is included by exactly one family.  A launcher is written
// next to its kernel, in namespace fbus, and declared in ekf_launch.hpp; this file holds the explicit instantiations.  gfx950 only.
#if !defined(FBUS_TU_FAMILY) || (FBUS_TU_FAMILY != 26 && (!defined(FBUS_TU_T) || !defined(FBUS_TU_N)))
#error "small_tu.hip: define FBUS_TU_FAMILY, and FBUS_TU_T and FBUS_TU_N for every family but 26 (see build.py)"
#endif

#if FBUS_TU_FAMILY == 21 || FBUS_TU_FAMILY == 26
#include "ekf_kernels.hpp"
#elif FBUS_TU_FAMILY == 22
#include "ekf_group.hpp"
#elif FBUS_TU_FAMILY == 23
#include "ekf_depth.hpp"
#include "ekf_velocity.hpp"
#include "ekf_rows.hpp"
#elif FBUS_TU_FAMILY == 24
#include "ekf_project.hpp"
#include "ekf_screen.hpp"
#elif FBUS_TU_FAMILY == 25
#include "ekf_sample.hpp"
#else
#error "FBUS_TU_FAMILY must be one of the families listed at the top of this file"
#endif
#include "ekf_launch.hpp"

// the launcher's own type, as ekf_launch.hpp declares it, names the instantiation
#define FBUS_INST(...) template decltype(__VA_ARGS__) __VA_ARGS__;
#define FBUS_TN FBUS_TU_T, FBUS_TU_N

#if FBUS_TU_FAMILY == 26
namespace {

// B x FBUS_NOISE_COLS row-major -> fields [FBUS_NOISE_COLS][B] (fbus_ekf_set_noise_dev; one thread per entry, reads coalesced)
__global__ void noise_fields_kernel(const double* __restrict__ rows, double* __restrict__ fields, int B)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * FBUS_NOISE_COLS) return;
    const size_t b = i / FBUS_NOISE_COLS, c = i % FBUS_NOISE_COLS;
    fields[c * (size_t)B + b] = rows[i];
}
// fbus_params' own row into every filter's table fields: what the likelihood kernels (always the tabled kind) read while the caller has
// set no table
__global__ void noise_own_row_kernel(double* __restrict__ fields, int B, double q0, double q1, double q2, double q3, double r_pos,
                                     double r_quat, double r_pix)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * FBUS_NOISE_COLS) return;
    const int c = (int)(i / (size_t)B);
    fields[i] = c == 0 ? q0 : c == 1 ? q1 : c == 2 ? q2 : c == 3 ? q3 : c == 4 ? r_pos : c == 5 ? r_quat : r_pix;
}
// the sums [4][B] as doubles -> the caller's typed arrays (fbus_ekf_loglik_get*; each may be null)
__global__ void lik_export_kernel(const double* __restrict__ acc, int B, double* __restrict__ ll, int64_t* __restrict__ rows,
                                  int32_t* __restrict__ applied, int32_t* __restrict__ rejected)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (ll) ll[b] = acc[b];
    if (rows) rows[b] = (int64_t)acc[(size_t)B + b];
    if (applied) applied[b] = (int32_t)acc[2 * (size_t)B + b];
    if (rejected) rejected[b] = (int32_t)acc[3 * (size_t)B + b];
}

}  // namespace
#endif

namespace fbus {

#if FBUS_TU_FAMILY == 21
FBUS_INST(launch_pack_k<FBUS_TN>)
FBUS_INST(launch_unpack_k<FBUS_TN>)
FBUS_INST(launch_reset_cov_k<FBUS_TN>)
FBUS_INST(launch_snapshot_k<FBUS_TN>)
FBUS_INST(launch_init_gravity_bias_k<FBUS_TN>)
FBUS_INST(launch_pose_init_k<FBUS_TN, DIALECT_MATLAB>)
FBUS_INST(launch_pose_init_k<FBUS_TN, DIALECT_CPP>)
#elif FBUS_TU_FAMILY == 22
FBUS_INST(launch_group_fuse_k<FBUS_TN>)
FBUS_INST(launch_group_collapse_k<FBUS_TN>)
FBUS_INST(launch_group_mix_k<FBUS_TN>)
#elif FBUS_TU_FAMILY == 23
FBUS_INST(launch_depth_k<FBUS_TN>)
FBUS_INST(launch_velocity_k<FBUS_TN>)
FBUS_INST(launch_rows_k<FBUS_TN>)
#elif FBUS_TU_FAMILY == 24
FBUS_INST(launch_screen_meas_k<FBUS_TN, SCREEN_PIX_LEFT>)
FBUS_INST(launch_screen_meas_k<FBUS_TN, SCREEN_PIX_STEREO>)
FBUS_INST(launch_screen_meas_k<FBUS_TN, SCREEN_CORNERS>)
FBUS_INST(launch_screen_pose_k<FBUS_TN, DIALECT_MATLAB>)
FBUS_INST(launch_screen_pose_k<FBUS_TN, DIALECT_CPP>)
FBUS_INST(launch_project_k<FBUS_TN, 1>)
FBUS_INST(launch_project_k<FBUS_TN, 2>)
#elif FBUS_TU_FAMILY == 25
FBUS_INST(launch_nees_k<FBUS_TN>)
FBUS_INST(launch_sample_k<FBUS_TN>)
#else
FBUS_INST(launch_marker_pose_k<float>)
FBUS_INST(launch_marker_pose_k<double>)
FBUS_INST(launch_imu_ema_k<float>)
FBUS_INST(launch_imu_ema_k<double>)
FBUS_INST(launch_l0_eval_k<float>)
FBUS_INST(launch_l0_eval_k<double>)

void launch_noise_fields_k(hipStream_t s, const double* rows, double* fields, int B)
{
    const size_t n = (size_t)FBUS_NOISE_COLS * B;
    hipLaunchKernelGGL(noise_fields_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, fields, B);
}
void launch_noise_own_row_k(hipStream_t s, double* fields, int B, const double* row)
{
    const size_t n = (size_t)FBUS_NOISE_COLS * B;
    hipLaunchKernelGGL(noise_own_row_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fields, B, row[0], row[1], row[2], row[3],
                       row[4], row[5], row[6]);
}
void launch_lik_export_k(hipStream_t s, const double* acc, int B, double* ll, int64_t* rows, int32_t* applied, int32_t* rejected)
{
    hipLaunchKernelGGL(lik_export_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, acc, B, ll, rows, applied, rejected);
}
#endif

}  // namespace fbus
