// batched_filter.hpp -- header-only C++ host class over the C ABI (include/fbus_ekf.h).
//
// fbus::BatchedFilter is the batched, device-resident counterpart of the reference's
// FBUSEKF::FILTER (C++/include/filter.hpp:60-230): it owns the state of B filters and
// exposes the two steps of the hot path under the names BASELINE.json asks for:
//
//   predict(accel, gyro, dt)          == FILTER::UpdateCovariance + UpdateNominalState
//                                        (C++/src/filter.cpp:588-616, 533-582) / ImuUpdate.m:36
//   correct(M, ids, pos, quat, mode)  == FILTER::ObservationUpdate (filter.cpp:622-754) / MeasureUpdate.m:37
//
// plus the reference's input conventions: IMUData-style samples (common.hpp:176-193) and
// DetectionResult-style marker poses (filter.hpp:39-57).  Errors are C++ exceptions carrying the
// library's message; the reference's "silent early return" cases stay silent (query applied()).
#pragma once
#include "../fbus_ekf.h"

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace fbus {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

template <typename Real = float>
class BatchedFilter {
    static_assert(sizeof(Real) == 4 || sizeof(Real) == 8, "Real must be float or double");

public:
    enum class Mode { Nearest = FBUS_MODE_NEAREST, Stacked = FBUS_MODE_STACKED };

    BatchedFilter(int batch, const fbus_params& prm, int device = 0, int nstate = 18)
        : batch_(batch), nstate_(nstate)
    {
        check(fbus_ekf_create(&h_, &prm, batch, device, int(sizeof(Real)) * 8, nstate), "fbus_ekf_create");
    }
    explicit BatchedFilter(int batch, int dialect = FBUS_DIALECT_CPP, int device = 0, int nstate = 18)
        : BatchedFilter(batch, defaults(dialect), device, nstate) {}
    ~BatchedFilter() { fbus_ekf_destroy(h_); }
    BatchedFilter(const BatchedFilter&) = delete;
    BatchedFilter& operator=(const BatchedFilter&) = delete;

    static fbus_params defaults(int dialect)
    {
        fbus_params p;
        if (fbus_params_default(&p, dialect) != FBUS_OK) throw Error(FBUS_ERR_INVALID, "fbus_params_default");
        return p;
    }

    int batch() const { return batch_; }
    int nstate() const { return nstate_; }
    fbus_ekf_t handle() const { return h_; }

    // ---- state (host vectors; B x 19, B x 9, B x N x N, B) -------------------------------------
    void set_state(const Real* nominal, const Real* rot, const Real* P, const int32_t* prev_id = nullptr)
    { check(fbus_ekf_set_state(h_, nominal, rot, P, prev_id), "set_state"); }
    void get_state(Real* nominal, Real* rot, Real* P, int32_t* prev_id = nullptr) const
    { check(fbus_ekf_get_state(h_, nominal, rot, P, prev_id), "get_state"); }
    void reset_covariance() { check(fbus_ekf_reset_cov(h_), "reset_cov"); }

    // ---- hot path, host pointers (staged) ---------------------------------------------------------
    void predict(const Real* accel, const Real* gyro, Real dt)
    { check(fbus_ekf_predict(h_, accel, gyro, &dt, 0), "predict"); }
    void predict(const Real* accel, const Real* gyro, const Real* dt_per_filter)
    { check(fbus_ekf_predict(h_, accel, gyro, dt_per_filter, 1), "predict"); }
    void correct(int M, const int32_t* ids, const Real* pos, const Real* quat, Mode mode = Mode::Nearest,
                 const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct(h_, M, ids, pos, quat, int(mode), skip), "correct"); }

    // ---- (round 6) the same host-pointer calls without the wait: arrays taken by value (pageable: copied into a pinned ring of the
    //      handle's on return; pinned: in place, unchanged until inputs_consumed() / sync()), nothing waits for the device -- one call
    //      per IMU sample as FILTER::SetImuData / BatchImuProcessing issue them (filter.cpp:24-55,505-516)
    void predict_async(const Real* accel, const Real* gyro, Real dt)
    { check(fbus_ekf_predict_async(h_, accel, gyro, &dt, 0), "predict_async"); }
    void predict_n_async(int K, const Real* accel, const Real* gyro, const Real* dt, bool dt_per_filter = false)
    { check(fbus_ekf_predict_n_async(h_, K, accel, gyro, dt, dt_per_filter), "predict_n_async"); }
    void correct_async(int M, const int32_t* ids, const Real* pos, const Real* quat, Mode mode = Mode::Nearest,
                       const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_async(h_, M, ids, pos, quat, int(mode), skip), "correct_async"); }
    void correct_pixels_async(int M, const int32_t* ids, const Real* left, const Real* right = nullptr, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_pixels_async(h_, M, ids, left, right, skip), "correct_pixels_async"); }
    void inputs_consumed() { check(fbus_ekf_async_inputs_consumed(h_), "async_inputs_consumed"); }

    // ---- hot path, device pointers (no copies, asynchronous until sync()) ----------------------------
    void predict_dev(const Real* accel, const Real* gyro, const Real* dt, bool dt_per_filter = false)
    { check(fbus_ekf_predict_dev(h_, accel, gyro, dt, dt_per_filter), "predict_dev"); }
    void predict_n_dev(int K, const Real* accel, const Real* gyro, const Real* dt, bool dt_per_filter = false)
    { check(fbus_ekf_predict_n_dev(h_, K, accel, gyro, dt, dt_per_filter), "predict_n_dev"); }
    void correct_dev(int M, const int32_t* ids, const Real* pos, const Real* quat, Mode mode = Mode::Nearest,
                     const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_dev(h_, M, ids, pos, quat, int(mode), skip), "correct_dev"); }
    // one camera frame: K per-sample predicts then one correct (filter.cpp:232-235)
    void frame_dev(int K, const Real* accel, const Real* gyro, const Real* dt, int M, const int32_t* ids,
                   const Real* pos, const Real* quat, Mode mode = Mode::Nearest)
    { check(fbus_ekf_frame_dev(h_, K, accel, gyro, dt, 0, M, ids, pos, quat, int(mode), nullptr), "frame_dev"); }

    // the same frame in one launch, and a window of frames in one launch (records resident in registers; offline replay)
    void frame_fused_dev(int K, const Real* accel, const Real* gyro, const Real* dt, int M, const int32_t* ids,
                         const Real* pos, const Real* quat, Mode mode = Mode::Nearest)
    { check(fbus_ekf_frame_fused_dev(h_, K, accel, gyro, dt, 0, M, ids, pos, quat, int(mode), nullptr), "frame_fused_dev"); }
    void frames_fused_dev(const std::vector<int32_t>& kcount, const Real* accel, const Real* gyro, const Real* dt, int M,
                          const int32_t* ids, const Real* pos, const Real* quat, Mode mode = Mode::Nearest,
                          const uint8_t* skip = nullptr)
    {
        check(fbus_ekf_frames_fused_dev(h_, int(kcount.size()), kcount.data(), accel, gyro, dt, 0, M, ids, pos, quat, int(mode), skip),
              "frames_fused_dev");
    }
    // the same window with its trajectory (fbus_ekf_frames_fused_traj_dev): device outputs [F][B][19], [F][B][N], [F][B], each may be null
    void frames_fused_dev(const std::vector<int32_t>& kcount, const Real* accel, const Real* gyro, const Real* dt, int M,
                          const int32_t* ids, const Real* pos, const Real* quat, Mode mode, const uint8_t* skip,
                          Real* out_nominal, Real* out_pdiag, uint8_t* out_applied)
    {
        check(fbus_ekf_frames_fused_traj_dev(h_, int(kcount.size()), kcount.data(), accel, gyro, dt, 0, M, ids, pos, quat, int(mode), skip,
                                             out_nominal, out_pdiag, out_applied), "frames_fused_traj_dev");
    }
    // nominal (B, 19), diag(P) (B, N), applied (B) of the current records into device buffers (fbus_ekf_snapshot_dev; each may be null)
    void snapshot_dev(Real* nominal, Real* pdiag, uint8_t* applied) { check(fbus_ekf_snapshot_dev(h_, nominal, pdiag, applied), "snapshot_dev"); }

    // correct() from corner pixels (north-star extension): left / right (B, M, 8) normalised image points, right may be null
    void correct_pixels(int M, const int32_t* ids, const Real* left, const Real* right = nullptr, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_pixels(h_, M, ids, left, right, skip), "correct_pixels"); }

    // correct() from stereo corners (north-star extension): left / right (B, M, 8) normalised image points, or left = (B, M, 12)
    // triangulated corners with geometry = FBUS_VIS_CORNERS3D; the triangulation of vision.cpp:472-618 runs on the device
    void correct_corners(int M, const int32_t* ids, const Real* left, const Real* right, int geometry, Mode mode = Mode::Nearest,
                         const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_corners(h_, M, ids, left, right, geometry, int(mode), skip), "correct_corners"); }

    // NIS and gating of correct() and the two updates above (include/fbus_ekf.h): the gate table indexed by dof (empty: no gate), then the
    // updates writing nis (B values) and dof (B int32) per filter, each may be null -- host arrays here, device arrays for _nis_dev
    void set_gate(const std::vector<double>& thresholds)
    { check(fbus_ekf_set_gate(h_, int(thresholds.size()), thresholds.empty() ? nullptr : thresholds.data()), "set_gate"); }
    void correct(int M, const int32_t* ids, const Real* pos, const Real* quat, Mode mode, const uint8_t* skip, Real* nis, int32_t* dof)
    { check(fbus_ekf_correct_nis(h_, M, ids, pos, quat, int(mode), skip, nis, dof), "correct_nis"); }
    void correct_nis_dev(int M, const int32_t* ids, const Real* pos, const Real* quat, Mode mode, const uint8_t* skip, Real* nis,
                         int32_t* dof)
    { check(fbus_ekf_correct_nis_dev(h_, M, ids, pos, quat, int(mode), skip, nis, dof), "correct_nis_dev"); }
    void correct_pixels(int M, const int32_t* ids, const Real* left, const Real* right, const uint8_t* skip, Real* nis, int32_t* dof)
    { check(fbus_ekf_correct_pixels_nis(h_, M, ids, left, right, skip, nis, dof), "correct_pixels_nis"); }
    void correct_pixels_nis_dev(int M, const int32_t* ids, const Real* left, const Real* right, const uint8_t* skip, Real* nis, int32_t* dof)
    { check(fbus_ekf_correct_pixels_nis_dev(h_, M, ids, left, right, skip, nis, dof), "correct_pixels_nis_dev"); }
    void correct_corners(int M, const int32_t* ids, const Real* left, const Real* right, int geometry, Mode mode, const uint8_t* skip,
                         Real* nis, int32_t* dof)
    { check(fbus_ekf_correct_corners_nis(h_, M, ids, left, right, geometry, int(mode), skip, nis, dof), "correct_corners_nis"); }
    void correct_corners_nis_dev(int M, const int32_t* ids, const Real* left, const Real* right, int geometry, Mode mode,
                                 const uint8_t* skip, Real* nis, int32_t* dof)
    { check(fbus_ekf_correct_corners_nis_dev(h_, M, ids, left, right, geometry, int(mode), skip, nis, dof), "correct_corners_nis_dev"); }

    // per-filter noise (include/fbus_ekf.h): a batch() x FBUS_NOISE_COLS table, row-major, columns q_v q_theta q_ba q_bg r_pos r_quat r_pix;
    // an empty table: none (back to fbus_params).  set_noise_dev: a device table, stream-ordered, not inspected
    void set_noise(const std::vector<double>& table)
    {
        if (!table.empty() && table.size() != size_t(batch_) * FBUS_NOISE_COLS)
            throw std::invalid_argument("fbus::BatchedFilter::set_noise: expected batch() x FBUS_NOISE_COLS entries");
        check(fbus_ekf_set_noise(h_, table.empty() ? nullptr : table.data()), "set_noise");
    }
    void set_noise_dev(const double* table) { check(fbus_ekf_set_noise_dev(h_, table), "set_noise_dev"); }
    std::vector<double> get_noise() const
    {
        std::vector<double> t(size_t(batch_) * FBUS_NOISE_COLS);
        check(fbus_ekf_get_noise(h_, t.data()), "get_noise");
        return t;
    }

    // per-filter innovation log-likelihood sums (include/fbus_ekf.h): every measurement update adds ll = -1/2 (nis + log det S + rows ln 2 pi)
    // while accumulation is on (the one-wave routes, as with a noise table); the sums of a run rank noise hypotheses
    struct LogLik { std::vector<double> ll; std::vector<int64_t> rows; std::vector<int32_t> applied, rejected; };
    void loglik_enable(bool on = true) { check(fbus_ekf_loglik_enable(h_, on ? 1 : 0), "loglik_enable"); }
    void loglik_reset() { check(fbus_ekf_loglik_reset(h_), "loglik_reset"); }
    LogLik loglik() const
    {
        LogLik s;
        s.ll.resize(batch_); s.rows.resize(batch_); s.applied.resize(batch_); s.rejected.resize(batch_);
        check(fbus_ekf_loglik_get(h_, s.ll.data(), s.rows.data(), s.applied.data(), s.rejected.data()), "loglik_get");
        return s;
    }
    // ... into device arrays of batch() entries, stream-ordered; each may be null
    void loglik_dev(double* ll, int64_t* rows, int32_t* applied, int32_t* rejected) const
    { check(fbus_ekf_loglik_get_dev(h_, ll, rows, applied, rejected), "loglik_get_dev"); }

    // hypothesis groups (include/fbus_ekf.h): contiguous groups of G filters, 2 <= G <= FBUS_GROUP_MAX, batch() % G == 0.  Device
    // pointers, stream-ordered.  group_fuse_dev: logw (batch(); null = the likelihood sums) -> weight (batch()), best (batch() / G),
    // and the moment-matched nominal (batch() / G, 19), P (batch() / G, N, N), pdiag (batch() / G, N); each output may be null.
    // group_collapse_dev: every member of group j becomes its member src[j], bit for bit; src[j] outside 0..G-1 skips the group
    void group_fuse_dev(int G, const double* logw, double* weight, int32_t* best, Real* nominal, Real* P, Real* pdiag) const
    { check(fbus_ekf_group_fuse_dev(h_, G, logw, weight, best, nominal, P, pdiag), "group_fuse_dev"); }
    void group_collapse_dev(int G, const int32_t* src) { check(fbus_ekf_group_collapse_dev(h_, G, src), "group_collapse_dev"); }
    // group_mix_dev: the IMM mixing step in place -- every member re-initialised from the mixture of its group's members under the
    // model-transition matrix trans (G x G row-major, trans[i][j] = the probability that model i is followed by model j; uninspected)
    // -> weight (batch(): mu), logc (batch(): log of the predicted model probability; + the next stretch's ll = the next logw); each
    // output may be null.  The cycle: logw = logc + ll, group_fuse_dev (the output estimate), group_mix_dev, loglik_reset, frames.
    void group_mix_dev(int G, const double* logw, const double* trans, double* weight, double* logc)
    { check(fbus_ekf_group_mix_dev(h_, G, logw, trans, weight, logc), "group_mix_dev"); }

    // ---- the depth (pressure) sensor update (fbus_ekf.h; the reference names the sensor, common.hpp:16, and has no update for it).
    // One scalar row per filter, h = axis . (p + R lever) + offset; at the sensor's own rate, between camera frames:
    //   loop { predict_n(imu since the last reading); correct_depth(z, var); }
    // set_depth_sensor first (axis: world frame, normalised by the library; lever: IMU frame, null = 0).  z: batch() readings; var: ONE
    // variance or (per_filter) batch() of them, always double; a skipped filter, a non-finite z and a var that is not finite and > 0
    // leave the filter untouched; otherwise the update is applied iff S > 0 and nis <= thr[1] of set_gate's table (both false for a
    // NaN), in every form.  nis / dof: batch() each, either may be null.
    void set_depth_sensor(const double axis[3], double offset = 0.0, const double* lever = nullptr)
    { check(fbus_ekf_set_depth_sensor(h_, axis, offset, lever), "fbus_ekf_set_depth_sensor"); }
    void correct_depth(const Real* z, double var, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_depth(h_, z, &var, 0, skip), "correct_depth"); }
    void correct_depth(const Real* z, const double* var, bool per_filter, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_depth(h_, z, var, per_filter ? 1 : 0, skip), "correct_depth"); }
    void correct_depth_dev(const Real* z, const double* var, bool per_filter, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_depth_dev(h_, z, var, per_filter ? 1 : 0, skip), "correct_depth_dev"); }
    void correct_depth_async(const Real* z, const double* var, bool per_filter, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_depth_async(h_, z, var, per_filter ? 1 : 0, skip), "correct_depth_async"); }
    void correct_depth_nis(const Real* z, const double* var, bool per_filter, const uint8_t* skip, Real* nis, int32_t* dof)
    { check(fbus_ekf_correct_depth_nis(h_, z, var, per_filter ? 1 : 0, skip, nis, dof), "correct_depth_nis"); }
    void correct_depth_nis_dev(const Real* z, const double* var, bool per_filter, const uint8_t* skip, Real* nis, int32_t* dof)
    { check(fbus_ekf_correct_depth_nis_dev(h_, z, var, per_filter ? 1 : 0, skip, nis, dof), "correct_depth_nis_dev"); }

    // ---- per-marker chi-square screening (fbus_ekf.h; in the place of VISION::RejectInvalidMarker, vision.cpp:825-853): every marker slot
    // judged alone against the prior, nis_m <= thr[dof_m] of set_gate's table or its id becomes -1 in ids_out.  kind: FBUS_SCREEN_POSE
    // (a, b = pos, quat), FBUS_SCREEN_PIXELS (left, right or null), FBUS_SCREEN_CORNERS (left, right under geometry).  ids_out (may be ids),
    // nis, dof: batch() x M; kept: batch(); each may be null.  Read-only; hand ids_out to the update in place of ids.
    void screen_markers(int kind, int M, const int32_t* ids, const Real* a, const Real* b, int32_t* ids_out, Real* nis = nullptr,
                        int32_t* dof = nullptr, int32_t* kept = nullptr, int geometry = FBUS_VIS_REFRACTIVE, const uint8_t* skip = nullptr)
    { check(fbus_ekf_screen_markers(h_, kind, M, ids, a, b, geometry, skip, ids_out, nis, dof, kept), "screen_markers"); }
    void screen_markers_dev(int kind, int M, const int32_t* ids, const Real* a, const Real* b, int32_t* ids_out, Real* nis = nullptr,
                            int32_t* dof = nullptr, int32_t* kept = nullptr, int geometry = FBUS_VIS_REFRACTIVE, const uint8_t* skip = nullptr)
    { check(fbus_ekf_screen_markers_dev(h_, kind, M, ids, a, b, geometry, skip, ids_out, nis, dof, kept), "screen_markers_dev"); }

    // ---- consistency against a truth state (fbus_ekf.h; no reference counterpart): with delta = truth (-) estimate, nees =
    // delta_J' P_JJ^-1 delta_J for the FBUS_NEES_COLS blocks (FBUS_NEES_FULL, _POSE, _P .. _G), err = delta (order p v theta ba bg [g]),
    // lnp = the log-density of the truth under N(estimate, P).  truth: batch() x 19, ALWAYS double, in get_state's order; nees:
    // batch() x FBUS_NEES_COLS, err: batch() x nstate(), lnp: batch(), all double; each output may be null.  Read-only.
    void nees(const double* truth, double* nees, double* err = nullptr, double* lnp = nullptr, const uint8_t* skip = nullptr)
    { check(fbus_ekf_nees(h_, truth, skip, nees, err, lnp), "nees"); }
    void nees_dev(const double* truth, double* nees, double* err = nullptr, double* lnp = nullptr, const uint8_t* skip = nullptr)
    { check(fbus_ekf_nees_dev(h_, truth, skip, nees, err, lnp), "nees_dev"); }

    // ---- draws from every filter's own Gaussian (fbus_ekf.h; no reference counterpart), the inverse of nees(): S states per filter,
    // estimate (+) Pi' L xi with L L' = Pi P Pi' in the order p theta v ba bg [g].  xi: S x batch() x nstate(), ALWAYS double, in that
    // order; state: S x batch() x 19 double in get_state's order (a row is a ready truth for nees()); drawn: batch() bytes, 0 = skipped
    // or not positive definite (every row of that filter is its nominal).  S <= FBUS_SAMPLE_MAX; either output may be null.  Read-only.
    void sample(int S, const double* xi, double* state, uint8_t* drawn = nullptr, const uint8_t* skip = nullptr)
    { check(fbus_ekf_sample(h_, S, xi, skip, state, drawn), "sample"); }
    void sample_dev(int S, const double* xi, double* state, uint8_t* drawn = nullptr, const uint8_t* skip = nullptr)
    { check(fbus_ekf_sample_dev(h_, S, xi, skip, state, drawn), "sample_dev"); }

    // ---- predicted corner pixels with their innovation covariance (fbus_ekf.h): the h(x) of correct_pixels as an output.  ids: batch() x M;
    // cameras: 1 = left, 2 = stereo; left, right: batch() x M x 8 (x0 y0 .. x3 y3, the arrays correct_pixels takes); cov_left, cov_right:
    // batch() x M x 4 x 3, ALWAYS double, (S_uu, S_uv, S_vv) per corner of S = H P_JJ H' + r_pix I; view: batch() x M bytes, bit k = left
    // corner k in view, bit 4 + k = right corner k.  A projection out of view, an absent slot and a skipped filter give zeros.  Each output
    // may be null.  Read-only.
    void project_markers(int M, const int32_t* ids, int cameras, Real* left, Real* right = nullptr, uint8_t* view = nullptr,
                         double* cov_left = nullptr, double* cov_right = nullptr, const uint8_t* skip = nullptr)
    { check(fbus_ekf_project_markers(h_, M, ids, cameras, skip, left, right, cov_left, cov_right, view), "project_markers"); }
    void project_markers_dev(int M, const int32_t* ids, int cameras, Real* left, Real* right = nullptr, uint8_t* view = nullptr,
                             double* cov_left = nullptr, double* cov_right = nullptr, const uint8_t* skip = nullptr)
    { check(fbus_ekf_project_markers_dev(h_, M, ids, cameras, skip, left, right, cov_left, cov_right, view), "project_markers_dev"); }

    // ---- the body-velocity (DVL) update (fbus_ekf.h; no reference counterpart).  Three rows per filter,
    // h = C (R' v + (gyro - bg) x lever); at the instrument's own rate, between camera frames:
    //   loop { predict_n(imu since the last reading); correct_velocity(z, gyro, var); }
    // With z = 0 it is the zero-velocity update of a vehicle sitting on the bottom.  set_velocity_sensor first (mount: the rotation IMU
    // frame -> instrument frame, row-major, null = identity; lever: IMU frame, null = 0).  z, gyro: batch() x 3 (gyro may be null: no lever
    // term, the gyro bias is not observed); var: THREE variances or (per_filter) batch() x 3 of them, always double; a skipped filter, a
    // non-finite z or gyro component and a var that is not finite and > 0 leave the filter untouched; thr[3] of set_gate's table gates
    // every form.  nis / dof: batch() each, either may be null.
    void set_velocity_sensor(const double* mount = nullptr, const double* lever = nullptr)
    { check(fbus_ekf_set_velocity_sensor(h_, mount, lever), "fbus_ekf_set_velocity_sensor"); }
    void correct_velocity(const Real* z, const Real* gyro, const double* var, bool per_filter = false, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_velocity(h_, z, gyro, var, per_filter ? 1 : 0, skip), "correct_velocity"); }
    void correct_velocity_dev(const Real* z, const Real* gyro, const double* var, bool per_filter = false, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_velocity_dev(h_, z, gyro, var, per_filter ? 1 : 0, skip), "correct_velocity_dev"); }
    void correct_velocity_async(const Real* z, const Real* gyro, const double* var, bool per_filter = false, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_velocity_async(h_, z, gyro, var, per_filter ? 1 : 0, skip), "correct_velocity_async"); }
    void correct_velocity_nis(const Real* z, const Real* gyro, const double* var, bool per_filter, const uint8_t* skip, Real* nis, int32_t* dof)
    { check(fbus_ekf_correct_velocity_nis(h_, z, gyro, var, per_filter ? 1 : 0, skip, nis, dof), "correct_velocity_nis"); }
    void correct_velocity_nis_dev(const Real* z, const Real* gyro, const double* var, bool per_filter, const uint8_t* skip, Real* nis,
                                  int32_t* dof)
    { check(fbus_ekf_correct_velocity_nis_dev(h_, z, gyro, var, per_filter ? 1 : 0, skip, nis, dof), "correct_velocity_nis_dev"); }

    // ---- the general linearised measurement update (fbus_ekf.h; no reference counterpart): m = 1..FBUS_ROWS_MAX rows per filter,
    // res [B][m] = z - h(x) and H [B][m][N] (columns p v theta ba bg [g], R_true ~ R (I + [dtheta]x)) formed by the caller at the state
    // of get_state_dev; the library does the gain, the injection, the covariance, the NIS, the gate and the likelihood sums.
    //   loop { predict_n(...); get_state_dev(nominal, rot, nullptr, nullptr); <rows of the sensor on the device>; correct_rows_dev(...); }
    // No _async form: res and H are functions of the device-resident state.
    void correct_rows(int m, const Real* res, const Real* H, const double* var, bool per_filter = false, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_rows(h_, m, res, H, var, per_filter ? 1 : 0, skip), "correct_rows"); }
    void correct_rows_dev(int m, const Real* res, const Real* H, const double* var, bool per_filter = false, const uint8_t* skip = nullptr)
    { check(fbus_ekf_correct_rows_dev(h_, m, res, H, var, per_filter ? 1 : 0, skip), "correct_rows_dev"); }
    void correct_rows_nis(int m, const Real* res, const Real* H, const double* var, bool per_filter, const uint8_t* skip, Real* nis, int32_t* dof)
    { check(fbus_ekf_correct_rows_nis(h_, m, res, H, var, per_filter ? 1 : 0, skip, nis, dof), "correct_rows_nis"); }
    void correct_rows_nis_dev(int m, const Real* res, const Real* H, const double* var, bool per_filter, const uint8_t* skip, Real* nis,
                              int32_t* dof)
    { check(fbus_ekf_correct_rows_nis_dev(h_, m, res, H, var, per_filter ? 1 : 0, skip, nis, dof), "correct_rows_nis_dev"); }

    // (round 5) one camera frame with the north star's update in ONE launch (device pointers): K predicts, then correct_pixels
    // (kind = FBUS_MEAS_PIXELS; right may be null = left camera) or correct_corners (FBUS_MEAS_CORNERS with its geometry / mode) --
    // filter.cpp:232-235 with the reprojection rows in place of the pose rows
    void frame_meas_fused_dev(int K, const Real* accel, const Real* gyro, const Real* dt, int kind, int M, const int32_t* ids,
                              const Real* left, const Real* right = nullptr, int geometry = FBUS_VIS_REFRACTIVE,
                              Mode mode = Mode::Stacked, const uint8_t* skip = nullptr)
    {
        check(fbus_ekf_frame_meas_fused_dev(h_, K, accel, gyro, dt, 0, kind, M, ids, left, right, geometry, int(mode), skip),
              "frame_meas_fused_dev");
    }

    // ... and a window of such frames in one launch (offline replay of recorded corners; measurements [F][B][M]...)
    void frames_meas_fused_dev(const std::vector<int32_t>& kcount, const Real* accel, const Real* gyro, const Real* dt, int kind, int M,
                               const int32_t* ids, const Real* left, const Real* right = nullptr, int geometry = FBUS_VIS_REFRACTIVE,
                               Mode mode = Mode::Stacked, const uint8_t* skip = nullptr)
    {
        check(fbus_ekf_frames_meas_fused_dev(h_, int(kcount.size()), kcount.data(), accel, gyro, dt, 0, kind, M, ids, left, right, geometry,
                                             int(mode), skip), "frames_meas_fused_dev");
    }
    // ... with its trajectory (fbus_ekf_frames_meas_fused_traj_dev): device outputs [F][B][19], [F][B][N], [F][B], each may be null
    void frames_meas_fused_dev(const std::vector<int32_t>& kcount, const Real* accel, const Real* gyro, const Real* dt, int kind, int M,
                               const int32_t* ids, const Real* left, const Real* right, int geometry, Mode mode, const uint8_t* skip,
                               Real* out_nominal, Real* out_pdiag, uint8_t* out_applied)
    {
        check(fbus_ekf_frames_meas_fused_traj_dev(h_, int(kcount.size()), kcount.data(), accel, gyro, dt, 0, kind, M, ids, left, right,
                                                  geometry, int(mode), skip, out_nominal, out_pdiag, out_applied), "frames_meas_fused_traj_dev");
    }

    // waves per 64-filter tile (fbus_ekf_set_team): 0 = chosen per launch, 1 = always one, 2..4 = always that many
    void set_team(int predict_roles, int correct_roles) { check(fbus_ekf_set_team(h_, predict_roles, correct_roles), "set_team"); }

    std::vector<uint8_t> applied() const
    {
        std::vector<uint8_t> a(batch_);
        check(fbus_ekf_get_applied(h_, a.data()), "get_applied");
        return a;
    }
    // hip_stream is the hipStream_t itself (nullptr = HIP's legacy default stream); FBUS_STREAM_OWN = the handle's own
    void set_stream(void* hip_stream) { check(fbus_ekf_set_stream(h_, hip_stream), "set_stream"); }
    void wait_stream(void* other) { check(fbus_ekf_wait_stream(h_, other), "wait_stream"); }
    void signal_stream(void* other) { check(fbus_ekf_signal_stream(h_, other), "signal_stream"); }
    void sync() { check(fbus_ekf_sync(h_), "sync"); }

private:
    void check(int rc, const char* where) const
    {
        if (rc == FBUS_OK) return;
        std::string msg = std::string(where) + ": " + fbus_status_string(rc);
        if (h_) { const char* d = fbus_ekf_last_error(h_); if (d && *d) msg += std::string(" (") + d + ")"; }
        throw Error(rc, msg);
    }
    fbus_ekf_t h_ = nullptr;
    int batch_, nstate_;
};

}  // namespace fbus
