// fbus_ekf.hip -- the handle and the C ABI (include/fbus_ekf.h) of the MI355X-native batched error-state EKF: argument checks,
// transports, the choice of <T, N[, D]>, timing and the records_warm bookkeeping.  No kernel is defined or launched here: every
// launch goes through a launcher declared in ekf_launch.hpp and built in a kernel unit.  gfx950 only; no CPU fallback.
//
// HBM layout of the filter records ("64-filter tiles of 16-byte chunks"): a record is
// NRECP elements of T = NCH chunks of 16 bytes.  Filters are grouped in tiles of 64
// (one wave); a tile is NCH consecutive 1 KiB pieces and piece c holds chunk c of the
// tile's 64 filters, lane-major.  Chunk c of filter b is therefore at byte offset
// ((b / 64) * NCH + c) * 1024 + (b % 64) * 16: a wave moves its tile with NCH fully
// coalesced 1 KiB buffer_load_dwordx4 / buffer_store_dwordx4 over one contiguous
// NCH KiB region, and a rank's records are one contiguous block for the RCCL gather.
#define FBUS_EKF_NO_ABI_CHECK      // this file DEFINES fbus_ekf_create: no macro here
#include "../../include/fbus_ekf.h"
#include "ekf_launch.hpp"
#include "ekf_route.hpp"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include <limits>

using namespace fbus;

namespace {

// ---------------------------------------------------------------------------------
// host-side constants
// ---------------------------------------------------------------------------------
void rotmat_to_quat(const double R[9], double q[4])
{   // trace based, as Eigen's Quaterniond(Matrix3d) (filter.cpp:630, main.cpp marker load)
    double t = R[0] + R[4] + R[8];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (R[7] - R[5]) * t; q[2] = (R[2] - R[6]) * t; q[3] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[3 * k + j] - R[3 * j + k]) * t;
        q[1 + j] = (R[3 * j + i] + R[3 * i + j]) * t;
        q[1 + k] = (R[3 * k + i] + R[3 * i + k]) * t;
    }
}

struct HostConst {
    double R_IL[9], P_IL[3], Q_IL[4], CL[16];
    std::vector<double> mk;             // n_markers x MK_STRIDE
    std::vector<double> mkc;            // FBUS_MAX_MARKERS x MKC_STRIDE: corner 0, x axis, y axis of every marker (pixel fold, double)
    std::vector<short> id2slot;
};

bool build_host_const(const fbus_params& prm, HostConst& hc, std::string& err)
{
    // T_IL = diag(-1,-1,1,1) * T_SC_left    FBUS_EKF.m:68 ; filter.hpp:67-70
    double T[16];
    std::memcpy(T, prm.T_SC_left, sizeof(T));
    for (int j = 0; j < 4; ++j) { T[j] = -T[j]; T[4 + j] = -T[4 + j]; }
    double t[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) hc.R_IL[3 * i + j] = T[4 * i + j];
        t[i] = T[4 * i + 3];
    }
    for (int i = 0; i < 3; ++i)         // P_IL = -R_IL' t   MeasureUpdate.m:47 ; filter.cpp:631-632
        hc.P_IL[i] = -(hc.R_IL[i] * t[0] + hc.R_IL[3 + i] * t[1] + hc.R_IL[6 + i] * t[2]);
    rotmat_to_quat(hc.R_IL, hc.Q_IL);
    if (prm.n_markers < 0 || prm.n_markers > FBUS_MAX_MARKERS) { err = "n_markers out of range"; return false; }
    hc.id2slot.assign(FBUS_MAX_MARKER_ID + 1, (short)-1);
    hc.mk.assign((size_t)FBUS_MAX_MARKERS * MK_STRIDE, 0.0);        // always the full table: kernels copy it to LDS whole
    hc.mkc.assign((size_t)FBUS_MAX_MARKERS * MKC_STRIDE, 0.0);
    const double w = hc.Q_IL[0], x = hc.Q_IL[1], y = hc.Q_IL[2], z = hc.Q_IL[3];
    // Lq(Q_IL) * L2, L2 = diag(1,-1,-1,-1)   MeasureUpdate.m:39-44
    const double LL2[16] = { w,  x,  y,  z,
                             x, -w,  z, -y,
                             y, -z, -w,  x,
                             z,  y, -x, -w };
    std::memcpy(hc.CL, LL2, sizeof(LL2));
    for (int k = 0; k < prm.n_markers; ++k) {
        const int id = prm.marker_id[k];
        if (id < 0 || id > FBUS_MAX_MARKER_ID) { err = "marker id out of range"; return false; }
        hc.id2slot[id] = (short)k;
        double* m = &hc.mk[(size_t)k * MK_STRIDE];
        for (int i = 0; i < 3; ++i) m[i] = prm.marker_pos[k][i];
        double q[4];
        rotmat_to_quat(prm.marker_rot[k], q);
        for (int i = 0; i < 4; ++i) m[3 + i] = q[i];
        // c_m = 1/4 |Q_IL|^2 |Qm|^2: the isotropic information of the marker's four quaternion rows per unit weight and |q|^2
        // (PoseFold, ekf_device.hpp)
        m[7] = 0.25 * (w * w + x * x + y * y + z * z) * (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        // the marker frame of the corner / pixel rows in double: R_m = rotmat(quat(marker_rot)) as the other kernels (and the
        // oracle) build it -- quaternion_to_rotmat.m:22-33 -- corner k at P_m + R_m c_k, c_k in the marker's x-y plane
        double* c = &hc.mkc[(size_t)k * MKC_STRIDE];
        const double Rm0[3] = { q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3], 2 * (q[1] * q[2] + q[0] * q[3]), 2 * (q[1] * q[3] - q[0] * q[2]) };
        const double Rm1[3] = { 2 * (q[1] * q[2] - q[0] * q[3]), q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3], 2 * (q[2] * q[3] + q[0] * q[1]) };
        for (int i = 0; i < 3; ++i) { c[i] = prm.marker_pos[k][i]; c[3 + i] = Rm0[i]; c[6 + i] = Rm1[i]; }
    }
    return true;
}

}  // namespace

// ---------------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------------
struct fbus_ekf {
    // ---- launch policy, derived from the device at create (fbus_ekf_create), environment overrides read there once ----------
    LaunchPolicy lp;                  // SIMD count, two-wave threshold, vector measurement loads (handed to the launchers)
    int cus = 256;                    // hipDeviceProp::multiProcessorCount (FBUS_FAKE_SIMDS / 4 overrides it)
    size_t l2_bytes = (size_t)4 << 20;        // hipDeviceProp::l2CacheSize (one XCD's L2)
    size_t mall_bytes = (size_t)256 << 20;    // memory-side Infinity Cache: not exposed by the runtime; 256 MiB (MI300X / MI355X), FBUS_MALL_MB
    int policy_batch = 0;             // fbus_ekf_set_policy_batch: the batch the kernel-FAMILY choice is keyed on (0 = this handle's)
    bool records_warm = false;        // the last kernel stored the records with the default cache policy (they sit in L2)
    int big_records_mb = 56;          // records larger than this run the predict with default-policy loads and stores (FBUS_BIG_RECORDS_MB)
    bool warm_after_correct = false;  // experiment knob FBUS_WARM_AFTER_CORRECT=1: the first predict behind a correct takes the "warm" load policy
    int predict_ld = 0;               // record-load policy of the per-call predict: 0 auto (see launch_predict_t), 1 always nt, 2 always default
    int predict_policy_force = -1;    // FBUS_PREDICT_POLICY=0|1|2 (sweeps): nt / nt, default loads + nt stores, default / default
    int B = 0, Bs = 0, device = 0, dtype = 32, N = 18;
    // RCCL communicator of the multi-GPU gather (fbus_ekf_comm_*): one rank per handle
    void* comm = nullptr;
    bool own_comm = false;
    int comm_rank = 0, comm_world = 1;
    // team kernels (several waves per 64-filter tile, ekf_team.hpp): 0 = chosen per launch from the wave count, 1 = never,
    // 2..4 = always with that many roles (fbus_ekf_set_team, FBUS_TEAM_PREDICT / FBUS_TEAM_CORRECT at create)
    int team_predict = 0, team_correct = 0;
    int team_frame = 0;               // FBUS_TEAM_FRAME: 0 = follows team_predict, 1 = never, 2 = always
    int meas_split = -1;              // FBUS_MEAS_SPLIT: -1 auto, 0 never, 2 / 4: always the divided-update pixel kernel with that many waves per tile
    bool no_frame_meas = false;       // FBUS_NO_FRAME_MEAS=1 (A/B runs): fbus_ekf_frame_meas_fused_dev always as predict_n + the per-call update
    fbus_params prm{};
    HostConst hc;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t order_ev = nullptr;    // fbus_ekf_wait_stream / fbus_ekf_signal_stream
    void* recs = nullptr;
    bool own_recs = false;
    size_t rec_bytes = 0, bytes_per_filter = 0;
    void* d_mk = nullptr;
    double* d_mkc = nullptr;            // HostConst::mkc on the device
    short* d_id2slot = nullptr;
    unsigned char* d_applied = nullptr;
    // the NIS gate (fbus_ekf_set_gate): FBUS_GATE_MAX_DOF + 1 thresholds on the device, +inf past gate_n (gate_n = 0: no table); allocated
    // at create and never moved, so a captured _nis_dev call reads the table that is current at its replay
    double* d_gate = nullptr;
    int gate_n = 0;
    // per-filter noise (fbus_ekf_set_noise): the table as fields [FBUS_NOISE_COLS][B] in double, followed by FBUS_GATE_MAX_DOF + 1 entries
    // of +inf (the "no gate" table of the plain pose update, which runs the NIS kernel on the tabled route); allocated at the first
    // set_noise and never moved, so a captured call reads the values current at its replay.  noise_on: the tabled routes are taken
    double* d_noise = nullptr;
    bool noise_on = false;
    // innovation log-likelihood sums (fbus_ekf_loglik_*): [4][B] doubles (ll, rows, applied, rejected), allocated at the first enable and
    // never moved.  lik_on: every measurement update takes the tabled one-wave route with the likelihood kernels (families 17 / 18);
    // without a noise table d_noise then holds fbus_params' own row (lik_fill), and noise_on stays false: predict keeps its untabled kernels
    double* d_lik = nullptr;
    bool lik_on = false;
    // the depth sensor (fbus_ekf_set_depth_sensor): handed to correct_depth_kernel by value at every launch, so a captured graph keeps
    // the values it was captured with.  depth_set: no correct_depth* form runs before the setter has been called
    DepthSensor depth{};
    bool depth_set = false;
    // the velocity sensor (fbus_ekf_set_velocity_sensor), by value at every launch as the depth sensor is; velocity_set: no
    // correct_velocity* form runs before the setter has been called
    VelocitySensor velocity{};
    bool velocity_set = false;
    void* d_ema_carry = nullptr;        // B x 6, previous EMA-filtered IMU sample
    bool ema_has_carry = false;
    // staging for the host-pointer entry points (grown on demand)
    void* stage[7] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };      // (seven arrays: fbus_ekf_screen_markers)
    size_t stage_cap[7] = { 0, 0, 0, 0, 0, 0, 0 };
    // asynchronous host-pointer entry points (fbus_ekf_predict_async / _correct_async): a ring of pinned staging slots + a copy stream
    struct AsyncSlot { void* host = nullptr; void* dev = nullptr; size_t cap = 0; hipEvent_t copied = nullptr, done = nullptr; bool busy = false; };
    static constexpr int ASYNC_SLOTS = 8;
    AsyncSlot aring[ASYNC_SLOTS];
    unsigned anext = 0;
    hipStream_t copy_stream = nullptr;
    int64_t async_calls = 0, async_waits = 0, async_direct = 0;      // calls, calls that had to wait for a slot, pieces DMA'd in place
    std::string err;
    // timing
    bool timing = false;
    struct EvPair { hipEvent_t a, b; int kind; int count; };
    bool timing_suspended = false;   // frame_dev brackets its run of predicts with ONE pair
    int timing_stride = 1;           // frame_dev: bracket every stride-th frame only
    bool capturing = false;          // between graph_begin and graph_end: no events, no host syncs
    std::vector<hipGraphExec_t> graphs;
    int64_t frame_count = 0;
    std::vector<EvPair> ev_pool;
    size_t ev_used = 0;
    double t_ms[FBUS_KERNEL_COUNT] = { 0, 0, 0, 0, 0, 0 };
    int64_t t_n[FBUS_KERNEL_COUNT] = { 0, 0, 0, 0, 0, 0 };
};

namespace {

// Every entry point runs with the handle's device current (a process may hold handles on several GPUs) and
// restores the caller's device on return.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const fbus_ekf* h) { if (h) enter(h->device); }
    explicit DeviceGuard(int device) { enter(device); }
    void enter(int device)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = (hipSetDevice(device) == hipSuccess);
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

int fail(fbus_ekf_t h, int code, const std::string& msg)
{
    if (h) h->err = msg;
    return code;
}

#define HIP_TRY(h, call)                                                                        \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((h), FBUS_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

size_t esize(const fbus_ekf* h) { return h->dtype == 32 ? 4 : 8; }
// what the entry points accept: an update mode, a corner geometry, and image-point arrays on a 16-byte boundary -- the kernels fetch a
// slot's points with 16-byte loads (a slot is 32 / 48 contiguous bytes): any allocation is aligned, a view offset by one to three
// elements is not and is refused, not read unaligned
bool mode_ok(int mode) { return mode == FBUS_MODE_NEAREST || mode == FBUS_MODE_STACKED; }
bool geometry_ok(int g) { return g == FBUS_VIS_REFRACTIVE || g == FBUS_VIS_PINHOLE || g == FBUS_VIS_CORNERS3D; }
bool points_aligned(const void* left, const void* right)
{
    return ((reinterpret_cast<uintptr_t>(left) | reinterpret_cast<uintptr_t>(right)) & 15) == 0;
}

template <typename T>
DevConst<T> make_dc(const fbus_ekf* h)
{
    DevConst<T> dc;
    for (int i = 0; i < 4; ++i) dc.qd[i] = (T)h->prm.q_diag[i];
    dc.r_pos = (T)h->prm.r_pos;
    dc.r_quat = (T)h->prm.r_quat;
    for (int i = 0; i < 9; ++i) dc.R_IL[i] = (T)h->hc.R_IL[i];
    for (int i = 0; i < 3; ++i) dc.P_IL[i] = (T)h->hc.P_IL[i];
    for (int i = 0; i < 4; ++i) dc.Q_IL[i] = (T)h->hc.Q_IL[i];
    for (int i = 0; i < 16; ++i) dc.CL[i] = (T)h->hc.CL[i];
    dc.switch_thres = (T)h->prm.switch_thres;
    dc.cov_form = h->prm.cov_form;
    dc.mk = (const T*)h->d_mk;
    dc.id2slot = h->d_id2slot;
    return dc;
}

int flush_events(fbus_ekf_t h)
{
    if (h->ev_used == 0) return FBUS_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < h->ev_used; ++i) {
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->ev_pool[i].a, h->ev_pool[i].b));
        h->t_ms[h->ev_pool[i].kind] += ms;
        h->t_n[h->ev_pool[i].kind] += h->ev_pool[i].count;
    }
    h->ev_used = 0;
    return FBUS_OK;
}

// returns the index of the event pair to close after the launch, or -1
int timing_begin(fbus_ekf_t h, int kind, int count = 1)
{
    if (!h->timing || h->timing_suspended || h->capturing) return -1;
    if (h->ev_used == h->ev_pool.size()) {
        if (h->ev_pool.size() >= 8192) {
            if (flush_events(h) != FBUS_OK) return -1;
        } else {
            fbus_ekf::EvPair p;
            if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return -1;
            h->ev_pool.push_back(p);
        }
    }
    const int i = (int)h->ev_used++;
    h->ev_pool[i].kind = kind;
    h->ev_pool[i].count = count;
    (void)hipEventRecord(h->ev_pool[i].a, h->stream);
    return i;
}

void timing_end(fbus_ekf_t h, int i)
{
    if (i >= 0) (void)hipEventRecord(h->ev_pool[i].b, h->stream);
}

// The launch policy (ekf_route.hpp: which kernels a call runs) reads the handle through this key alone.
static_assert(ROUTE_MODE_NEAREST == FBUS_MODE_NEAREST && ROUTE_MODE_STACKED == FBUS_MODE_STACKED && ROUTE_PIXELS == FBUS_MEAS_PIXELS &&
              ROUTE_CORNERS == FBUS_MEAS_CORNERS && ROUTE_MAX_RESIDENT_K == 255, "ekf_route.hpp restates include/fbus_ekf.h");
RouteKey route_key(const fbus_ekf* h)
{
    const double* n = h->prm.port_normal;
    RouteKey k;
    k.dtype = h->dtype;
    k.joseph = h->prm.cov_form == FBUS_COV_JOSEPH;
    k.noise_on = h->noise_on;
    k.lik_on = h->lik_on;
    k.tiles = policy_tiles_of(h->policy_batch, h->B);
    k.simds = h->lp.simds;
    k.team_predict = h->team_predict;
    k.team_correct = h->team_correct;
    k.team_frame = h->team_frame;
    k.meas_split = h->meas_split;
    k.no_frame_meas = h->no_frame_meas;
    k.square_port = n[0] == 0.0 && n[1] == 0.0 && n[2] == 1.0;
    return k;
}

template <typename T, int N, int D>
int launch_predict_t(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter)
{
    const int ev = timing_begin(h, K == 1 ? FBUS_KERNEL_PREDICT : FBUS_KERNEL_PREDICT_N);
    // the first predict after a kernel that stored the records with the default cache policy (correct, fused frame)
    // reads them with the default policy too; the others stream them non-temporally (see predict_kernel)
    // ... and larger batches run with the default policy on loads AND stores.  Measured on the final round-2 kernels
    // (profiles/logs/r02_policy_by_size.log, headline nt/nt -> default/default): 65 536 filters (52 MB of records, 1024 waves = one
    // round) 4.91e9 -> 4.39e9; 73 728: +1 %; 81 920: +2.5 %; 98 304: +3 %; 131 072: +7 %; 163 840: +11 %; 196 608: +13 %;
    // 262 144 (210 MB): 65.4 -> 55.7 us per launch.  The non-temporal stream only pays while the whole batch is one round of
    // waves whose records stay in the Infinity Cache between launches; the threshold sits just above that batch.
    // Round 3 sweep (profiles/logs/r03_policy_sweep.txt: fp32 N = 18 / N = 15 and fp64, 32 768 .. 1 048 576 filters, all three
    // policies forced through the environment knobs): the crossover between nt / nt and default / default sits at 52-60 MB of
    // records for 800-byte, 608-byte AND 1600-byte records alike (768 waves of fp64 records are on the default side, 1024 waves
    // of N = 15 records on the nt side): a cache-capacity effect, keyed on bytes, not on the wave count.  Beyond the 256 MiB
    // Infinity Cache the records stream from HBM and non-temporal STORES win again (524 288 filters = 419 MB: 133 -> 116 us
    // with default loads; 1 048 576 = 839 MB: 290 -> 275 us with nt loads as well -- nothing is left to hit).
    const size_t mall = h->mall_bytes;
    const bool big = h->rec_bytes > ((size_t)h->big_records_mb << 20);
    int policy = (big ? 2 : (h->records_warm ? 1 : 0));
    if (big && h->rec_bytes > mall) policy = (h->rec_bytes > 2 * mall) ? 0 : 1;
    if (h->predict_ld == 1) policy = 0;
    if (h->predict_ld == 2) policy = big ? 2 : 1;
    if (h->predict_policy_force >= 0) policy = h->predict_policy_force;
    h->records_warm = false;
    const int roles = team_roles_predict(route_key(h), K);
    const auto one_wave = [&](auto... x) {
        launch_predict_k<T, N, D>(h->stream, (T*)h->recs, h->B, K, policy, (const T*)accel, (const T*)gyro, (const T*)dt,
                                  dt_per_filter ? 1 : 0, make_dc<T>(h), h->lp, x...);
    };
    if constexpr (sizeof(T) == 4) {
        if (roles > 1)
            launch_predict_team_k<T, N, D>(h->stream, (T*)h->recs, h->B, K, roles, policy, (const T*)accel, (const T*)gyro,
                                           (const T*)dt, dt_per_filter ? 1 : 0, make_dc<T>(h));
    }
    if (h->noise_on) one_wave(NoiseIn{ h->d_noise, h->B });     // (roles == 1) the same kernel choice with this filter's q
    else if (roles <= 1 || sizeof(T) != 4) one_wave();
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}

// Outputs of an _nis call: nis [B] in the record type and dof [B] on the device, each may be null
struct NisDst { void* nis; int32_t* dof; };
// One measurement update with the pack that the handle and the call ask for; `go(x...)` launches it.  While the likelihood sums are on:
// NisOut, NoiseIn, LikOut; on a tabled handle: NisOut, NoiseIn; an _nis call (nis != nullptr) otherwise: NisOut; the plain update: none.
// An _nis call gates with the handle's table; the plain update of a tabled handle runs the NIS kernel with no outputs and `no_gate`.
template <typename T, typename GO>
void with_update_pack(fbus_ekf_t h, const NisDst* nis, const double* no_gate, GO go)
{
    const NisOut<T> no = nis ? NisOut<T>{ (T*)nis->nis, (int*)nis->dof, h->d_gate } : NisOut<T>{ nullptr, nullptr, no_gate };
    const NoiseIn ni{ h->d_noise, h->B };
    if (h->lik_on) go(no, ni, LikOut{ h->d_lik, h->B });
    else if (h->noise_on) go(no, ni);
    else if (nis) go(no);
    else go();
}
template <typename T, int N, int D>
int launch_correct_t(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode,
                     const uint8_t* skip, const NisDst* nis = nullptr)
{
    const int ev = timing_begin(h, FBUS_KERNEL_CORRECT);
    h->records_warm = h->warm_after_correct;   // false: written through (sc1), the next predict streams them like any other
    // (the pose kernel always reads a gate table: "no gate" is the row of +inf behind the noise table)
    const double* no_gate = tabled(route_key(h)) ? h->d_noise + (size_t)FBUS_NOISE_COLS * h->B : nullptr;
    with_update_pack<T>(h, nis, no_gate, [&](auto... x) {
        launch_correct_k<T, N, D>(h->stream, (T*)h->recs, h->B, M, (const int*)ids, (const T*)pos, (const T*)quat, mode,
                                  h->prm.cov_form == FBUS_COV_JOSEPH, (const unsigned char*)skip, h->d_applied, make_dc<T>(h), h->lp, x...);
    });
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}

#define DISPATCH(h, FN, ...)                                                                     \
    do {                                                                                         \
        const int key_ = ((h)->dtype == 64 ? 4 : 0) | ((h)->N == 15 ? 2 : 0) | ((h)->prm.dialect == FBUS_DIALECT_CPP ? 1 : 0); \
        switch (key_) {                                                                          \
            case 0: return FN<float, 18, DIALECT_MATLAB>(__VA_ARGS__);                           \
            case 1: return FN<float, 18, DIALECT_CPP>(__VA_ARGS__);                              \
            case 2: return FN<float, 15, DIALECT_MATLAB>(__VA_ARGS__);                           \
            case 3: return FN<float, 15, DIALECT_CPP>(__VA_ARGS__);                              \
            case 4: return FN<double, 18, DIALECT_MATLAB>(__VA_ARGS__);                          \
            case 5: return FN<double, 18, DIALECT_CPP>(__VA_ARGS__);                             \
            case 6: return FN<double, 15, DIALECT_MATLAB>(__VA_ARGS__);                          \
            default: return FN<double, 15, DIALECT_CPP>(__VA_ARGS__);                            \
        }                                                                                        \
    } while (0)

// the kernels that exist for fp32 records only (team, resident windows): their routes are never chosen for fp64 records (ekf_route.hpp)
#define DISPATCH_F32(h, FN, ...)                                                                 \
    do {                                                                                         \
        switch (((h)->dtype == 64 ? 4 : 0) | ((h)->N == 15 ? 2 : 0) | ((h)->prm.dialect == FBUS_DIALECT_CPP ? 1 : 0)) { \
            case 0: return FN<float, 18, DIALECT_MATLAB>(__VA_ARGS__);                           \
            case 1: return FN<float, 18, DIALECT_CPP>(__VA_ARGS__);                              \
            case 2: return FN<float, 15, DIALECT_MATLAB>(__VA_ARGS__);                           \
            case 3: return FN<float, 15, DIALECT_CPP>(__VA_ARGS__);                              \
            default: return fail((h), FBUS_ERR_UNSUPPORTED, #FN ": an fp32 route for fp64 records"); \
        }                                                                                        \
    } while (0)

int launch_predict(fbus_ekf_t h, int K, const void* a, const void* g, const void* dt, int per)
{
    DISPATCH(h, launch_predict_t, h, K, a, g, dt, per);
}

int launch_correct(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode,
                   const uint8_t* skip, const NisDst* nis = nullptr)
{
    DISPATCH(h, launch_correct_t, h, M, ids, pos, quat, mode, skip, nis);
}

// ---- the bodies of the frame and window routes (ekf_route.hpp; the entry points choose, these launch) ---------------------------------------
// Output slices of a trajectory window (fbus_ekf_frames_fused_traj_dev / _frames_meas_fused_traj_dev): [nframes][B][19], [nframes][B][N],
// [nframes][B]; any may be null
struct TrajDst { void* nom; void* pdiag; uint8_t* applied; };

// FRAME_FUSED / FRAME_F64_FUSED: one camera frame in ONE launch, one wave per tile.  fp64 (round 4; stacked, simple form): the parked
// K-step predict loop + the row-split passes with the record resident in registers / LDS (frame2_kernel<double>)
template <typename T, int N, int D>
int launch_frame_t(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter, int M,
                   const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip)
{
    const int ev = timing_begin(h, FBUS_KERNEL_FRAME);
    h->records_warm = true;
    launch_frame_k<T, N, D>(h->stream, (T*)h->recs, h->B, K, (const T*)accel, (const T*)gyro, (const T*)dt,
                            dt_per_filter ? 1 : 0, M, (const int*)ids, (const T*)pos, (const T*)quat, mode,
                            h->prm.cov_form == FBUS_COV_JOSEPH, (const unsigned char*)skip, h->d_applied, make_dc<T>(h), h->lp);
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int launch_frame(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int per, int M,
                 const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip)
{
    DISPATCH(h, launch_frame_t, h, K, accel, gyro, dt, per, M, ids, pos, quat, mode, skip);
}

// One launch of a one-wave window kernel with the pack the entry point chose beside the route (window_pack); `go(x...)` launches it.
// tj: frame f's rows written from its registers; a tabled handle's window without rows passes three null pointers.
template <typename T, typename GO>
void with_window_pack(fbus_ekf_t h, WindowPack pack, const TrajDst* tj, GO go)
{
    const TrajOut<T> to = tj ? TrajOut<T>{ (T*)tj->nom, (T*)tj->pdiag, tj->applied } : TrajOut<T>{ nullptr, nullptr, nullptr };
    switch (pack) {
        case PACK_TRAJ_NOISE: go(to, NoiseIn{ h->d_noise, h->B }); break;
        case PACK_TRAJ: go(to); break;
        case PACK_NONE: go(); break;
    }
}
// WINDOW_ONE_WAVE, and FRAME_TABLED_RESIDENT with F = 1 (pose rows): frames_kernel
template <typename T, int N, int D>
int launch_frames_t(fbus_ekf_t h, WindowPack pack, int F, const unsigned char* kc, const void* accel, const void* gyro, const void* dt,
                    int dt_per_filter, int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip,
                    const TrajDst* tj)
{
    const int ev = timing_begin(h, FBUS_KERNEL_FRAME, F);
    h->records_warm = true;
    with_window_pack<T>(h, pack, tj, [&](auto... x) {
        launch_frames_k<T, N, D>(h->stream, (T*)h->recs, h->B, F, kc, (const T*)accel, (const T*)gyro, (const T*)dt,
                                 dt_per_filter ? 1 : 0, M, (const int*)ids, (const T*)pos, (const T*)quat, mode,
                                 h->prm.cov_form == FBUS_COV_JOSEPH, (const unsigned char*)skip, h->d_applied, make_dc<T>(h), x...);
    });
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int launch_frames(fbus_ekf_t h, WindowPack pack, int F, const unsigned char* kc, const void* a, const void* g, const void* dt, int per, int M,
                  const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip, const TrajDst* tj)
{
    DISPATCH_F32(h, launch_frames_t, h, pack, F, kc, a, g, dt, per, M, ids, pos, quat, mode, skip, tj);
}
// WINDOW_TEAM, and FRAME_TEAM with F = 1: frames_team_kernel
template <typename T, int N, int D>
int launch_frames_team_t(fbus_ekf_t h, int F, const unsigned char* kc, const void* accel, const void* gyro, const void* dt,
                         int dt_per_filter, int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip)
{
    const int ev = timing_begin(h, FBUS_KERNEL_FRAME, F);
    h->records_warm = true;
    launch_frames_team_k<T, N, D>(h->stream, (T*)h->recs, h->B, F, kc, (const T*)accel, (const T*)gyro, (const T*)dt,
                                  dt_per_filter ? 1 : 0, M, (const int*)ids, (const T*)pos, (const T*)quat, mode,
                                  (const unsigned char*)skip, h->d_applied, make_dc<T>(h));
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int launch_frames_team(fbus_ekf_t h, int F, const unsigned char* kc, const void* a, const void* g, const void* dt, int per, int M,
                       const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip)
{
    DISPATCH_F32(h, launch_frames_team_t, h, F, kc, a, g, dt, per, M, ids, pos, quat, mode, skip);
}


template <typename T, int N>
int pack_t(fbus_ekf_t h, const void* nom, const void* rot, const void* P, const int32_t* prev)
{
    launch_pack_k<T, N>(h->stream, (T*)h->recs, h->B, (const T*)nom, (const T*)rot, (const T*)P, (const int*)prev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}

template <typename T, int N>
int unpack_t(fbus_ekf_t h, void* nom, void* rot, void* P, int32_t* prev)
{
    launch_unpack_k<T, N>(h->stream, (const T*)h->recs, h->B, (T*)nom, (T*)rot, (T*)P, (int*)prev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}

template <typename T, int N>
int reset_cov_t(fbus_ekf_t h)
{
    launch_reset_cov_k<T, N>(h->stream, (T*)h->recs, h->B, h->prm.p0_diag);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}

#define DISPATCH2(h, FN, ...)                                                        \
    do {                                                                             \
        if ((h)->dtype == 32) {                                                      \
            if ((h)->N == 18) return FN<float, 18>(__VA_ARGS__);                     \
            return FN<float, 15>(__VA_ARGS__);                                       \
        }                                                                            \
        if ((h)->N == 18) return FN<double, 18>(__VA_ARGS__);                        \
        return FN<double, 15>(__VA_ARGS__);                                          \
    } while (0)

int do_pack(fbus_ekf_t h, const void* n, const void* r, const void* P, const int32_t* pv) { DISPATCH2(h, pack_t, h, n, r, P, pv); }
int do_unpack(fbus_ekf_t h, void* n, void* r, void* P, int32_t* pv) { DISPATCH2(h, unpack_t, h, n, r, P, pv); }
int do_reset_cov(fbus_ekf_t h) { DISPATCH2(h, reset_cov_t, h); }

template <typename T, int N>
int snapshot_t(fbus_ekf_t h, void* nom, void* pdiag, uint8_t* applied)
{
    launch_snapshot_k<T, N>(h->stream, (const T*)h->recs, h->B, h->d_applied, (T*)nom, (T*)pdiag, applied);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int do_snapshot(fbus_ekf_t h, void* n, void* pd, uint8_t* a) { DISPATCH2(h, snapshot_t, h, n, pd, a); }
// ---- hypothesis groups (ekf_group.hpp): one wave per floor(64 / G) whole groups ------------------------------------------------------------
template <typename T, int N>
int group_fuse_t(fbus_ekf_t h, int G, const double* logw, double* weight, int32_t* best, void* nom, void* P, void* pdiag)
{
    launch_group_fuse_k<T, N>(h->stream, (const T*)h->recs, h->rec_bytes, h->B, G, logw, weight, (int*)best, (T*)nom, (T*)P, (T*)pdiag);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int do_group_fuse(fbus_ekf_t h, int G, const double* lw, double* w, int32_t* best, void* nom, void* P, void* pd)
{
    DISPATCH2(h, group_fuse_t, h, G, lw, w, best, nom, P, pd);
}
template <typename T, int N>
int group_collapse_t(fbus_ekf_t h, int G, const int32_t* src)
{
    h->records_warm = true;                                  // stored with the default cache policy
    launch_group_collapse_k<T, N>(h->stream, (T*)h->recs, h->rec_bytes, h->B, G, (const int*)src);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int do_group_collapse(fbus_ekf_t h, int G, const int32_t* src) { DISPATCH2(h, group_collapse_t, h, G, src); }
template <typename T, int N>
int group_mix_t(fbus_ekf_t h, int G, const double* logw, const double* trans, double* weight, double* logc)
{
    h->records_warm = true;                                  // stored with the default cache policy
    launch_group_mix_k<T, N>(h->stream, (T*)h->recs, h->rec_bytes, h->B, G, logw, trans, weight, logc);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int do_group_mix(fbus_ekf_t h, int G, const double* lw, const double* tr, double* w, double* lc) { DISPATCH2(h, group_mix_t, h, G, lw, tr, w, lc); }
// ---- the streamed sensor updates (ekf_depth.hpp, ekf_velocity.hpp, ekf_rows.hpp): one launcher for every form of each, one route: one wave
// per tile whatever the batch, the team setting, the noise table or the likelihood switch.  The gate table is the handle's (+inf without
// one), the likelihood accumulator null while the sums are off.  SensorDev: the arrays every one of them takes behind its own inputs
struct SensorDev { const double* var; int var_stride; const unsigned char* skip; void* nis; int* dof; };
// `go(lik)` launches the update
template <typename GO>
int launch_sensor(fbus_ekf_t h, GO go)
{
    h->records_warm = h->warm_after_correct;      // written through (sc1), as correct_kernel's records
    go(h->lik_on ? h->d_lik : nullptr);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
template <typename T, int N>
int launch_depth_t(fbus_ekf_t h, const void* z, const SensorDev& d)
{
    return launch_sensor(h, [&](double* lik) {
        launch_depth_k<T, N>(h->stream, (T*)h->recs, h->B, (const T*)z, d.var, d.var_stride, d.skip, h->d_applied, h->depth, h->d_gate,
                             (T*)d.nis, d.dof, lik);
    });
}
int launch_depth(fbus_ekf_t h, const void* z, const SensorDev& d) { DISPATCH2(h, launch_depth_t, h, z, d); }
template <typename T, int N>
int launch_velocity_t(fbus_ekf_t h, const void* z, const void* gyro, const SensorDev& d)
{
    return launch_sensor(h, [&](double* lik) {
        launch_velocity_k<T, N>(h->stream, (T*)h->recs, h->B, (const T*)z, (const T*)gyro, d.var, d.var_stride, d.skip, h->d_applied,
                                h->velocity, h->d_gate, (T*)d.nis, d.dof, lik);
    });
}
int launch_velocity(fbus_ekf_t h, const void* z, const void* gyro, const SensorDev& d) { DISPATCH2(h, launch_velocity_t, h, z, gyro, d); }
template <typename T, int N>
int launch_rows_t(fbus_ekf_t h, int m, const void* res, const void* H, const SensorDev& d)
{
    return launch_sensor(h, [&](double* lik) {
        launch_rows_k<T, N>(h->stream, (T*)h->recs, h->B, m, (const T*)res, (const T*)H, d.var, d.var_stride, d.skip, h->d_applied, h->d_gate,
                            (T*)d.nis, d.dof, lik);
    });
}
int launch_rows(fbus_ekf_t h, int m, const void* res, const void* H, const SensorDev& d) { DISPATCH2(h, launch_rows_t, h, m, res, H, d); }

// the snapshot into row block f of a trajectory window's outputs (the frame-by-frame routes)
int snapshot_row(fbus_ekf_t h, const TrajDst& tj, int f)
{
    const size_t es = esize(h), rows = (size_t)f * h->B;
    return do_snapshot(h, tj.nom ? (char*)tj.nom + rows * 19 * es : nullptr, tj.pdiag ? (char*)tj.pdiag + rows * h->N * es : nullptr,
                       tj.applied ? tj.applied + rows : nullptr);
}
// does a device output of `bytes` at p overlap the records (the rule of fbus_ekf_snapshot_dev)?
bool in_records(fbus_ekf_t h, const void* p, size_t bytes)
{
    const uintptr_t r0 = reinterpret_cast<uintptr_t>(h->recs), r1 = r0 + h->rec_bytes, a = reinterpret_cast<uintptr_t>(p);
    return p && a < r1 && a + bytes > r0;
}
// outputs must not overlap the records (the kernels read the records while the rows go out); FBUS_ERR_INVALID otherwise
int check_traj(fbus_ekf_t h, const TrajDst& tj, int nframes, const char* what)
{
    const size_t es = esize(h), rows = (size_t)nframes * h->B;
    if (in_records(h, tj.nom, rows * 19 * es) || in_records(h, tj.pdiag, rows * h->N * es) || in_records(h, tj.applied, rows))
        return fail(h, FBUS_ERR_INVALID, std::string(what) + ": an output overlaps the records");
    return FBUS_OK;
}

template <typename T>
VisConst<T> make_vc(const fbus_ekf* h)
{
    const fbus_params& p = h->prm;
    double RL[9], RR[9], PL[3], PR[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { RL[3 * i + j] = p.T_SC_left[4 * i + j]; RR[3 * i + j] = p.T_SC_right[4 * i + j]; }
        PL[i] = p.T_SC_left[4 * i + 3]; PR[i] = p.T_SC_right[4 * i + 3];
    }
    VisConst<T> vc;
    double Rrl[9], Rlr[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = 0, b = 0;
            for (int k = 0; k < 3; ++k) { a += RL[3 * i + k] * RR[3 * j + k]; b += RR[3 * i + k] * RL[3 * j + k]; }
            Rrl[3 * i + j] = a; Rlr[3 * i + j] = b;
        }
    for (int i = 0; i < 3; ++i) {
        double a = 0, b = 0;
        for (int k = 0; k < 3; ++k) { a += Rrl[3 * i + k] * PR[k]; b += Rlr[3 * i + k] * PR[k]; }
        vc.P_LR[i] = (T)(PL[i] - a);
        vc.t_LRn[i] = (T)(PL[i] - b);
    }
    for (int i = 0; i < 9; ++i) { vc.R_RL[i] = (T)Rrl[i]; vc.R_LRn[i] = (T)Rlr[i]; }
    {   // exact inverse of R_RL (adjugate / determinant), for the forward projection into the right camera
        const double* m = Rrl;
        const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
        const double inv[9] = { (m[4] * m[8] - m[5] * m[7]), (m[2] * m[7] - m[1] * m[8]), (m[1] * m[5] - m[2] * m[4]),
                                (m[5] * m[6] - m[3] * m[8]), (m[0] * m[8] - m[2] * m[6]), (m[2] * m[3] - m[0] * m[5]),
                                (m[3] * m[7] - m[4] * m[6]), (m[1] * m[6] - m[0] * m[7]), (m[0] * m[4] - m[1] * m[3]) };
        for (int i = 0; i < 9; ++i) vc.R_RL_inv[i] = (T)(inv[i] / det);
    }
    vc.alpha0 = (T)(p.n_air / p.n_glass);
    vc.alpha1 = (T)(p.n_glass / p.n_water);
    vc.sqrt_minus0 = p.n_air < p.n_glass;       // vision.cpp:513
    vc.sqrt_minus1 = p.n_glass > p.n_water;     // vision.cpp:532
    vc.d_air = (T)p.d_air; vc.d_glass = (T)p.d_glass;
    for (int i = 0; i < 3; ++i) vc.nrm[i] = (T)p.port_normal[i];
    {
        const double a = (p.n_air / p.n_glass) * (p.n_glass / p.n_water);
        for (int i = 0; i < 3; ++i) {
            vc.tri[2 * i] = (T)(a * Rrl[3 * i]); vc.tri[2 * i + 1] = (T)(a * Rrl[3 * i + 1]);
            vc.tri[6 + i] = (T)(Rrl[3 * i + 2] * (p.d_air + p.d_glass) + (double)vc.P_LR[i]);
        }
        vc.tri[9] = (T)(p.d_air / a); vc.tri[10] = (T)(p.d_glass * (p.n_air / p.n_glass) / a); vc.tri[11] = (T)a;
    }
    return vc;
}

// constants of the round-4 pixel fold (double whatever the record type)
MeasConst make_mc(const fbus_ekf* h)
{
    const fbus_params& p = h->prm;
    const VisConst<double> vc = make_vc<double>(h);
    MeasConst mc;
    for (int i = 0; i < 3; ++i) mc.P_IL[i] = h->hc.P_IL[i];
    // XL = F R_IL t_I (the triangulation's axis flip undone, vision.cpp:597-599); XR = R_RL^-1 (XL - P_LR) (vision.cpp:555-556)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) mc.McL[3 * i + j] = (i < 2 ? -1.0 : 1.0) * h->hc.R_IL[3 * i + j];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            double a = 0;
            for (int k = 0; k < 3; ++k) a += vc.R_RL_inv[3 * i + k] * mc.McL[3 * k + j];
            mc.McR[3 * i + j] = a;
        }
        double b = 0;
        for (int k = 0; k < 3; ++k) b += vc.R_RL_inv[3 * i + k] * vc.P_LR[k];
        mc.tR[i] = -b;
    }
    for (int j = 0; j < 3; ++j) {
        mc.n[j] = p.port_normal[j];
        mc.nML[j] = mc.nMR[j] = 0;
    }
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) { mc.nML[j] += mc.n[i] * mc.McL[3 * i + j]; mc.nMR[j] += mc.n[i] * mc.McR[3 * i + j]; }
    {   // R_IL' R_IL = McL' McL (F is orthogonal)
        const double* Mm = mc.McL;
        int o = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j) mc.NI[o++] = Mm[i] * Mm[j] + Mm[3 + i] * Mm[3 + j] + Mm[6 + i] * Mm[6 + j];
    }
    {   // adj(McL) (cofactors transposed) and McL^-T = cof(McL) / det
        const double* m = mc.McL;
        const double adj[9] = { (m[4] * m[8] - m[5] * m[7]), (m[2] * m[7] - m[1] * m[8]), (m[1] * m[5] - m[2] * m[4]),
                                (m[5] * m[6] - m[3] * m[8]), (m[0] * m[8] - m[2] * m[6]), (m[2] * m[3] - m[0] * m[5]),
                                (m[3] * m[7] - m[4] * m[6]), (m[1] * m[6] - m[0] * m[7]), (m[0] * m[4] - m[1] * m[3]) };
        const double det = m[0] * adj[0] + m[1] * adj[3] + m[2] * adj[6];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) { mc.adjL[3 * i + j] = adj[3 * i + j]; mc.MiTL[3 * i + j] = adj[3 * j + i] / det; }
    }
    mc.a0 = p.n_air / p.n_glass;
    mc.a1 = p.n_air / p.n_water;
    mc.d_air = p.d_air; mc.d_glass = p.d_glass;
    mc.klim = 0.81 * mc.a1 * mc.a1 / (1.0 - mc.a1 * mc.a1);
    mc.st[0] = (float)mc.a1; mc.st[1] = (float)(mc.a1 * mc.a1); mc.st[2] = (float)(1.0 - mc.a1 * mc.a1); mc.st[3] = (float)(1.0 - mc.a0 * mc.a0);
    mc.st[4] = (float)mc.d_air; mc.st[5] = (float)(mc.d_glass * mc.a0); mc.st[6] = (float)((mc.d_air + mc.d_glass * mc.a0) / mc.a1); mc.st[7] = 0.f;
    mc.mkc = h->d_mkc;
    return mc;
}

template <typename T>
int launch_marker_pose_t(fbus_ekf_t h, int n, int geometry, const void* left, const void* right, void* pos,
                         void* quat, void* corners3d)
{
    const int ev = timing_begin(h, FBUS_KERNEL_MARKER_POSE);
    launch_marker_pose_k<T>(h->stream, n, geometry, (const T*)left, (const T*)right, (T*)pos, (T*)quat, (T*)corners3d, make_vc<double>(h));
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}

template <typename T, int N>
int init_gb_t(fbus_ekf_t h, int Tn, const void* accel, const void* gyro)
{
    launch_init_gravity_bias_k<T, N>(h->stream, (T*)h->recs, h->B, Tn, (const T*)accel, (const T*)gyro);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int do_init_gb(fbus_ekf_t h, int Tn, const void* a, const void* g) { DISPATCH2(h, init_gb_t, h, Tn, a, g); }

template <typename T, int N, int D>
int pose_init_t(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int what,
                const uint8_t* mask, void* out7)
{
    launch_pose_init_k<T, N, D>(h->stream, (T*)h->recs, h->B, M, (const int*)ids, (const T*)pos, (const T*)quat, what, h->prm.max_dist,
                                (const unsigned char*)mask, (T*)out7, h->d_applied, make_dc<T>(h));
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int do_pose_init(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int what,
                 const uint8_t* mask, void* out7)
{
    DISPATCH(h, pose_init_t, h, M, ids, pos, quat, what, mask, out7);
}

// the pixel update with the handle's and the call's pack; roles: waves per tile of the plain update
template <typename T, int N, int D>
void update_pixels(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, int roles, const uint8_t* skip,
                   const NisDst* nis)
{
    with_update_pack<T>(h, nis, nullptr, [&](auto... x) {
        launch_pixels2_k<T, N, D>(h->stream, (T*)h->recs, h->B, M, (const int*)ids, (const T*)left, (const T*)right, roles,
                                  h->prm.marker_size, h->prm.r_pix, (const unsigned char*)skip, h->d_applied, h->d_id2slot, make_mc(h), x...);
    });
}
template <typename T, int N, int D>
int launch_correct_corners_t(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, int geometry,
                             int mode, const uint8_t* skip, const NisDst* nis = nullptr)
{
    const int ev = timing_begin(h, FBUS_KERNEL_CORRECT_CORNERS);
    // triangulation and fold in double, non-cancelling update (ekf_meas.hpp); records written through (sc1) as correct_kernel's
    h->records_warm = h->warm_after_correct;
    // (the markers of a filter divided among the waves of a tile: the plain stacked update alone)
    const int roles = mode == MODE_STACKED && !nis ? team_roles_pixels(route_key(h), M) : 1;
    with_update_pack<T>(h, nis, nullptr, [&](auto... x) {
        launch_corners2_k<T, N, D>(h->stream, (T*)h->recs, h->B, M, (const int*)ids, (const T*)left, (const T*)right, geometry, mode,
                                   roles, h->prm.marker_size, h->prm.r_pos, h->prm.switch_thres, (const unsigned char*)skip,
                                   h->d_applied, h->d_id2slot, make_mc(h), make_vc<double>(h), make_vc<T>(h), x...);
    });
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}

template <typename T, int N, int D>
int launch_correct_pixels_t(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, const uint8_t* skip)
{
    const int ev = timing_begin(h, FBUS_KERNEL_CORRECT_CORNERS);
    // double-precision fold + non-cancelling update (ekf_meas.hpp), both record types, either covariance form (the form is
    // symmetric by construction and subtracts nothing on the rows the measurement shrinks: what Joseph's form is chosen for)
    h->records_warm = h->warm_after_correct;          // written through (sc1), as correct_kernel's records
    const RouteKey key = route_key(h);
    const int split = meas_split_roles(key, M);       // (0 on a tabled handle, as team_roles_pixels is 1)
    if constexpr (sizeof(T) == 4) {
        if (split > 0)
            launch_pixels_split_k<T, N, D>(h->stream, (T*)h->recs, h->B, M, (const int*)ids, (const T*)left, (const T*)right, split,
                                           h->prm.marker_size, h->prm.r_pix, (const unsigned char*)skip, h->d_applied, h->d_id2slot, make_mc(h));
    }
    if (split == 0 || sizeof(T) != 4) update_pixels<T, N, D>(h, M, ids, left, right, team_roles_pixels(key, M), skip, nullptr);
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}

int launch_correct_pixels(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, const uint8_t* skip)
{
    DISPATCH(h, launch_correct_pixels_t, h, M, ids, left, right, skip);
}

// FRAME_MEAS_RESIDENT (F = 1), WINDOW_ONE_WAVE of the measurement windows, and FRAME_TABLED_RESIDENT with F = 1 (pixel / corner rows):
// K predicts + correct_pixels (kind 0) / correct_corners (kind 1) per frame in ONE launch (frame_meas_kernel: record resident, covariance
// parked in LDS across the fold).  Equal to the per-call sequence to fp32 rounding (bit-equal: its update alone, K = 0, and a window
// to its frames).
template <typename T, int N, int D>
int launch_frame_meas_t(fbus_ekf_t h, WindowPack pack, int F, const unsigned char* kc, const void* accel, const void* gyro, const void* dt, int dt_per_filter,
                        int kind, int M, const int32_t* ids, const void* left, const void* right, int geometry, int mode, const uint8_t* skip,
                        const TrajDst* tj)
{
    const int ev = timing_begin(h, FBUS_KERNEL_FRAME, F);
    h->records_warm = h->warm_after_correct;      // written through (sc1), as the per-call updates: the next predict streams them
    const DevConst<T> dc = make_dc<T>(h);
    with_window_pack<T>(h, pack, tj, [&](auto... x) {
        launch_frame_meas_k<T, N, D>(h->stream, (T*)h->recs, h->B, F, kc, (const T*)accel, (const T*)gyro, (const T*)dt, dt_per_filter ? 1 : 0,
                                     kind, M, (const int*)ids, (const T*)left, (const T*)right, geometry, mode, h->prm.marker_size,
                                     kind == MEAS_PIXELS ? h->prm.r_pix : h->prm.r_pos, h->prm.switch_thres, (const unsigned char*)skip,
                                     h->d_applied, h->d_id2slot, make_mc(h), make_vc<double>(h), make_vc<T>(h), dc.qd, x...);
    });
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int launch_frame_meas(fbus_ekf_t h, WindowPack pack, int F, const unsigned char* kc, const void* accel, const void* gyro, const void* dt, int per, int kind,
                      int M, const int32_t* ids, const void* left, const void* right, int geometry, int mode, const uint8_t* skip,
                      const TrajDst* tj)
{
    DISPATCH_F32(h, launch_frame_meas_t, h, pack, F, kc, accel, gyro, dt, per, kind, M, ids, left, right, geometry, mode, skip, tj);
}

int launch_correct_corners(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, int geometry,
                           int mode, const uint8_t* skip, const NisDst* nis = nullptr)
{
    DISPATCH(h, launch_correct_corners_t, h, M, ids, left, right, geometry, mode, skip, nis);
}

// the pixel update with the NIS output and the gate: always the one-wave-per-tile kernel
template <typename T, int N, int D>
int launch_correct_pixels_nis_t(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, const uint8_t* skip,
                                const NisDst& nd)
{
    const int ev = timing_begin(h, FBUS_KERNEL_CORRECT_CORNERS);
    h->records_warm = h->warm_after_correct;
    update_pixels<T, N, D>(h, M, ids, left, right, 1, skip, &nd);
    timing_end(h, ev);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int launch_correct_pixels_nis(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, const uint8_t* skip,
                              const NisDst& nd)
{
    DISPATCH(h, launch_correct_pixels_nis_t, h, M, ids, left, right, skip, nd);
}
// a call whose largest possible dof has no entry in the gate table is refused (before anything is launched)
int check_gate_dof(fbus_ekf_t h, int max_dof, const char* where)
{
    if (h->gate_n > 0 && max_dof >= h->gate_n)
        return fail(h, FBUS_ERR_INVALID, std::string(where) + ": the gate table has " + std::to_string(h->gate_n) +
                                         " entries, the call can reach dof " + std::to_string(max_dof));
    return FBUS_OK;
}

// ---- argument checks: one per update -------------------------------------------------------------------------------------------
// Every form of an update (device pointers, host pointers, asynchronous, _nis) calls its check first: a refused call stages, copies,
// queues and launches nothing.  where: the entry point the messages name; nis: an _nis form (the gate table must reach the call's
// largest dof); dev: left / right are device pointers, which the kernels load 16 bytes at a time (staging memory is aligned as allocated).
int check_predict(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt)
{
    return (!h || !accel || !gyro || !dt || K < 1) ? FBUS_ERR_INVALID : FBUS_OK;
}
int check_points(fbus_ekf_t h, const void* left, const void* right, const char* where)
{
    if (points_aligned(left, right)) return FBUS_OK;
    return fail(h, FBUS_ERR_INVALID, std::string(where) + ": left / right must be 16-byte aligned device pointers");
}
int check_pose(fbus_ekf_t h, const char* where, bool nis, int M, const void* ids, const void* pos, const void* quat, int mode)
{
    if (!h || !ids || !pos || !quat || M < 1 || M > FBUS_MAX_VISIBLE) return FBUS_ERR_INVALID;
    if (!mode_ok(mode)) return FBUS_ERR_UNSUPPORTED;
    const int rows = h->prm.dialect == FBUS_DIALECT_CPP ? 7 : 3;
    return nis ? check_gate_dof(h, rows * (mode == FBUS_MODE_NEAREST ? 1 : M), where) : FBUS_OK;
}
int check_r_pix(fbus_ekf_t h) { return h->prm.r_pix > 0 ? FBUS_OK : fail(h, FBUS_ERR_INVALID, "r_pix must be positive"); }
int check_pixels(fbus_ekf_t h, const char* where, bool nis, bool dev, int M, const void* ids, const void* left, const void* right)
{
    if (!h || !ids || !left || M < 1 || M > FBUS_MAX_VISIBLE) return FBUS_ERR_INVALID;
    int rc = check_r_pix(h);
    if (rc == FBUS_OK && nis) rc = check_gate_dof(h, M * 8 * (right ? 2 : 1), where);
    if (rc == FBUS_OK && dev) rc = check_points(h, left, right, where);
    return rc;
}
// geometry and mode of corner rows; rows: the call has marker slots (a frame may have none)
int check_corner_kind(bool rows, const void* right, int geometry, int mode)
{
    if (!geometry_ok(geometry)) return FBUS_ERR_UNSUPPORTED;
    if (rows && geometry != FBUS_VIS_CORNERS3D && !right) return FBUS_ERR_INVALID;
    return mode_ok(mode) ? FBUS_OK : FBUS_ERR_UNSUPPORTED;
}
int check_corners(fbus_ekf_t h, const char* where, bool nis, bool dev, int M, const void* ids, const void* left, const void* right,
                  int geometry, int mode)
{
    if (!h || !ids || !left || M < 1 || M > FBUS_MAX_VISIBLE) return FBUS_ERR_INVALID;
    int rc = check_corner_kind(true, right, geometry, mode);
    if (rc == FBUS_OK && nis) rc = check_gate_dof(h, 12 * (mode == FBUS_MODE_NEAREST ? 1 : M), where);
    if (rc == FBUS_OK && dev) rc = check_points(h, left, right, where);
    return rc;
}

// kcount -> the window kernels' byte counts (kc, may be null) and the sample total; false when an entry lies outside 0..kmax
bool frame_counts(int nframes, const int32_t* kcount, int kmax, unsigned char* kc, size_t* total)
{
    *total = 0;
    for (int f = 0; f < nframes; ++f) {
        if (kcount[f] < 0 || kcount[f] > kmax) return false;
        if (kc) kc[f] = (unsigned char)kcount[f];
        *total += (size_t)kcount[f];
    }
    return true;
}
// The frame / window family.  A single frame is a window of one whose count K may exceed a byte (kcount = &K, kmax = INT_MAX, kc = null).
// kind: KIND_POSE (a, b = pos, quat) or FBUS_MEAS_PIXELS / FBUS_MEAS_CORNERS (a, b = left, right: device pointers); geometry and mode
// of a pixel frame are set to the values the launchers expect.  An empty window (nframes = 0) passes: the caller returns FBUS_OK.
constexpr int KIND_POSE = -1;
static_assert(KIND_POSE == ROUTE_POSE, "a frame's kind is handed to ekf_route.hpp as it is");
int check_frames(fbus_ekf_t h, const char* where, int nframes, const int32_t* kcount, int kmax, unsigned char* kc, const void* accel,
                 const void* gyro, const void* dt, int kind, int M, const void* ids, const void* a, const void* b, int& geometry,
                 int& mode, const TrajDst* tj)
{
    const bool window = kc != nullptr;
    if (!h || nframes < 0 || nframes > FBUS_MAX_WINDOW_FRAMES || M < 0 || M > FBUS_MAX_VISIBLE) return FBUS_ERR_INVALID;
    if (!window && kcount[0] < 0) return FBUS_ERR_INVALID;
    if (kind != KIND_POSE && kind != FBUS_MEAS_PIXELS && kind != FBUS_MEAS_CORNERS) return FBUS_ERR_UNSUPPORTED;
    if (nframes > 0 && !kcount) return FBUS_ERR_INVALID;
    // (a pose window tests its mode before kcount's entries, a single pose frame behind its arrays: as they always have)
    const bool pose_mode_bad = kind == KIND_POSE && !mode_ok(mode);
    if (pose_mode_bad && window) return FBUS_ERR_UNSUPPORTED;
    size_t total = 0;
    if (!frame_counts(nframes, kcount, kmax, kc, &total)) return FBUS_ERR_INVALID;
    if (total > 0 && (!accel || !gyro || !dt)) return FBUS_ERR_INVALID;
    const bool rows = M > 0 && nframes > 0;
    if (rows && (!ids || !a || (kind == KIND_POSE && !b))) return FBUS_ERR_INVALID;
    if (pose_mode_bad) return FBUS_ERR_UNSUPPORTED;
    int rc = FBUS_OK;
    if (kind == FBUS_MEAS_PIXELS) {
        rc = check_r_pix(h);
        geometry = FBUS_VIS_REFRACTIVE; mode = FBUS_MODE_STACKED;          // (not used by the pixel rows)
    } else if (kind == FBUS_MEAS_CORNERS)
        rc = check_corner_kind(rows, b, geometry, mode);
    if (rc != FBUS_OK || nframes == 0) return rc;
    // on every route, not only the resident one: the per-call updates behind the fall-back routes would meet unaligned image points AFTER
    // the predicts have run.  Every frame's arrays start a multiple of 16 bytes behind the first (B M x 32 / 48 bytes x element size)
    if (kind != KIND_POSE && M > 0 && (rc = check_points(h, a, b, where)) != FBUS_OK) return rc;
    return tj ? check_traj(h, *tj, nframes, where) : FBUS_OK;
}

int ensure_stage(fbus_ekf_t h, int slot, size_t bytes)
{
    if (bytes <= h->stage_cap[slot]) return FBUS_OK;
    if (h->stage[slot]) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipFree(h->stage[slot]));
        h->stage[slot] = nullptr;
        h->stage_cap[slot] = 0;
    }
    HIP_TRY(h, hipMalloc(&h->stage[slot], bytes));
    h->stage_cap[slot] = bytes;
    return FBUS_OK;
}

// ---- the arrays of a call, and the three ways they reach the kernels -----------------------------------------------------------------
// One array: the caller's pointer as an input (in), as an output (out) or both, its size (0: absent), and where the pointer the launch
// uses goes.  An update describes its arrays once (`*_pieces` below) and hands the description to run_pieces with the transport.
struct Piece { const void* in; void* out; size_t bytes; const void** dev; bool zero; };
Piece in_piece(const void* p, size_t bytes, const void** dev) { return { p, nullptr, p ? bytes : 0, dev, false }; }
// zero: the staged copy starts as zeros (a kernel that writes only some entries)
Piece out_piece(void* p, size_t bytes, void** dev, bool zero = false) { return { nullptr, p, p ? bytes : 0, const_cast<const void**>(dev), zero }; }
Piece inout_piece(void* p, size_t bytes, void** dev) { return { p, p, p ? bytes : 0, const_cast<const void**>(dev), false }; }

// ---- asynchronous host-pointer calls ---------------------------------------------------------------------------------
// The reference's caller hands one IMU sample at a time to a filter thread and returns at once (FILTER::SetImuData under a mutex,
// filter.cpp:24-55; BatchImuProcessing issues one predict per sample, :505-516).  The synchronous host-pointer entry points stage
// pageable memory and wait for the kernel (103 us per predict at 65 536 filters); these do not wait:
//   * every input array is taken BY VALUE at the call: pageable memory is copied into a pinned ring slot by the calling thread
//     (the caller's buffer is free again on return), pinned memory (hipHostMalloc / hipHostRegister / fbus_ekf_host_register) is
//     DMA'd in place (it must stay unchanged until fbus_ekf_async_inputs_consumed / fbus_ekf_sync);
//   * the H2D copy runs on a copy stream of the handle's, the kernel on the handle's stream behind an event: the copy of call i + 1
//     overlaps the kernel of call i;
//   * a slot is reused after ASYNC_SLOTS calls; the call then waits for THAT slot's kernel only (back-pressure, counted).
// Completion and device-side errors: fbus_ekf_sync, or any host-pointer result (fbus_ekf_get_state, fbus_ekf_get_applied).
bool host_ptr_is_pinned(const void* p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (an ordinary malloc'ed pointer)
    return at.type == hipMemoryTypeHost;
}

// (input pieces only: no asynchronous form has outputs)
int async_begin(fbus_ekf_t h, Piece* pieces, int n, fbus_ekf::AsyncSlot** out)
{
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "the asynchronous host-pointer calls cannot be captured into a graph (use the _dev entry points)");
    if (!h->copy_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    fbus_ekf::AsyncSlot& a = h->aring[h->anext++ % fbus_ekf::ASYNC_SLOTS];
    if (!a.copied) {
        HIP_TRY(h, hipEventCreateWithFlags(&a.copied, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&a.done, hipEventDisableTiming));
    }
    ++h->async_calls;
    if (a.busy) {                                   // the kernel that read this slot ASYNC_SLOTS calls ago
        if (hipEventQuery(a.done) != hipSuccess) { ++h->async_waits; HIP_TRY(h, hipEventSynchronize(a.done)); }
        a.busy = false;
    }
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (pieces[i].bytes + 255) & ~(size_t)255;
    if (total > a.cap) {
        if (a.host) HIP_TRY(h, hipHostFree(a.host));
        if (a.dev) HIP_TRY(h, hipFree(a.dev));
        a.host = a.dev = nullptr; a.cap = 0;
        const size_t cap = (total + (total >> 2) + 65535) & ~(size_t)65535;
        HIP_TRY(h, hipHostMalloc(&a.host, cap, hipHostMallocDefault));
        HIP_TRY(h, hipMalloc(&a.dev, cap));
        a.cap = cap;
    }
    // staged pieces first (one contiguous range -> ONE copy), then the pinned ones in place
    size_t off = 0, staged_end = 0;
    bool direct[8] = { false, false, false, false, false, false, false, false };
    for (int i = 0; i < n; ++i) {
        *pieces[i].dev = nullptr;
        if (!pieces[i].in || pieces[i].bytes == 0) continue;
        direct[i] = pieces[i].bytes >= 4096 && host_ptr_is_pinned(pieces[i].in);
        if (direct[i]) continue;
        std::memcpy((char*)a.host + off, pieces[i].in, pieces[i].bytes);
        *pieces[i].dev = (char*)a.dev + off;
        off += (pieces[i].bytes + 255) & ~(size_t)255;
        staged_end = off;
    }
    if (staged_end) HIP_TRY(h, hipMemcpyAsync(a.dev, a.host, staged_end, hipMemcpyHostToDevice, h->copy_stream));
    for (int i = 0; i < n; ++i) {
        if (!direct[i]) continue;
        HIP_TRY(h, hipMemcpyAsync((char*)a.dev + off, pieces[i].in, pieces[i].bytes, hipMemcpyHostToDevice, h->copy_stream));
        *pieces[i].dev = (char*)a.dev + off;
        off += (pieces[i].bytes + 255) & ~(size_t)255;
        ++h->async_direct;
    }
    HIP_TRY(h, hipEventRecord(a.copied, h->copy_stream));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, a.copied, 0));
    *out = &a;
    return FBUS_OK;
}

int async_end(fbus_ekf_t h, fbus_ekf::AsyncSlot* a, int rc)
{
    // (also behind a failed launch: the slot's memory must not be rewritten while the stream may still read it)
    HIP_TRY(h, hipEventRecord(a->done, h->stream));
    a->busy = true;
    return rc;
}

// DEV: the caller's pointers are device pointers and the launch takes them as they are.  STAGED: piece i goes through staging slot i
// (inputs copied in, outputs copied back) and the call returns when the stream has drained -- the staging buffers and the caller's
// arrays are free again.  ASYNC: the inputs go through the pinned ring and nothing waits.  `go` launches with the pieces' device pointers.
enum Transport { DEV, STAGED, ASYNC };
template <typename GO>
int run_pieces(fbus_ekf_t h, Transport t, Piece* pc, int n, GO go)
{
    if (t == DEV) {
        for (int i = 0; i < n; ++i) *pc[i].dev = pc[i].in ? pc[i].in : pc[i].out;
        return go();
    }
    int rc;
    if (t == ASYNC) {
        fbus_ekf::AsyncSlot* a;
        if ((rc = async_begin(h, pc, n, &a)) != FBUS_OK) return rc;
        return async_end(h, a, go());
    }
    for (int i = 0; i < n; ++i) {
        *pc[i].dev = nullptr;
        if (pc[i].bytes == 0) continue;
        if ((rc = ensure_stage(h, i, pc[i].bytes)) != FBUS_OK) return rc;
        if (pc[i].in) HIP_TRY(h, hipMemcpyAsync(h->stage[i], pc[i].in, pc[i].bytes, hipMemcpyHostToDevice, h->stream));
        else if (pc[i].zero) HIP_TRY(h, hipMemsetAsync(h->stage[i], 0, pc[i].bytes, h->stream));
        *pc[i].dev = h->stage[i];
    }
    if ((rc = go()) != FBUS_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (pc[i].out && pc[i].bytes) HIP_TRY(h, hipMemcpyAsync(pc[i].out, h->stage[i], pc[i].bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // the staging buffers are reused by the next host call, the host arrays by the caller
    return FBUS_OK;
}

size_t record_elems(int dtype, int N)
{
    if (dtype == 32) return N == 18 ? Rec<float, 18>::NRECP : Rec<float, 15>::NRECP;
    return N == 18 ? Rec<double, 18>::NRECP : Rec<double, 15>::NRECP;
}

// ---- the updates: check, describe the arrays, run through the transport ---------------------------------------------------------------
int predict_any(fbus_ekf_t h, Transport t, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter)
{
    DeviceGuard guard_(h);
    const int rc = check_predict(h, K, accel, gyro, dt);
    if (rc != FBUS_OK) return rc;
    const size_t es = esize(h), B = (size_t)h->B;
    const void *da, *dg, *dd;
    Piece pc[3] = { in_piece(accel, (size_t)K * B * 3 * es, &da), in_piece(gyro, (size_t)K * B * 3 * es, &dg),
                    in_piece(dt, (size_t)K * (dt_per_filter ? B : 1) * es, &dd) };
    return run_pieces(h, t, pc, 3, [&] { return launch_predict(h, K, da, dg, dd, dt_per_filter); });
}

// The arrays of a measurement update on the device: ids [B][M], a / b [B][M][wa / wb] in the record type (pos, quat: 3, 4; left, right:
// 8 or 12, 8), skip [B], and an _nis form's outputs nis [B] in the record type, dof [B].  Absent arrays (b, skip, nis, dof; b_unused:
// `right` beside corner positions, which the device forms hand on as it is) take no bytes.
struct RowsDev { const void *ids, *a, *b, *skip; void *nis, *dof; };
void rows_pieces(const fbus_ekf* h, Piece* pc, RowsDev& d, int M, const void* ids, const void* a, size_t wa, const void* b, size_t wb,
                 bool b_unused, const void* skip, void* nis, int32_t* dof)
{
    const size_t es = esize(h), BM = (size_t)h->B * M;
    pc[0] = in_piece(ids, BM * sizeof(int32_t), &d.ids);
    pc[1] = in_piece(a, BM * wa * es, &d.a);
    pc[2] = in_piece(b, b_unused ? 0 : BM * wb * es, &d.b);
    pc[3] = in_piece(skip, (size_t)h->B, &d.skip);
    pc[4] = out_piece(nis, (size_t)h->B * es, &d.nis);
    pc[5] = out_piece(dof, (size_t)h->B * sizeof(int32_t), &d.dof);
}
// nis: an _nis form (its outputs may still be null)
int correct_any(fbus_ekf_t h, Transport t, bool nis, int M, const int32_t* ids, const void* pos, const void* quat, int mode,
                const uint8_t* skip, void* out_nis, int32_t* out_dof)
{
    DeviceGuard guard_(h);
    const int rc = check_pose(h, "fbus_ekf_correct_nis", nis, M, ids, pos, quat, mode);
    if (rc != FBUS_OK) return rc;
    Piece pc[6];
    RowsDev d;
    rows_pieces(h, pc, d, M, ids, pos, 3, quat, 4, false, skip, out_nis, out_dof);
    return run_pieces(h, t, pc, 6, [&] {
        const NisDst nd{ d.nis, (int32_t*)d.dof };
        return launch_correct(h, M, (const int32_t*)d.ids, d.a, d.b, mode, (const uint8_t*)d.skip, nis ? &nd : nullptr);
    });
}
int correct_pixels_any(fbus_ekf_t h, Transport t, bool nis, int M, const int32_t* ids, const void* left, const void* right,
                       const uint8_t* skip, void* out_nis, int32_t* out_dof)
{
    DeviceGuard guard_(h);
    const int rc = check_pixels(h, nis ? "fbus_ekf_correct_pixels_nis" : "fbus_ekf_correct_pixels", nis, t == DEV, M, ids, left, right);
    if (rc != FBUS_OK) return rc;
    Piece pc[6];
    RowsDev d;
    rows_pieces(h, pc, d, M, ids, left, 8, right, 8, false, skip, out_nis, out_dof);
    return run_pieces(h, t, pc, 6, [&] {
        const NisDst nd{ d.nis, (int32_t*)d.dof };
        return nis ? launch_correct_pixels_nis(h, M, (const int32_t*)d.ids, d.a, d.b, (const uint8_t*)d.skip, nd)
                   : launch_correct_pixels(h, M, (const int32_t*)d.ids, d.a, d.b, (const uint8_t*)d.skip);
    });
}
int correct_corners_any(fbus_ekf_t h, Transport t, bool nis, int M, const int32_t* ids, const void* left, const void* right,
                        int geometry, int mode, const uint8_t* skip, void* out_nis, int32_t* out_dof)
{
    DeviceGuard guard_(h);
    const int rc = check_corners(h, nis ? "fbus_ekf_correct_corners_nis" : "fbus_ekf_correct_corners", nis, t == DEV, M, ids, left, right,
                                 geometry, mode);
    if (rc != FBUS_OK) return rc;
    const bool c3d = geometry == FBUS_VIS_CORNERS3D;
    Piece pc[6];
    RowsDev d;
    rows_pieces(h, pc, d, M, ids, left, c3d ? 12 : 8, right, 8, c3d, skip, out_nis, out_dof);
    return run_pieces(h, t, pc, 6, [&] {
        const NisDst nd{ d.nis, (int32_t*)d.dof };
        return launch_correct_corners(h, M, (const int32_t*)d.ids, d.a, d.b, geometry, mode, (const uint8_t*)d.skip, nis ? &nd : nullptr);
    });
}

// ---- frames and windows ------------------------------------------------------------------------------------------------------------------
// The device arrays of a frame or of a window: IMU samples [samples][B][3], dt [samples] or [samples][B]; per frame ids [B][M],
// a / b [B][M][wa / wb] (pos, quat: 3, 4; left, right: 8 or 12, 8), skip [B]
struct FrameArrays { const void *accel, *gyro, *dt; int per, M; const int32_t* ids; const void *a, *b; size_t wa, wb; const uint8_t* skip; };
// frame f of a window whose frames 0 .. f - 1 hold k0 samples (f = 0: the arrays from sample k0 on)
FrameArrays frame_slice(const fbus_ekf* h, const FrameArrays& w, size_t k0, int f)
{
    const size_t es = esize(h), B = (size_t)h->B, fBM = (size_t)f * B * w.M;
    const auto at = [](const void* p, size_t bytes) { return p ? (const void*)((const char*)p + bytes) : nullptr; };
    FrameArrays s = w;
    s.accel = at(w.accel, k0 * B * 3 * es);
    s.gyro = at(w.gyro, k0 * B * 3 * es);
    s.dt = at(w.dt, k0 * (w.per ? B : 1) * es);
    s.ids = (const int32_t*)at(w.ids, fBM * sizeof(int32_t));
    s.a = at(w.a, fBM * w.wa * es);
    s.b = at(w.b, fBM * w.wb * es);
    s.skip = (const uint8_t*)at(w.skip, (size_t)f * B);
    return s;
}

// One camera frame: its route asked (frame_route), then the route's launches.  kind: KIND_POSE (s.a, s.b = pos, quat) or FBUS_MEAS_PIXELS / FBUS_MEAS_CORNERS (left, right)
int run_frame(fbus_ekf_t h, const RouteKey& key, int kind, int K, const FrameArrays& s, int geometry, int mode)
{
    const FrameRoute route = frame_route(key, (RouteKind)kind, mode, s.M, K);
    const WindowPack pack = window_pack(key, false);
    const unsigned char kc1 = (unsigned char)K;       // (the routes that count in a byte are chosen for K <= 255 only)
    switch (route) {
        case FRAME_PER_CALL: {
            int rc = FBUS_OK;
            if (K > 0) rc = launch_predict(h, K, s.accel, s.gyro, s.dt, s.per);
            if (rc != FBUS_OK || s.M == 0) return rc;
            if (kind == KIND_POSE) return launch_correct(h, s.M, s.ids, s.a, s.b, mode, s.skip);
            return kind == FBUS_MEAS_PIXELS ? launch_correct_pixels(h, s.M, s.ids, s.a, s.b, s.skip)
                                            : launch_correct_corners(h, s.M, s.ids, s.a, s.b, geometry, mode, s.skip);
        }
        case FRAME_F64_FUSED:
        case FRAME_FUSED: return launch_frame(h, K, s.accel, s.gyro, s.dt, s.per, s.M, s.ids, s.a, s.b, mode, s.skip);
        case FRAME_TEAM: return launch_frames_team(h, 1, &kc1, s.accel, s.gyro, s.dt, s.per, s.M, s.ids, s.a, s.b, mode, s.skip);
        case FRAME_TABLED_RESIDENT:
            if (kind == KIND_POSE) return launch_frames(h, pack, 1, &kc1, s.accel, s.gyro, s.dt, s.per, s.M, s.ids, s.a, s.b, mode, s.skip, nullptr);
            [[fallthrough]];
        case FRAME_MEAS_RESIDENT:
            return launch_frame_meas(h, pack, 1, &kc1, s.accel, s.gyro, s.dt, s.per, kind, s.M, s.ids, s.a, s.b, geometry, mode, s.skip, nullptr);
    }
    return FBUS_ERR_INVALID;
}
// A window frame by frame (WINDOW_BY_FRAME, WINDOW_TEAM_FRAMES): every frame on its own route, its trajectory rows by the snapshot kernel.
// kcount: nframes counts, each the K of its frame (a single frame's may exceed a byte)
int run_frames(fbus_ekf_t h, const RouteKey& key, int kind, int nframes, const int32_t* kcount, const FrameArrays& w, int geometry, int mode,
               const TrajDst* tj)
{
    size_t k0 = 0;
    for (int f = 0; f < nframes; ++f) {
        const int K = kcount[f];
        int rc = run_frame(h, key, kind, K, frame_slice(h, w, k0, f), geometry, mode);
        if (rc == FBUS_OK && tj) rc = snapshot_row(h, *tj, f);
        if (rc != FBUS_OK) return rc;
        k0 += (size_t)K;
    }
    return FBUS_OK;
}

// fbus_ekf_frame_dev (fused = false: K predict launches + one correct launch) and fbus_ekf_frame_fused_dev
int frame_any(fbus_ekf_t h, bool fused, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter, int M,
              const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip)
{
    DeviceGuard guard_(h);
    // everything is validated before the first launch: a rejected call must not leave the state advanced by the K predicts
    int geometry = 0;
    int rc = check_frames(h, fused ? "fbus_ekf_frame_fused_dev" : "fbus_ekf_frame_dev", 1, &K, std::numeric_limits<int>::max(), nullptr, accel, gyro, dt, KIND_POSE, M, ids, pos, quat,
                          geometry, mode, nullptr);
    if (rc != FBUS_OK) return rc;
    const FrameArrays w{ accel, gyro, dt, dt_per_filter, M, ids, pos, quat, 3, 4, skip };
    if (fused) return run_frame(h, route_key(h), KIND_POSE, K, w, geometry, mode);
    // one event pair around the whole run of K back-to-back predict launches: a pair per launch
    // would cost ~8 us of stream time each and read ~3 us long; duration / K is the per-launch time
    const bool sampled = (h->frame_count++ % h->timing_stride) == 0;
    const int ev = (K > 0 && sampled) ? timing_begin(h, FBUS_KERNEL_PREDICT, K) : -1;
    h->timing_suspended = true;
    for (int k = 0; k < K && rc == FBUS_OK; ++k) {
        const FrameArrays s = frame_slice(h, w, (size_t)k, 0);
        rc = launch_predict(h, 1, s.accel, s.gyro, s.dt, dt_per_filter);
    }
    timing_end(h, ev);
    if (rc != FBUS_OK) { h->timing_suspended = false; return rc; }
    h->timing_suspended = !sampled;
    if (M > 0) rc = launch_correct(h, M, ids, pos, quat, mode, skip);
    h->timing_suspended = false;
    return rc;
}

// fbus_ekf_frames_fused_dev (tj = null) and fbus_ekf_frames_fused_traj_dev
int frames_any(fbus_ekf_t h, const char* where, int nframes, const int32_t* kcount, const void* accel, const void* gyro, const void* dt,
               int dt_per_filter, int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip,
               const TrajDst* tj)
{
    DeviceGuard guard_(h);
    unsigned char kc[FBUS_MAX_WINDOW_FRAMES];
    int geometry = 0;
    int rc = check_frames(h, where, nframes, kcount, 255, kc, accel, gyro, dt, KIND_POSE, M, ids, pos, quat, geometry, mode, tj);
    if (rc != FBUS_OK || nframes == 0) return rc;
    const RouteKey key = route_key(h);
    switch (window_route(key, ROUTE_POSE, mode, M, tj != nullptr)) {
        case WINDOW_ONE_WAVE:
            return launch_frames(h, window_pack(key, tj != nullptr), nframes, kc, accel, gyro, dt, dt_per_filter, M, ids, pos, quat, mode, skip, tj);
        case WINDOW_TEAM: return launch_frames_team(h, nframes, kc, accel, gyro, dt, dt_per_filter, M, ids, pos, quat, mode, skip);
        case WINDOW_TEAM_FRAMES:        // (every frame's route is then FRAME_TEAM)
        case WINDOW_BY_FRAME: break;
    }
    const FrameArrays w{ accel, gyro, dt, dt_per_filter, M, ids, pos, quat, 3, 4, skip };
    return run_frames(h, key, KIND_POSE, nframes, kcount, w, geometry, mode, tj);
}

// fbus_ekf_frame_meas_fused_dev (kcount = &K, nframes = 1, single = true: K may exceed a byte), fbus_ekf_frames_meas_fused_dev (tj = null)
// and fbus_ekf_frames_meas_fused_traj_dev: one validation, one choice of route
int frames_meas_any(fbus_ekf_t h, const char* where, bool single, int nframes, const int32_t* kcount, const void* accel, const void* gyro,
                    const void* dt, int dt_per_filter, int kind, int M, const int32_t* ids, const void* left, const void* right,
                    int geometry, int mode, const uint8_t* skip, const TrajDst* tj)
{
    DeviceGuard guard_(h);
    // everything is validated before the first launch: a rejected call must not leave the state advanced by the predicts
    unsigned char kc[FBUS_MAX_WINDOW_FRAMES];
    int rc = check_frames(h, where, nframes, kcount, single ? std::numeric_limits<int>::max() : 255, single ? nullptr : kc, accel, gyro,
                          dt, kind, M, ids, left, right, geometry, mode, tj);
    if (rc != FBUS_OK || nframes == 0) return rc;
    // a single frame, and a window of one, run as that frame; a longer window in one launch where its frames take a resident kernel,
    // elsewhere frame by frame through the frame's routes -- the same arithmetic
    const RouteKey key = route_key(h);
    switch (nframes > 1 ? window_route(key, (RouteKind)kind, mode, M, tj != nullptr) : WINDOW_BY_FRAME) {
        case WINDOW_ONE_WAVE:
            return launch_frame_meas(h, window_pack(key, tj != nullptr), nframes, kc, accel, gyro, dt, dt_per_filter, kind, M, ids, left, right,
                                     geometry, mode, skip, tj);
        case WINDOW_TEAM:               // (never chosen for pixel / corner rows: their frames have no team route)
        case WINDOW_TEAM_FRAMES:
        case WINDOW_BY_FRAME: break;
    }
    const bool c3d = kind == FBUS_MEAS_CORNERS && geometry == FBUS_VIS_CORNERS3D;
    const FrameArrays w{ accel, gyro, dt, dt_per_filter, M, ids, left, right, c3d ? (size_t)12 : (size_t)8, 8, skip };
    return run_frames(h, key, kind, nframes, kcount, w, geometry, mode, tj);
}

// ---- the element-wise entry points --------------------------------------------------------------------------------------------------------
int marker_pose_any(fbus_ekf_t h, Transport t, int n, int geometry, const void* left, const void* right, void* pos, void* quat,
                    void* corners3d)
{
    DeviceGuard guard_(h);
    if (!h || n < 1 || !left || !pos || !quat) return FBUS_ERR_INVALID;
    if (!geometry_ok(geometry)) return FBUS_ERR_UNSUPPORTED;
    const bool c3d = geometry == FBUS_VIS_CORNERS3D;
    if (!c3d && !right) return FBUS_ERR_INVALID;
    const size_t es = esize(h), nn = (size_t)n;
    const void *dl, *dr;
    void *dp, *dq, *dc;
    Piece pc[5] = { in_piece(left, nn * (c3d ? 12 : 8) * es, &dl), in_piece(right, c3d ? 0 : nn * 8 * es, &dr),
                    out_piece(pos, nn * 3 * es, &dp), out_piece(quat, nn * 4 * es, &dq), out_piece(corners3d, nn * 12 * es, &dc) };
    return run_pieces(h, t, pc, 5, [&] {
        return h->dtype == 32 ? launch_marker_pose_t<float>(h, n, geometry, dl, dr, dp, dq, dc)
                              : launch_marker_pose_t<double>(h, n, geometry, dl, dr, dp, dq, dc);
    });
}

int init_gravity_bias_any(fbus_ekf_t h, Transport t, int T, const void* accel, const void* gyro)
{
    DeviceGuard guard_(h);
    if (!h || T < 1 || !accel || !gyro) return FBUS_ERR_INVALID;
    const size_t bytes = (size_t)T * h->B * 3 * esize(h);
    const void *da, *dg;
    Piece pc[2] = { in_piece(accel, bytes, &da), in_piece(gyro, bytes, &dg) };
    return run_pieces(h, t, pc, 2, [&] { return do_init_gb(h, T, da, dg); });
}

// fbus_ekf_pose_init (what = FBUS_POSE_INIT / FBUS_POSE_RESET) and fbus_ekf_vision_only_pose (what = POSE_VISION: out_pose [B][7], the
// state is not touched; the kernel writes the filters that see a marker, the staged copy starts as zeros)
constexpr int POSE_VISION = 2;
int pose_init_any(fbus_ekf_t h, Transport t, int M, const int32_t* ids, const void* pos, const void* quat, int what, const uint8_t* mask,
                  void* out_pose)
{
    DeviceGuard guard_(h);
    if (!h || !ids || !pos || !quat || M < 1 || M > FBUS_MAX_VISIBLE) return FBUS_ERR_INVALID;
    if (what == POSE_VISION ? !out_pose : (what != FBUS_POSE_INIT && what != FBUS_POSE_RESET)) return FBUS_ERR_INVALID;
    const size_t es = esize(h), B = (size_t)h->B;
    RowsDev d;
    Piece pc[6];
    rows_pieces(h, pc, d, M, ids, pos, 3, quat, 4, false, mask, nullptr, nullptr);
    void* dout;
    pc[4] = out_piece(out_pose, B * 7 * es, &dout, true);         // (in the place of the nis output, which this call does not have)
    return run_pieces(h, t, pc, 5, [&] { return do_pose_init(h, M, (const int32_t*)d.ids, d.a, d.b, what, (const uint8_t*)d.skip, dout); });
}

int imu_ema_any(fbus_ekf_t h, Transport t, int T, void* accel, void* gyro, int restart)
{
    DeviceGuard guard_(h);
    if (!h || T < 0 || (T > 0 && (!accel || !gyro))) return FBUS_ERR_INVALID;
    if (!h->d_ema_carry) HIP_TRY(h, hipMalloc(&h->d_ema_carry, (size_t)h->B * 6 * esize(h)));
    if (restart) h->ema_has_carry = false;
    if (T == 0) return FBUS_OK;
    const size_t bytes = (size_t)T * h->B * 3 * esize(h);
    void *da, *dg;
    Piece pc[2] = { inout_piece(accel, bytes, &da), inout_piece(gyro, bytes, &dg) };
    return run_pieces(h, t, pc, 2, [&] {
        if (h->dtype == 32)
            launch_imu_ema_k<float>(h->stream, h->B, T, (float*)da, (float*)dg, (float*)h->d_ema_carry, h->ema_has_carry ? 1 : 0);
        else
            launch_imu_ema_k<double>(h->stream, h->B, T, (double*)da, (double*)dg, (double*)h->d_ema_carry, h->ema_has_carry ? 1 : 0);
        HIP_TRY(h, hipGetLastError());
        h->ema_has_carry = true;
        return (int)FBUS_OK;
    });
}

// ---- hypothesis groups: fbus_ekf_group_fuse / _collapse / _mix, host and device forms ----------------------------------------------------------
int check_group(fbus_ekf_t h, const char* where, int G)
{
    if (!h) return FBUS_ERR_INVALID;
    if (G < 2 || G > FBUS_GROUP_MAX)
        return fail(h, FBUS_ERR_INVALID, std::string(where) + ": G = " + std::to_string(G) + " outside 2.." + std::to_string(FBUS_GROUP_MAX));
    if (h->B % G != 0)
        return fail(h, FBUS_ERR_INVALID, std::string(where) + ": the batch of " + std::to_string(h->B) + " is not a multiple of G = " + std::to_string(G));
    return FBUS_OK;
}
// One wrapper for the calls that read the records and report on them, or rewrite them group by group: fbus_ekf_group_fuse / _collapse /
// _mix, fbus_ekf_nees and fbus_ekf_sample, each also _dev.  (the order of the tests is part of the interface: include/fbus_ekf.h)
// A caller returns on a NULL handle, takes its name from report_name, runs its own tests (check_group, required pointers, ranges),
// describes its arrays and ends in report_any, which tests in this order: _dev, an output piece inside the records; host form, a
// capture in progress, then `inspect` -- what only the host form can look at; only_reads, no output asked for: nothing to do.
std::string report_name(const char* stem, Transport t) { return std::string("fbus_ekf_") + stem + (t == DEV ? "_dev" : ""); }
template <typename INSPECT, typename GO>
int report_any(fbus_ekf_t h, Transport t, const std::string& where, bool only_reads, Piece* pc, int n, INSPECT inspect, GO go)
{
    DeviceGuard guard_(h);
    bool any_out = false;
    for (int i = 0; i < n; ++i) {
        any_out = any_out || pc[i].out;
        if (t == DEV && pc[i].out && in_records(h, pc[i].out, pc[i].bytes))     // (staged outputs are the handle's own buffers)
            return fail(h, FBUS_ERR_INVALID, where + ": an output overlaps the records");
    }
    if (t != DEV) {
        if (h->capturing) return fail(h, FBUS_ERR_INVALID, where + ": not between graph_begin and graph_end");
        const int rc = inspect();
        if (rc != FBUS_OK) return rc;
    }
    if (only_reads && !any_out) return FBUS_OK;
    return run_pieces(h, t, pc, n, go);
}
template <typename GO>
int report_any(fbus_ekf_t h, Transport t, const std::string& where, bool only_reads, Piece* pc, int n, GO go)
{
    return report_any(h, t, where, only_reads, pc, n, [] { return (int)FBUS_OK; }, go);
}

int group_fuse_any(fbus_ekf_t h, Transport t, int G, const double* logw, double* weight, int32_t* best, void* nominal, void* P, void* pdiag)
{
    const std::string where = report_name("group_fuse", t);
    const int rc = check_group(h, where.c_str(), G);
    if (rc != FBUS_OK) return rc;
    if (!logw && !h->d_lik) return fail(h, FBUS_ERR_INVALID, where + ": logw is NULL and fbus_ekf_loglik_enable(h, 1) has not been called");
    const size_t es = esize(h), B = (size_t)h->B, NG = B / G, N = (size_t)h->N;
    const void* dl;
    void *dw, *db, *dn, *dP, *dd;
    Piece pc[6] = { in_piece(logw, B * sizeof(double), &dl), out_piece(weight, B * sizeof(double), &dw),
                    out_piece(best, NG * sizeof(int32_t), &db), out_piece(nominal, NG * 19 * es, &dn),
                    out_piece(P, NG * N * N * es, &dP), out_piece(pdiag, NG * N * es, &dd) };
    return report_any(h, t, where, true, pc, 6, [&] {
        return do_group_fuse(h, G, dl ? (const double*)dl : h->d_lik, (double*)dw, (int32_t*)db, dn, dP, dd);
    });
}
int group_collapse_any(fbus_ekf_t h, Transport t, int G, const int32_t* src)
{
    const std::string where = report_name("group_collapse", t);
    const int rc = check_group(h, where.c_str(), G);
    if (rc != FBUS_OK) return rc;
    if (!src) return fail(h, FBUS_ERR_INVALID, where + ": src is NULL");
    const size_t NG = (size_t)h->B / G;
    const auto members = [&] {
        for (size_t j = 0; j < NG; ++j)
            if (src[j] >= G)
                return fail(h, FBUS_ERR_INVALID, where + ": src[" + std::to_string(j) + "] = " + std::to_string(src[j]) +
                                                 " is not a member of a group of " + std::to_string(G) + " (negative: skip the group)");
        return (int)FBUS_OK;
    };
    const void* ds;
    Piece pc[1] = { in_piece(src, NG * sizeof(int32_t), &ds) };
    return report_any(h, t, where, false, pc, 1, members, [&] { return do_group_collapse(h, G, (const int32_t*)ds); });
}
int group_mix_any(fbus_ekf_t h, Transport t, int G, const double* logw, const double* trans, double* weight, double* logc)
{
    const std::string where = report_name("group_mix", t);
    const int rc = check_group(h, where.c_str(), G);
    if (rc != FBUS_OK) return rc;
    if (!trans) return fail(h, FBUS_ERR_INVALID, where + ": trans is NULL");
    if (!logw && !h->d_lik) return fail(h, FBUS_ERR_INVALID, where + ": logw is NULL and fbus_ekf_loglik_enable(h, 1) has not been called");
    const auto stochastic = [&] {
        for (int i = 0; i < G; ++i) {
            double s = 0.0;
            for (int j = 0; j < G; ++j) {
                const double v = trans[i * G + j];
                if (!std::isfinite(v) || v < 0.0)
                    return fail(h, FBUS_ERR_INVALID, where + ": trans row " + std::to_string(i) + " column " + std::to_string(j) + " = " +
                                                     std::to_string(v) + " is not a probability");
                s += v;
            }
            if (std::fabs(s - 1.0) > 1e-9)
                return fail(h, FBUS_ERR_INVALID, where + ": trans row " + std::to_string(i) + " sums to " + std::to_string(s) + ", not to 1");
        }
        return (int)FBUS_OK;
    };
    const size_t B = (size_t)h->B;
    const void *dl, *dt;
    void *dw, *dc;
    Piece pc[4] = { in_piece(logw, B * sizeof(double), &dl), in_piece(trans, (size_t)G * G * sizeof(double), &dt),
                    out_piece(weight, B * sizeof(double), &dw), out_piece(logc, B * sizeof(double), &dc) };
    // (in place: runs with both outputs NULL)
    return report_any(h, t, where, false, pc, 4, stochastic, [&] {
        return do_group_mix(h, G, dl ? (const double*)dl : h->d_lik, (const double*)dt, (double*)dw, (double*)dc);
    });
}

// ---- the streamed sensor updates: fbus_ekf_correct_depth / _velocity / _rows, each also _dev, _nis and _nis_dev; depth and velocity _async --
// One argument check and one transport for the three.  (the order of the tests is part of the interface: include/fbus_ekf.h)
struct SensorCall {
    const char* stem;                   // the entry point the messages name: fbus_ekf_correct_<stem> + _async, or [_nis][_dev]
    bool ready;                         // the update's own precondition, tested first, and what is said when it fails
    const char* not_ready;
    bool have;                          // the arrays that must not be NULL are there, and what is said when one is not
    const char* missing;
    int rows;                           // variances per filter
    bool gated;                         // every form is gated: the table must reach dof `rows`
};
// nis: an _nis form (its outputs may still be null); in: the update's own input pieces, in front of var, skip, nis and dof;
// go(SensorDev): the launch
template <typename GO>
int sensor_any(fbus_ekf_t h, Transport t, bool nis, const SensorCall& c, const Piece* in, int n_in, const double* var, int var_per_filter,
               const uint8_t* skip, void* out_nis, int32_t* out_dof, GO go)
{
    DeviceGuard guard_(h);
    const auto where = [&] {            // (put together only where it is said)
        return std::string("fbus_ekf_correct_") + c.stem +
               (t == ASYNC ? "_async" : nis ? (t == DEV ? "_nis_dev" : "_nis") : (t == DEV ? "_dev" : ""));
    };
    if (!c.ready) return fail(h, FBUS_ERR_INVALID, where() + ": " + c.not_ready);
    if (!c.have) return fail(h, FBUS_ERR_INVALID, where() + ": " + c.missing);
    if (var_per_filter != 0 && var_per_filter != 1) return fail(h, FBUS_ERR_INVALID, where() + ": var_per_filter must be 0 or 1");
    if (c.gated) {
        const int rc = check_gate_dof(h, c.rows, where().c_str());
        if (rc != FBUS_OK) return rc;
    }
    if (t == STAGED && h->capturing) return fail(h, FBUS_ERR_INVALID, where() + ": not between graph_begin and graph_end");
    const size_t B = (size_t)h->B;
    const void *dv, *ds;
    void *dn, *dd;
    Piece pc[6];
    std::copy(in, in + n_in, pc);
    pc[n_in] = in_piece(var, (var_per_filter ? B : 1) * c.rows * sizeof(double), &dv);
    pc[n_in + 1] = in_piece(skip, B, &ds);
    pc[n_in + 2] = out_piece(out_nis, B * esize(h), &dn);
    pc[n_in + 3] = out_piece(out_dof, B * sizeof(int32_t), &dd);
    return run_pieces(h, t, pc, n_in + 4, [&] {
        return go(SensorDev{ (const double*)dv, var_per_filter ? 1 : 0, (const unsigned char*)ds, dn, (int*)dd });
    });
}
int depth_any(fbus_ekf_t h, Transport t, bool nis, const void* z, const double* var, int var_per_filter, const uint8_t* skip,
              void* out_nis, int32_t* out_dof)
{
    if (!h) return FBUS_ERR_INVALID;
    const void* dz;
    const Piece in[1] = { in_piece(z, (size_t)h->B * esize(h), &dz) };
    const SensorCall c{ "depth", h->depth_set, "fbus_ekf_set_depth_sensor has not been called", z && var, "z and var must not be NULL", 1, false };
    return sensor_any(h, t, nis, c, in, 1, var, var_per_filter, skip, out_nis, out_dof,
                      [&](const SensorDev& d) { return launch_depth(h, dz, d); });
}
int velocity_any(fbus_ekf_t h, Transport t, bool nis, const void* z, const void* gyro, const double* var, int var_per_filter,
                 const uint8_t* skip, void* out_nis, int32_t* out_dof)
{
    if (!h) return FBUS_ERR_INVALID;
    const void *dz, *dg;
    const size_t bytes = (size_t)h->B * 3 * esize(h);
    const Piece in[2] = { in_piece(z, bytes, &dz), in_piece(gyro, bytes, &dg) };
    const SensorCall c{ "velocity", h->velocity_set, "fbus_ekf_set_velocity_sensor has not been called", z && var, "z and var must not be NULL", 3, false };
    return sensor_any(h, t, nis, c, in, 2, var, var_per_filter, skip, out_nis, out_dof,
                      [&](const SensorDev& d) { return launch_velocity(h, dz, dg, d); });
}
// (no _async form)
int rows_any(fbus_ekf_t h, Transport t, bool nis, int m, const void* res, const void* H, const double* var, int var_per_filter,
             const uint8_t* skip, void* out_nis, int32_t* out_dof)
{
    if (!h) return FBUS_ERR_INVALID;
    const bool m_ok = m >= 1 && m <= FBUS_ROWS_MAX;
    const void *dr, *dH;
    const size_t bytes = (size_t)h->B * (size_t)m * esize(h);
    const Piece in[2] = { in_piece(res, bytes, &dr), in_piece(H, bytes * (size_t)h->N, &dH) };
    const std::string bad_m = m_ok ? std::string() : "m = " + std::to_string(m) + " outside 1.." + std::to_string(FBUS_ROWS_MAX);
    const SensorCall c{ "rows", m_ok, bad_m.c_str(), res && H && var, "res, H and var must not be NULL", m, true };
    return sensor_any(h, t, nis, c, in, 2, var, var_per_filter, skip, out_nis, out_dof,
                      [&](const SensorDev& d) { return launch_rows(h, m, dr, dH, d); });
}

// ---- per-marker screening (ekf_screen.hpp): fbus_ekf_screen_markers / _dev ----------------------------------------------------------------------
// One launcher for both forms and one route: one wave per tile whatever the batch, the team setting, the policy batch or the likelihood
// switch.  Read-only: the records, the applied flags, the likelihood sums, the noise table and records_warm stay as they are.
struct ScreenDst { int32_t* ids; void* nis; int32_t* dof; int32_t* kept; };
template <typename T, int N, int D>
int launch_screen_t(fbus_ekf_t h, int kind, int M, const int32_t* ids, const void* a, const void* b, int geometry, const uint8_t* skip,
                    const ScreenDst& o)
{
    const ScreenOut<T> out{ (int*)o.ids, (T*)o.nis, (int*)o.dof, (int*)o.kept, h->d_gate };
    const double* noise = h->noise_on ? h->d_noise : nullptr;
    const unsigned char* sk = (const unsigned char*)skip;
    if (kind == FBUS_SCREEN_POSE) {
        launch_screen_pose_k<T, N, D>(h->stream, (const T*)h->recs, h->B, M, (const int*)ids, (const T*)a, (const T*)b, noise, sk, make_dc<T>(h), out);
    } else {
        const bool sq = route_key(h).square_port;
        const auto go = [&](auto kind_c, double r) {
            launch_screen_meas_k<T, N, decltype(kind_c)::value>(h->stream, (const T*)h->recs, h->B, M, (const int*)ids, (const T*)a, (const T*)b,
                                                                geometry, sq, h->prm.marker_size, r, noise, sk, h->d_id2slot, make_mc(h),
                                                                make_vc<double>(h), make_vc<T>(h), out);
        };
        if (kind == FBUS_SCREEN_CORNERS) go(std::integral_constant<int, SCREEN_CORNERS>{}, h->prm.r_pos);
        else if (b) go(std::integral_constant<int, SCREEN_PIX_STEREO>{}, h->prm.r_pix);
        else go(std::integral_constant<int, SCREEN_PIX_LEFT>{}, h->prm.r_pix);
    }
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int launch_screen(fbus_ekf_t h, int kind, int M, const int32_t* ids, const void* a, const void* b, int geometry, const uint8_t* skip,
                  const ScreenDst& o)
{
    DISPATCH(h, launch_screen_t, h, kind, M, ids, a, b, geometry, skip, o);
}
// (the order of the tests is part of the interface: include/fbus_ekf.h)
int screen_any(fbus_ekf_t h, Transport t, int kind, int M, const int32_t* ids, const void* a, const void* b, int geometry, const uint8_t* skip,
               int32_t* ids_out, void* nis, int32_t* dof, int32_t* kept)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    const std::string where = t == DEV ? "fbus_ekf_screen_markers_dev" : "fbus_ekf_screen_markers";
    if (kind != FBUS_SCREEN_POSE && kind != FBUS_SCREEN_PIXELS && kind != FBUS_SCREEN_CORNERS)
        return fail(h, FBUS_ERR_INVALID, where + ": kind = " + std::to_string(kind) + " is none of FBUS_SCREEN_POSE / _PIXELS / _CORNERS");
    if (M < 1 || M > FBUS_MAX_VISIBLE)
        return fail(h, FBUS_ERR_INVALID, where + ": M = " + std::to_string(M) + " outside 1.." + std::to_string(FBUS_MAX_VISIBLE));
    if (!ids || !a) return fail(h, FBUS_ERR_INVALID, where + ": ids and a must not be NULL");
    const bool c3d = kind == FBUS_SCREEN_CORNERS && geometry == FBUS_VIS_CORNERS3D;
    if (kind == FBUS_SCREEN_CORNERS && !geometry_ok(geometry)) return fail(h, FBUS_ERR_UNSUPPORTED, where + ": unknown geometry");
    if ((kind == FBUS_SCREEN_POSE || (kind == FBUS_SCREEN_CORNERS && !c3d)) && !b)
        return fail(h, FBUS_ERR_INVALID, where + ": b must not be NULL for this kind");
    if (kind != FBUS_SCREEN_POSE && t == DEV && !points_aligned(a, b))
        return fail(h, FBUS_ERR_INVALID, where + ": a / b must be 16-byte aligned device pointers");
    if (kind == FBUS_SCREEN_PIXELS && !(h->prm.r_pix > 0)) return fail(h, FBUS_ERR_INVALID, where + ": r_pix must be positive");
    const int max_dof = kind == FBUS_SCREEN_PIXELS ? (b ? 16 : 8) : kind == FBUS_SCREEN_CORNERS ? 12 : h->prm.dialect == FBUS_DIALECT_CPP ? 7 : 3;
    const int rc = check_gate_dof(h, max_dof, where.c_str());
    if (rc != FBUS_OK) return rc;
    if (t == DEV) return launch_screen(h, kind, M, ids, a, b, geometry, skip, ScreenDst{ ids_out, nis, dof, kept });
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, where + ": not between graph_begin and graph_end");
    // staged: the ids go in, are screened in place and come back into ids_out
    const size_t es = esize(h), B = (size_t)h->B, BM = B * M;
    const size_t wa = kind == FBUS_SCREEN_POSE ? 3 : (c3d ? 12 : 8), wb = kind == FBUS_SCREEN_POSE ? 4 : 8;
    const void *di, *da, *db, *ds;
    void *dn, *dd, *dk;
    Piece pc[7] = { Piece{ ids, ids_out, BM * sizeof(int32_t), &di, false }, in_piece(a, BM * wa * es, &da),
                    in_piece(b, c3d ? 0 : BM * wb * es, &db), in_piece(skip, B, &ds), out_piece(nis, BM * es, &dn),
                    out_piece(dof, BM * sizeof(int32_t), &dd), out_piece(kept, B * sizeof(int32_t), &dk) };
    return run_pieces(h, t, pc, 7, [&] {
        int32_t* io = ids_out ? const_cast<int32_t*>((const int32_t*)di) : nullptr;
        return launch_screen(h, kind, M, (const int32_t*)di, da, db, geometry, (const uint8_t*)ds, ScreenDst{ io, dn, (int32_t*)dd, (int32_t*)dk });
    });
}

// ---- consistency against a truth state (ekf_nees.hpp): fbus_ekf_nees / _dev ---------------------------------------------------------------------
// One launcher for both forms and one route, as the screening has.  Read-only.
template <typename T, int N, int D>
int launch_nees_t(fbus_ekf_t h, const double* truth, const uint8_t* skip, const NeesOut& o)
{
    launch_nees_k<T, N>(h->stream, (const T*)h->recs, h->B, truth, (const unsigned char*)skip, o);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int launch_nees(fbus_ekf_t h, const double* truth, const uint8_t* skip, const NeesOut& o) { DISPATCH(h, launch_nees_t, h, truth, skip, o); }
int nees_any(fbus_ekf_t h, Transport t, const double* truth, const uint8_t* skip, double* nees, double* err, double* lnp)
{
    if (!h) return FBUS_ERR_INVALID;
    const std::string where = report_name("nees", t);
    if (!truth) return fail(h, FBUS_ERR_INVALID, where + ": truth is NULL");
    const size_t B = (size_t)h->B, N = (size_t)h->N;
    const void *dt, *ds;
    void *dn, *de, *dl;
    Piece pc[5] = { in_piece(truth, B * 19 * sizeof(double), &dt), in_piece(skip, B, &ds),
                    out_piece(nees, B * FBUS_NEES_COLS * sizeof(double), &dn), out_piece(err, B * N * sizeof(double), &de),
                    out_piece(lnp, B * sizeof(double), &dl) };
    return report_any(h, t, where, true, pc, 5, [&] {
        return launch_nees(h, (const double*)dt, (const uint8_t*)ds, NeesOut{ (double*)dn, (double*)de, (double*)dl });
    });
}

// ---- draws from every filter's own Gaussian (ekf_sample.hpp): fbus_ekf_sample / _dev ---------------------------------------------------------
// One launcher for both forms and one route, as NEES has.  Read-only.
template <typename T, int N, int D>
int launch_sample_t(fbus_ekf_t h, int S, const double* xi, const uint8_t* skip, const SampleOut& o)
{
    launch_sample_k<T, N>(h->stream, (const T*)h->recs, h->B, S, xi, (const unsigned char*)skip, o);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int launch_sample(fbus_ekf_t h, int S, const double* xi, const uint8_t* skip, const SampleOut& o) { DISPATCH(h, launch_sample_t, h, S, xi, skip, o); }
int sample_any(fbus_ekf_t h, Transport t, int S, const double* xi, const uint8_t* skip, double* state, uint8_t* drawn)
{
    if (!h) return FBUS_ERR_INVALID;
    const std::string where = report_name("sample", t);
    if (S < 1 || S > FBUS_SAMPLE_MAX) return fail(h, FBUS_ERR_INVALID, where + ": S must be 1.." + std::to_string(FBUS_SAMPLE_MAX));
    if (!xi) return fail(h, FBUS_ERR_INVALID, where + ": xi is NULL");
    const size_t B = (size_t)h->B, N = (size_t)h->N;
    const void *dx, *ds;
    void *dst, *dd;
    Piece pc[4] = { in_piece(xi, (size_t)S * B * N * sizeof(double), &dx), in_piece(skip, B, &ds),
                    out_piece(state, (size_t)S * B * 19 * sizeof(double), &dst), out_piece(drawn, B, &dd) };
    return report_any(h, t, where, true, pc, 4, [&] {
        return launch_sample(h, S, (const double*)dx, (const uint8_t*)ds, SampleOut{ (double*)dst, (unsigned char*)dd });
    });
}

// ---- predicted corner pixels with their innovation covariance (ekf_project.hpp): fbus_ekf_project_markers / _dev -------------------------------
// One launcher for both forms and one route, as the screening has.  Read-only.
struct ProjectDst { void* left; void* right; double* cov_left; double* cov_right; uint8_t* view; };
template <typename T, int N, int D>
int launch_project_t(fbus_ekf_t h, int M, const int32_t* ids, int cameras, const uint8_t* skip, const ProjectDst& o)
{
    const ProjectOut<T> out{ (T*)o.left, (T*)o.right, o.cov_left, o.cov_right, (unsigned char*)o.view };
    const double* noise = h->noise_on ? h->d_noise : nullptr;
    const bool sq = route_key(h).square_port;
    const auto go = [&](auto cam) {
        launch_project_k<T, N, decltype(cam)::value>(h->stream, (const T*)h->recs, h->B, M, (const int*)ids, sq, h->prm.marker_size, h->prm.r_pix,
                                                     noise, (const unsigned char*)skip, h->d_id2slot, make_mc(h), out);
    };
    if (cameras == 2) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 1>{});
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
int launch_project(fbus_ekf_t h, int M, const int32_t* ids, int cameras, const uint8_t* skip, const ProjectDst& o)
{
    DISPATCH(h, launch_project_t, h, M, ids, cameras, skip, o);
}
// (the order of the tests is part of the interface: include/fbus_ekf.h)
int project_any(fbus_ekf_t h, Transport t, int M, const int32_t* ids, int cameras, const uint8_t* skip, void* left, void* right,
                double* cov_left, double* cov_right, uint8_t* view)
{
    if (!h) return FBUS_ERR_INVALID;
    const std::string where = report_name("project_markers", t);
    if (M < 1 || M > FBUS_MAX_VISIBLE)
        return fail(h, FBUS_ERR_INVALID, where + ": M = " + std::to_string(M) + " outside 1.." + std::to_string(FBUS_MAX_VISIBLE));
    if (!ids) return fail(h, FBUS_ERR_INVALID, where + ": ids is NULL");
    if (cameras != 1 && cameras != 2)
        return fail(h, FBUS_ERR_INVALID, where + ": cameras = " + std::to_string(cameras) + " is neither 1 (left) nor 2 (stereo)");
    if (cameras == 1) { right = nullptr; cov_right = nullptr; }                 // (not written: may be anything)
    if (t == DEV && !(points_aligned(left, right) && points_aligned(cov_left, cov_right)))
        return fail(h, FBUS_ERR_INVALID, where + ": left / right / cov_left / cov_right must be 16-byte aligned device pointers");
    if (!(h->prm.r_pix > 0)) return fail(h, FBUS_ERR_INVALID, where + ": r_pix must be positive");
    const size_t es = esize(h), B = (size_t)h->B, BM = B * M;
    const void *di, *ds;
    void *dl, *dr, *dcl, *dcr, *dv;
    Piece pc[7] = { in_piece(ids, BM * sizeof(int32_t), &di), in_piece(skip, B, &ds), out_piece(left, BM * 8 * es, &dl),
                    out_piece(right, BM * 8 * es, &dr), out_piece(cov_left, BM * 12 * sizeof(double), &dcl),
                    out_piece(cov_right, BM * 12 * sizeof(double), &dcr), out_piece(view, BM, &dv) };
    return report_any(h, t, where, true, pc, 7, [&] {
        return launch_project(h, M, (const int32_t*)di, cameras, (const uint8_t*)ds, ProjectDst{ dl, dr, (double*)dcl, (double*)dcr, (uint8_t*)dv });
    });
}

}  // namespace

// ---------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------
extern "C" {

const char* fbus_status_string(int s)
{
    switch (s) {
        case FBUS_OK: return "ok";
        case FBUS_ERR_INVALID: return "invalid argument";
        case FBUS_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
        case FBUS_ERR_HIP: return "HIP runtime error";
        case FBUS_ERR_UNSUPPORTED: return "unsupported dtype/nstate/mode";
        case FBUS_ERR_NOMEM: return "out of memory";
        case FBUS_ERR_ABI: return "caller and library were built against different versions of fbus_ekf.h";
        default: return "unknown status";
    }
}

int fbus_params_default(fbus_params* prm, int dialect)
{
    if (!prm || (dialect != FBUS_DIALECT_MATLAB && dialect != FBUS_DIALECT_CPP)) return FBUS_ERR_INVALID;
    std::memset(prm, 0, sizeof(*prm));
    prm->dialect = dialect;
    prm->cov_form = FBUS_COV_SIMPLE;
    // FBUS_EKF.m:36-39,103-106 ; paramconfig.yml:46-49 via filter.hpp:108-115
    prm->q_diag[0] = 1e-3; prm->q_diag[1] = 1e-4; prm->q_diag[2] = 1e-3; prm->q_diag[3] = 1e-4;
    if (dialect == FBUS_DIALECT_MATLAB) {
        prm->r_pos = 0.01; prm->r_quat = 0.01;                       // FBUS_EKF.m:32-33
        const double d[6] = { 1e-4, 0.1, 1e-4, 1e-3, 1e-3, 100.0 };  // FBUS_EKF.m:88-99
        std::memcpy(prm->p0_diag, d, sizeof(d));
    } else {
        prm->r_pos = 0.001; prm->r_quat = 0.001;                     // paramconfig.yml:53-54
        const double d[6] = { 1e-4, 1e-2, 1e-4, 1e-2, 1e-2, 100.0 }; // filter.hpp:29-34
        std::memcpy(prm->p0_diag, d, sizeof(d));
    }
    // camerainfo1.yml == matlab/config/camerainfo.yml, raw T_SC
    const double TL[16] = { -0.999862, 0.015685, -0.00548, 0.059967,
                            -0.015639, -0.999843, -0.00827, 0.000127837,
                            -0.005609, -0.008183, 0.999951, -0.002,
                            0, 0, 0, 1 };
    const double TR[16] = { -0.999826, 0.00929485, -0.0161445, -0.0601272,
                            -0.00937869, -0.999942, 0.00514829, 0.000124714,
                            -0.0160959, 0.00529897, 0.999857, -0.002,
                            0, 0, 0, 1 };
    std::memcpy(prm->T_SC_left, TL, sizeof(TL));
    std::memcpy(prm->T_SC_right, TR, sizeof(TR));
    // GetMarkerMap.m:1-63 == markersetup.yml
    const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    const double RA[9] = { 1, 0, 0, 0, 0, -1, 0, 1, 0 };
    const double RB[9] = { 1, 0, 0, 0, -1, 0, 0, 0, -1 };
    const struct { int id; double pos[3]; const double* rot; } map[12] = {
        { 0, { 0, 0, 0 }, I3 },         { 1, { 0, 0.61, 0.285 }, RA },  { 2, { 0, 0.61, 1.185 }, RA },
        { 3, { 0, 0.61, 2.085 }, RA },  { 4, { 0, 0.61, 2.985 }, RA },  { 5, { 0, 0.265, 4.12 }, RB },
        { 6, { 0, -0.635, 4.12 }, RB }, { 7, { 0, -1.535, 4.12 }, RB }, { 8, { 0, -2.435, 4.12 }, RB },
        { 16, { 0, -2.7, 0 }, I3 },     { 17, { 0, -1.8, 0 }, I3 },     { 18, { 0, -0.9, 0 }, I3 } };
    prm->n_markers = 12;
    for (int k = 0; k < 12; ++k) {
        prm->marker_id[k] = map[k].id;
        std::memcpy(prm->marker_pos[k], map[k].pos, sizeof(double) * 3);
        std::memcpy(prm->marker_rot[k], map[k].rot, sizeof(double) * 9);
    }
    prm->switch_thres = 0.5;    // paramconfig.yml:57
    prm->max_dist = 2.0;        // paramconfig.yml:56
    prm->n_air = 1.00; prm->n_glass = 1.49; prm->n_water = 1.32;    // paramconfig.yml:31-42
    prm->d_air = 0.002; prm->d_glass = 0.02;
    prm->port_normal[0] = 0; prm->port_normal[1] = 0; prm->port_normal[2] = 1;
    prm->marker_size = 0.28;    // vision.hpp:114
    prm->r_pix = 1e-6;          // (1e-3)^2 in normalised image coordinates: ~0.4 px at the recordings' focal length
    return FBUS_OK;
}

int fbus_params_validate(const fbus_params* prm, char* msg, size_t msg_len)
{
    // everything fbus_ekf_create derives from the parameters on the HOST (no device needed): the camera constants, the marker
    // table and the id -> slot map.  Also what the CPU sanitizer build exercises (tests/test_sanitizers_cpu.py).
    if (msg && msg_len) msg[0] = 0;
    if (!prm) return FBUS_ERR_INVALID;
    std::string err;
    if (prm->dialect != FBUS_DIALECT_MATLAB && prm->dialect != FBUS_DIALECT_CPP) err = "dialect must be FBUS_DIALECT_MATLAB or FBUS_DIALECT_CPP";
    else if (prm->cov_form != FBUS_COV_SIMPLE && prm->cov_form != FBUS_COV_JOSEPH) err = "cov_form must be FBUS_COV_SIMPLE or FBUS_COV_JOSEPH";
    else if (!(prm->r_pos > 0) || !(prm->r_quat > 0)) err = "measurement noise must be positive";
    else {
        HostConst hc;
        (void)build_host_const(*prm, hc, err);
    }
    if (err.empty()) return FBUS_OK;
    if (msg && msg_len) { std::strncpy(msg, err.c_str(), msg_len - 1); msg[msg_len - 1] = 0; }
    return FBUS_ERR_INVALID;
}

int fbus_ekf_abi_version(void) { return FBUS_ABI_VERSION; }
size_t fbus_params_size(void) { return sizeof(fbus_params); }

int fbus_ekf_create_checked(fbus_ekf_t* out, const fbus_params* prm, size_t params_size, int abi_version, int batch, int device,
                            int dtype, int nstate)
{
    if (out) *out = nullptr;
    // checked BEFORE prm is read: a shorter struct must not be copied past its end
    if (abi_version != FBUS_ABI_VERSION || params_size != sizeof(fbus_params)) return FBUS_ERR_ABI;
    return fbus_ekf_create(out, prm, batch, device, dtype, nstate);
}

int fbus_ekf_create(fbus_ekf_t* out, const fbus_params* prm, int batch, int device, int dtype, int nstate)
{
    if (!out) return FBUS_ERR_INVALID;
    *out = nullptr;
    if (!prm || batch <= 0) return FBUS_ERR_INVALID;
    if ((dtype != 32 && dtype != 64) || (nstate != 15 && nstate != 18)) return FBUS_ERR_UNSUPPORTED;
    // the checks of fbus_params_validate (dialect, cov_form, positive noise -- a zero r_pos would turn the fold's weights into NaN --,
    // marker table): the header promises them here
    if (fbus_params_validate(prm, nullptr, 0) != FBUS_OK) return FBUS_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return FBUS_ERR_NO_DEVICE;
    DeviceGuard guard_(device);
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device) return FBUS_ERR_NO_DEVICE;

    fbus_ekf* h = new (std::nothrow) fbus_ekf();
    if (!h) return FBUS_ERR_NOMEM;
    h->B = batch;
    h->Bs = (batch + 63) / 64 * 64;
    {   // launch policy from the device: CU count -> SIMDs, L2 size; the memory-side cache is not exposed (256 MiB assumed)
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
            if (prop.multiProcessorCount > 0) h->cus = prop.multiProcessorCount;
            if (prop.l2CacheSize > 0) h->l2_bytes = (size_t)prop.l2CacheSize;
        }
        int simds = h->cus * 4;
        bool fake = false;
        if (const char* e = std::getenv("FBUS_FAKE_SIMDS")) { const int v = std::atoi(e); if (v >= 4) { simds = v / 4 * 4; h->cus = simds / 4; fake = true; } }
        h->lp.simds = simds;
        h->lp.two_wave_min_b = simds * 64 + 1;
        if (const char* e = std::getenv("FBUS_TWO_WAVE_MIN_B")) h->lp.two_wave_min_b = std::atoi(e);
        h->lp.meas_vec = std::getenv("FBUS_NO_MEAS_VEC") == nullptr;
        // 256 MiB is MI355X's (and MI300X's) Infinity Cache whatever the CU count of the SKU: not scaled with the device; only the
        // test knob FBUS_FAKE_SIMDS (a pretended smaller chip) scales it down with the SIMD count, FBUS_MALL_MB sets it outright
        h->mall_bytes = (size_t)256 << 20;
        if (fake && simds < 1024) h->mall_bytes = ((size_t)256 << 20) / 1024 * (size_t)simds;
        if (const char* e = std::getenv("FBUS_MALL_MB")) { const long v = std::atol(e); if (v > 0) h->mall_bytes = (size_t)v << 20; }
        // records larger than this leave the one-round, cache-resident regime (measured crossover 52-60 MB on 1024 SIMDs, 4.1)
        // (a cache-capacity effect: the same 56 MB on any part with a 256 MiB Infinity Cache; scaled only for a pretended chip)
        h->big_records_mb = (fake && simds < 1024) ? (int)(56L * simds / 1024) : 56;
    }
    if (const char* e = std::getenv("FBUS_BIG_RECORDS_MB")) h->big_records_mb = std::atoi(e);
    if (const char* e = std::getenv("FBUS_WARM_AFTER_CORRECT")) h->warm_after_correct = std::atoi(e) != 0;
    if (const char* e = std::getenv("FBUS_PREDICT_POLICY")) { const int v = std::atoi(e); if (v >= 0 && v <= 2) h->predict_policy_force = v; }
    if (const char* e = std::getenv("FBUS_TEAM_PREDICT")) { const int v = std::atoi(e); if (v >= 0 && v <= 4) h->team_predict = v; }
    if (const char* e = std::getenv("FBUS_TEAM_CORRECT")) { const int v = std::atoi(e); if (v >= 0 && v <= 4) h->team_correct = v; }
    if (const char* e = std::getenv("FBUS_NO_FRAME_MEAS")) h->no_frame_meas = std::atoi(e) != 0;
    if (const char* e = std::getenv("FBUS_MEAS_SPLIT")) { const int v = std::atoi(e); if (v == 0 || v == 2 || v == 4) h->meas_split = v; }
    if (const char* e = std::getenv("FBUS_TEAM_FRAME")) { const int v = std::atoi(e); if (v >= 0 && v <= 2) h->team_frame = v; }
    if (const char* e = std::getenv("FBUS_PREDICT_LD"))          // experiment knob: nt | default | auto
        h->predict_ld = !std::strcmp(e, "nt") ? 1 : (!std::strcmp(e, "default") ? 2 : 0);
    h->device = device;
    h->dtype = dtype;
    h->N = nstate;
    h->prm = *prm;
    std::string err;
    if (!build_host_const(h->prm, h->hc, err)) { delete h; return FBUS_ERR_INVALID; }

    auto bail = [&](int code) { fbus_ekf_destroy(h); return code; };
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(FBUS_ERR_HIP);
    h->stream = h->own_stream;
    h->bytes_per_filter = record_elems(dtype, nstate) * esize(h);
    h->rec_bytes = h->bytes_per_filter * (size_t)h->Bs;
    if (hipMalloc(&h->recs, h->rec_bytes) != hipSuccess) return bail(FBUS_ERR_NOMEM);
    h->own_recs = true;
    if (hipMemsetAsync(h->recs, 0, h->rec_bytes, h->stream) != hipSuccess) return bail(FBUS_ERR_HIP);
    if (hipMalloc((void**)&h->d_applied, (size_t)h->Bs) != hipSuccess) return bail(FBUS_ERR_NOMEM);
    if (hipMemsetAsync(h->d_applied, 0, (size_t)h->Bs, h->stream) != hipSuccess) return bail(FBUS_ERR_HIP);
    // marker table + id lookup
    const size_t nmk = h->hc.mk.size();
    if (hipMalloc(&h->d_mk, nmk * esize(h)) != hipSuccess) return bail(FBUS_ERR_NOMEM);
    if (dtype == 32) {
        std::vector<float> f(h->hc.mk.begin(), h->hc.mk.end());
        if (hipMemcpy(h->d_mk, f.data(), nmk * 4, hipMemcpyHostToDevice) != hipSuccess) return bail(FBUS_ERR_HIP);
    } else {
        if (hipMemcpy(h->d_mk, h->hc.mk.data(), nmk * 8, hipMemcpyHostToDevice) != hipSuccess) return bail(FBUS_ERR_HIP);
    }
    if (hipMalloc((void**)&h->d_mkc, h->hc.mkc.size() * sizeof(double)) != hipSuccess) return bail(FBUS_ERR_NOMEM);
    if (hipMemcpy(h->d_mkc, h->hc.mkc.data(), h->hc.mkc.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return bail(FBUS_ERR_HIP);
    const size_t lut = h->hc.id2slot.size() * sizeof(short);
    if (hipMalloc((void**)&h->d_id2slot, lut) != hipSuccess) return bail(FBUS_ERR_NOMEM);
    if (hipMemcpy(h->d_id2slot, h->hc.id2slot.data(), lut, hipMemcpyHostToDevice) != hipSuccess) return bail(FBUS_ERR_HIP);
    {
        const std::vector<double> none(FBUS_GATE_MAX_DOF + 1, std::numeric_limits<double>::infinity());
        if (hipMalloc((void**)&h->d_gate, none.size() * sizeof(double)) != hipSuccess) return bail(FBUS_ERR_NOMEM);
        if (hipMemcpy(h->d_gate, none.data(), none.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return bail(FBUS_ERR_HIP);
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess) return bail(FBUS_ERR_HIP);
    *out = h;
    return FBUS_OK;
}

int fbus_ekf_destroy(fbus_ekf_t h)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_OK;
    (void)hipStreamSynchronize(h->stream);
    for (auto& p : h->ev_pool) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto g : h->graphs) if (g) (void)hipGraphExecDestroy(g);
    for (void* st : h->stage) if (st) (void)hipFree(st);
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
    for (auto& a : h->aring) {
        if (a.host) (void)hipHostFree(a.host);
        if (a.dev) (void)hipFree(a.dev);
        if (a.copied) (void)hipEventDestroy(a.copied);
        if (a.done) (void)hipEventDestroy(a.done);
    }
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->own_recs && h->recs) (void)hipFree(h->recs);
    if (h->d_applied) (void)hipFree(h->d_applied);
    if (h->d_ema_carry) (void)hipFree(h->d_ema_carry);
    if (h->d_mk) (void)hipFree(h->d_mk);
    if (h->d_mkc) (void)hipFree(h->d_mkc);
    if (h->d_id2slot) (void)hipFree(h->d_id2slot);
    if (h->d_gate) (void)hipFree(h->d_gate);
    if (h->d_noise) (void)hipFree(h->d_noise);
    if (h->d_lik) (void)hipFree(h->d_lik);
    if (h->order_ev) (void)hipEventDestroy(h->order_ev);
    (void)fbus_ekf_comm_destroy(h);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return FBUS_OK;
}

int fbus_ekf_set_team(fbus_ekf_t h, int predict_roles, int correct_roles)
{
    if (!h || predict_roles < 0 || predict_roles > 4 || correct_roles < 0 || correct_roles > 4) return FBUS_ERR_INVALID;
    h->team_predict = predict_roles;
    h->team_correct = correct_roles;
    return FBUS_OK;
}

int fbus_ekf_set_policy_batch(fbus_ekf_t h, int total_filters)
{
    if (!h || total_filters < 0) return FBUS_ERR_INVALID;
    h->policy_batch = total_filters;
    h->lp.policy_b = total_filters;      // the two-wave (<= 256-register) kernel forms follow the job's size too (ekf_launch.hpp)
    return FBUS_OK;
}

int fbus_ekf_launch_info(fbus_ekf_t h, int what, int arg, int* value)
{
    if (!h || !value) return FBUS_ERR_INVALID;
    const RouteKey key = route_key(h);
    switch (what) {
        case FBUS_INFO_SIMDS: *value = h->lp.simds; break;
        case FBUS_INFO_ONE_ROUND_FILTERS: *value = h->lp.simds * 64; break;
        case FBUS_INFO_TWO_WAVE_MIN_B: *value = h->lp.two_wave_min_b; break;
        case FBUS_INFO_BIG_RECORDS_MB: *value = h->big_records_mb; break;
        case FBUS_INFO_MALL_MB: *value = (int)(h->mall_bytes >> 20); break;
        case FBUS_INFO_L2_KB: *value = (int)(h->l2_bytes >> 10); break;
        case FBUS_INFO_POLICY_BATCH: *value = h->policy_batch > 0 ? h->policy_batch : h->B; break;
        case FBUS_INFO_ROLES_PREDICT: *value = team_roles_predict(key, arg > 1 ? arg : 1); break;
        case FBUS_INFO_ROLES_MEAS: *value = team_roles_pixels(key, arg > 0 ? arg : 4); break;
        case FBUS_INFO_TEAM_FRAMES: *value = team_frames(key, FBUS_MODE_STACKED) ? 1 : 0; break;
        case FBUS_INFO_MEAS_SPLIT: *value = meas_split_roles(key, arg > 0 ? arg : 4); break;
        case FBUS_INFO_NOISE_RESIDENT: *value = noise_resident(key) ? 1 : 0; break;
        default: return FBUS_ERR_INVALID;
    }
    return FBUS_OK;
}

int fbus_ekf_set_stream(fbus_ekf_t h, void* hip_stream)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->stream = (hip_stream == FBUS_STREAM_OWN) ? h->own_stream : (hipStream_t)hip_stream;   // NULL = legacy default stream
    return FBUS_OK;
}

// cross-stream ordering without a host sync: one reusable event per handle
static int order_streams(fbus_ekf_t h, hipStream_t first, hipStream_t then)
{
    if (first == then) return FBUS_OK;
    if (!h->order_ev) HIP_TRY(h, hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(h->order_ev, first));
    HIP_TRY(h, hipStreamWaitEvent(then, h->order_ev, 0));
    return FBUS_OK;
}

int fbus_ekf_wait_stream(fbus_ekf_t h, void* other_stream)
{
    DeviceGuard guard_(h);
    if (!h || other_stream == FBUS_STREAM_OWN) return FBUS_ERR_INVALID;
    return order_streams(h, (hipStream_t)other_stream, h->stream);
}

int fbus_ekf_signal_stream(fbus_ekf_t h, void* other_stream)
{
    DeviceGuard guard_(h);
    if (!h || other_stream == FBUS_STREAM_OWN) return FBUS_ERR_INVALID;
    return order_streams(h, h->stream, (hipStream_t)other_stream);
}

int fbus_ekf_sync(fbus_ekf_t h)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FBUS_OK;
}

const char* fbus_ekf_last_error(fbus_ekf_t h) { return h ? h->err.c_str() : "null handle"; }

int fbus_ekf_set_state_dev(fbus_ekf_t h, const void* nominal, const void* rot, const void* P, const int32_t* prev_id)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    return do_pack(h, nominal, rot, P, prev_id);
}

int fbus_ekf_get_state_dev(fbus_ekf_t h, void* nominal, void* rot, void* P, int32_t* prev_id)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    return do_unpack(h, nominal, rot, P, prev_id);
}

int fbus_ekf_set_state(fbus_ekf_t h, const void* nominal, const void* rot, const void* P, const int32_t* prev_id)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    const size_t es = esize(h), B = (size_t)h->B, N = (size_t)h->N;
    const void *dn, *dr, *dP, *dp;
    Piece pc[4] = { in_piece(nominal, B * 19 * es, &dn), in_piece(rot, B * 9 * es, &dr), in_piece(P, B * N * N * es, &dP),
                    in_piece(prev_id, B * sizeof(int32_t), &dp) };
    return run_pieces(h, STAGED, pc, 4, [&] { return do_pack(h, dn, dr, dP, (const int32_t*)dp); });
}

int fbus_ekf_get_state(fbus_ekf_t h, void* nominal, void* rot, void* P, int32_t* prev_id)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    const size_t es = esize(h), B = (size_t)h->B, N = (size_t)h->N;
    void *dn, *dr, *dP, *dp;
    Piece pc[4] = { out_piece(nominal, B * 19 * es, &dn), out_piece(rot, B * 9 * es, &dr), out_piece(P, B * N * N * es, &dP),
                    out_piece(prev_id, B * sizeof(int32_t), &dp) };
    return run_pieces(h, STAGED, pc, 4, [&] { return do_unpack(h, dn, dr, dP, (int32_t*)dp); });
}

int fbus_ekf_reset_cov(fbus_ekf_t h)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    return do_reset_cov(h);
}

// ---------------------------------------------------------------------------------
// multi-GPU: the one collective of the path, a gather of the packed records over RCCL
// ---------------------------------------------------------------------------------
// RCCL is bound at first use (dlopen by soname): a process that already holds an RCCL -- PyTorch-ROCm loads its own copy of
// librccl.so.1 -- shares it, and the library still loads on a box without RCCL (the single-GPU path never touches it).
extern "C++" {
namespace {
struct Rccl {
    using UniqueId = struct { char internal[128]; };
    int (*GetUniqueId)(UniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string err;
    bool ok = false;
};
Rccl& rccl()
{
    static Rccl r = [] {
        Rccl x;
        void* lib = nullptr;
        for (const char* name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" })
            if ((lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!lib) {
            const char* why = dlerror();            // one call: dlerror() clears the message it returns
            x.err = std::string("librccl.so.1 not found: ") + (why ? why : "");
            return x;
        }
        auto sym = [&](const char* n) { void* p = dlsym(lib, n); if (!p && x.err.empty()) x.err = std::string("RCCL symbol missing: ") + n; return p; };
        x.GetUniqueId = (decltype(x.GetUniqueId))sym("ncclGetUniqueId");
        x.CommInitRank = (decltype(x.CommInitRank))sym("ncclCommInitRank");
        x.CommInitAll = (decltype(x.CommInitAll))sym("ncclCommInitAll");
        x.CommDestroy = (decltype(x.CommDestroy))sym("ncclCommDestroy");
        x.AllGather = (decltype(x.AllGather))sym("ncclAllGather");
        x.Broadcast = (decltype(x.Broadcast))sym("ncclBroadcast");
        x.GroupStart = (decltype(x.GroupStart))sym("ncclGroupStart");
        x.GroupEnd = (decltype(x.GroupEnd))sym("ncclGroupEnd");
        x.GetErrorString = (decltype(x.GetErrorString))sym("ncclGetErrorString");
        x.ok = x.err.empty();
        return x;
    }();
    return r;
}
constexpr int kNcclUint8 = 1;       // ncclDataType_t (rccl.h): ncclInt8 = 0, ncclUint8 = 1
int rccl_fail(fbus_ekf_t h, const char* what, int rc)
{
    Rccl& r = rccl();
    return fail(h, FBUS_ERR_HIP, std::string(what) + ": " + (r.GetErrorString ? r.GetErrorString(rc) : "RCCL error"));
}
}  // namespace
}  // extern "C++"

int fbus_ekf_comm_unique_id(void* id128)
{
    if (!id128) return FBUS_ERR_INVALID;
    Rccl& r = rccl();
    if (!r.ok) return FBUS_ERR_UNSUPPORTED;
    Rccl::UniqueId id;
    if (r.GetUniqueId(&id) != 0) return FBUS_ERR_HIP;
    std::memcpy(id128, &id, sizeof(id));
    return FBUS_OK;
}

int fbus_ekf_comm_init(fbus_ekf_t h, const void* id128, int rank, int world)
{
    DeviceGuard guard_(h);
    if (!h || !id128 || world < 1 || rank < 0 || rank >= world) return FBUS_ERR_INVALID;
    Rccl& r = rccl();
    if (!r.ok) return fail(h, FBUS_ERR_UNSUPPORTED, r.err);
    (void)fbus_ekf_comm_destroy(h);
    Rccl::UniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    void* comm = nullptr;
    const int rc = r.CommInitRank(&comm, world, id, rank);         // binds to the current device = the handle's
    if (rc != 0) return rccl_fail(h, "ncclCommInitRank", rc);
    h->comm = comm; h->own_comm = true; h->comm_rank = rank; h->comm_world = world;
    return FBUS_OK;
}

int fbus_ekf_comm_init_all(fbus_ekf_t* handles, int n)
{
    // one process, n handles on n DIFFERENT devices (fbus::NodeFilter): ncclCommInitAll, rank k = handles[k]
    if (!handles || n < 1) return FBUS_ERR_INVALID;
    for (int k = 0; k < n; ++k) {
        if (!handles[k]) return FBUS_ERR_INVALID;
        for (int j = 0; j < k; ++j)
            if (handles[j]->device == handles[k]->device)
                return fail(handles[k], FBUS_ERR_INVALID, "fbus_ekf_comm_init_all: two handles on one device (RCCL wants one rank per device)");
    }
    Rccl& r = rccl();
    if (!r.ok) return fail(handles[0], FBUS_ERR_UNSUPPORTED, r.err);
    std::vector<int> devs(n);
    std::vector<void*> comms(n, nullptr);
    for (int k = 0; k < n; ++k) { devs[k] = handles[k]->device; (void)fbus_ekf_comm_destroy(handles[k]); }
    const int rc = r.CommInitAll(comms.data(), n, devs.data());
    if (rc != 0) return rccl_fail(handles[0], "ncclCommInitAll", rc);
    for (int k = 0; k < n; ++k) { handles[k]->comm = comms[k]; handles[k]->own_comm = true; handles[k]->comm_rank = k; handles[k]->comm_world = n; }
    return FBUS_OK;
}

int fbus_ekf_gather_group(fbus_ekf_t* handles, int n, void* const* out_dev, const size_t* bytes_of_rank)
{
    // the gather of ALL ranks of one process in one RCCL group (a single thread may not issue the ranks' collectives one by one)
    if (!handles || !out_dev || n < 1) return FBUS_ERR_INVALID;
    // everything fbus_ekf_gather would refuse is refused HERE, before the group is opened: a rank that fails inside an open group
    // leaves the ranks in front of it with an incomplete collective enqueued, and ncclGroupEnd would then hang their streams
    for (int k = 0; k < n; ++k) {
        fbus_ekf_t h = handles[k];
        if (!h) return FBUS_ERR_INVALID;
        if (!out_dev[k]) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_gather_group: out_dev[k] is NULL");
        if (!h->comm) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_gather_group: a handle without communicator (fbus_ekf_comm_init_all first)");
        if (h->comm_world != n || h->comm_rank != k)
            return fail(h, FBUS_ERR_INVALID, "fbus_ekf_gather_group: handles[k] is not rank k of an n-rank communicator");
        if (bytes_of_rank && bytes_of_rank[k] != h->rec_bytes)
            return fail(h, FBUS_ERR_INVALID, "fbus_ekf_gather_group: bytes_of_rank[k] is not handles[k]'s record size");
        if (!bytes_of_rank && h->rec_bytes != handles[0]->rec_bytes)
            return fail(h, FBUS_ERR_INVALID, "fbus_ekf_gather_group: ragged shards need bytes_of_rank");
    }
    Rccl& r = rccl();
    if (!r.ok) return fail(handles[0], FBUS_ERR_UNSUPPORTED, r.err);
    int rc = r.GroupStart();
    int first = FBUS_OK;
    for (int k = 0; k < n && rc == 0; ++k) {
        const int e = fbus_ekf_gather(handles[k], out_dev[k], bytes_of_rank);
        if (e != FBUS_OK && first == FBUS_OK) first = e;
    }
    const int rc2 = r.GroupEnd();
    if (first != FBUS_OK) return first;
    if (rc != 0 || rc2 != 0) return rccl_fail(handles[0], "ncclGroupStart / ncclGroupEnd", rc != 0 ? rc : rc2);
    return FBUS_OK;
}

int fbus_ekf_copy_records(fbus_ekf_t h, void* dst, int dst_device)
{
    // this handle's packed records -> dst on dst_device (any device of the process), on the handle's stream: the gather of a
    // single-process job whose consumer sits on ONE device (or whose shards share a device) without a communicator
    DeviceGuard guard_(h);
    if (!h || !dst || dst_device < 0) return FBUS_ERR_INVALID;
    if (dst_device == h->device) HIP_TRY(h, hipMemcpyAsync(dst, h->recs, h->rec_bytes, hipMemcpyDeviceToDevice, h->stream));
    else HIP_TRY(h, hipMemcpyPeerAsync(dst, dst_device, h->recs, h->device, h->rec_bytes, h->stream));
    return FBUS_OK;
}

int fbus_ekf_comm_attach(fbus_ekf_t h, void* nccl_comm, int rank, int world)
{
    if (!h || !nccl_comm || world < 1 || rank < 0 || rank >= world) return FBUS_ERR_INVALID;
    Rccl& r = rccl();
    if (!r.ok) return fail(h, FBUS_ERR_UNSUPPORTED, r.err);
    (void)fbus_ekf_comm_destroy(h);
    h->comm = nccl_comm; h->own_comm = false; h->comm_rank = rank; h->comm_world = world;
    return FBUS_OK;
}

int fbus_ekf_comm_destroy(fbus_ekf_t h)
{
    if (!h) return FBUS_ERR_INVALID;
    if (h->comm && h->own_comm) {
        DeviceGuard guard_(h);
        (void)hipStreamSynchronize(h->stream);
        (void)rccl().CommDestroy(h->comm);
    }
    h->comm = nullptr; h->own_comm = false; h->comm_rank = 0; h->comm_world = 1;
    return FBUS_OK;
}

int fbus_ekf_gather(fbus_ekf_t h, void* out_dev, const size_t* bytes_of_rank)
{
    DeviceGuard guard_(h);
    if (!h || !out_dev) return FBUS_ERR_INVALID;
    if (!h->comm) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_gather: no communicator (fbus_ekf_comm_init / fbus_ekf_comm_attach first)");
    Rccl& r = rccl();
    const int W = h->comm_world;
    bool equal = true;
    if (bytes_of_rank) {
        if (bytes_of_rank[h->comm_rank] != h->rec_bytes) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_gather: bytes_of_rank[rank] is not this handle's record size");
        for (int k = 0; k < W; ++k) equal = equal && bytes_of_rank[k] == h->rec_bytes;
    }
    if (equal) {
        // equal shards (weak scaling, or a total that divides evenly): one all-gather of the packed records
        const int rc = r.AllGather(h->recs, out_dev, h->rec_bytes, kNcclUint8, h->comm, h->stream);
        if (rc != 0) return rccl_fail(h, "ncclAllGather", rc);
        return FBUS_OK;
    }
    // ragged shards (a total batch cut into 64-aligned ranges): one grouped broadcast per rank = an all-gather-v, no padding
    int rc = r.GroupStart();
    size_t off = 0;
    for (int k = 0; k < W && rc == 0; ++k) {
        rc = r.Broadcast(h->recs, (char*)out_dev + off, bytes_of_rank[k], kNcclUint8, k, h->comm, h->stream);
        off += bytes_of_rank[k];
    }
    const int rc2 = r.GroupEnd();
    if (rc != 0 || rc2 != 0) return rccl_fail(h, "ncclBroadcast (grouped)", rc != 0 ? rc : rc2);
    return FBUS_OK;
}

int fbus_ekf_records(fbus_ekf_t h, void** dev_ptr, size_t* bytes_per_filter, size_t* total_bytes)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (dev_ptr) *dev_ptr = h->recs;
    if (bytes_per_filter) *bytes_per_filter = h->bytes_per_filter;
    if (total_bytes) *total_bytes = h->rec_bytes;
    return FBUS_OK;
}

int fbus_ekf_attach_records(fbus_ekf_t h, void* dev_ptr, size_t total_bytes)
{
    DeviceGuard guard_(h);
    if (!h || !dev_ptr) return FBUS_ERR_INVALID;
    if (total_bytes != h->rec_bytes) return fail(h, FBUS_ERR_INVALID, "attach_records: size mismatch");
    if (((uintptr_t)dev_ptr & 15) != 0) return fail(h, FBUS_ERR_INVALID, "attach_records: pointer not 16-byte aligned");
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(dev_ptr, h->recs, h->rec_bytes, hipMemcpyDeviceToDevice));
    if (h->own_recs) HIP_TRY(h, hipFree(h->recs));
    h->recs = dev_ptr;
    h->own_recs = false;
    return FBUS_OK;
}

int fbus_ekf_predict_n_dev(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter)
{
    return predict_any(h, DEV, K, accel, gyro, dt, dt_per_filter);
}

int fbus_ekf_predict_dev(fbus_ekf_t h, const void* accel, const void* gyro, const void* dt, int dt_per_filter)
{
    return predict_any(h, DEV, 1, accel, gyro, dt, dt_per_filter);
}

int fbus_ekf_predict_n(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter)
{
    return predict_any(h, STAGED, K, accel, gyro, dt, dt_per_filter);
}

int fbus_ekf_predict(fbus_ekf_t h, const void* accel, const void* gyro, const void* dt, int dt_per_filter)
{
    return predict_any(h, STAGED, 1, accel, gyro, dt, dt_per_filter);
}

int fbus_ekf_predict_n_async(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter)
{
    return predict_any(h, ASYNC, K, accel, gyro, dt, dt_per_filter);
}

int fbus_ekf_predict_async(fbus_ekf_t h, const void* accel, const void* gyro, const void* dt, int dt_per_filter)
{
    return predict_any(h, ASYNC, 1, accel, gyro, dt, dt_per_filter);
}

int fbus_ekf_correct_async(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip)
{
    return correct_any(h, ASYNC, false, M, ids, pos, quat, mode, skip, nullptr, nullptr);
}

int fbus_ekf_correct_pixels_async(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, const uint8_t* skip)
{
    return correct_pixels_any(h, ASYNC, false, M, ids, left, right, skip, nullptr, nullptr);
}

int fbus_ekf_async_inputs_consumed(fbus_ekf_t h)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (h->copy_stream) HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
    return FBUS_OK;
}

int fbus_ekf_async_stats(fbus_ekf_t h, int64_t* calls, int64_t* waits, int64_t* direct_pieces)
{
    if (!h) return FBUS_ERR_INVALID;
    if (calls) *calls = h->async_calls;
    if (waits) *waits = h->async_waits;
    if (direct_pieces) *direct_pieces = h->async_direct;
    return FBUS_OK;
}

int fbus_ekf_host_register(void* ptr, size_t bytes)
{
    if (!ptr || bytes == 0) return FBUS_ERR_INVALID;
    return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? FBUS_OK : ((void)hipGetLastError(), FBUS_ERR_HIP);
}

int fbus_ekf_host_unregister(void* ptr)
{
    if (!ptr) return FBUS_ERR_INVALID;
    return hipHostUnregister(ptr) == hipSuccess ? FBUS_OK : ((void)hipGetLastError(), FBUS_ERR_HIP);
}

int fbus_ekf_correct_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode,
                         const uint8_t* skip)
{
    return correct_any(h, DEV, false, M, ids, pos, quat, mode, skip, nullptr, nullptr);
}

int fbus_ekf_correct(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode,
                     const uint8_t* skip)
{
    return correct_any(h, STAGED, false, M, ids, pos, quat, mode, skip, nullptr, nullptr);
}

int fbus_ekf_correct_corners_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right,
                                 int geometry, int mode, const uint8_t* skip)
{
    return correct_corners_any(h, DEV, false, M, ids, left, right, geometry, mode, skip, nullptr, nullptr);
}

int fbus_ekf_correct_corners(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right,
                             int geometry, int mode, const uint8_t* skip)
{
    return correct_corners_any(h, STAGED, false, M, ids, left, right, geometry, mode, skip, nullptr, nullptr);
}

int fbus_ekf_correct_pixels_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right,
                                const uint8_t* skip)
{
    return correct_pixels_any(h, DEV, false, M, ids, left, right, skip, nullptr, nullptr);
}

int fbus_ekf_correct_pixels(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right,
                            const uint8_t* skip)
{
    return correct_pixels_any(h, STAGED, false, M, ids, left, right, skip, nullptr, nullptr);
}

int fbus_ekf_set_gate(fbus_ekf_t h, int n, const double* thresholds)
{
    DeviceGuard guard_(h);
    if (!h || n < 0) return FBUS_ERR_INVALID;
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_gate: not between graph_begin and graph_end");
    if (!thresholds) n = 0;
    if (n > FBUS_GATE_MAX_DOF + 1) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_gate: more than FBUS_GATE_MAX_DOF + 1 thresholds");
    std::vector<double> thr(FBUS_GATE_MAX_DOF + 1, std::numeric_limits<double>::infinity());
    for (int i = 0; i < n; ++i) {
        if (!(thresholds[i] >= 0.0)) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_gate: thresholds must be >= 0 (+inf allowed, NaN not)");
        thr[i] = thresholds[i];
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_gate, thr.data(), thr.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // (thr is a local)
    h->gate_n = n;
    return FBUS_OK;
}

// ---- per-filter noise (fbus_ekf_set_noise*, include/fbus_ekf.h) ----
namespace {
const char* const kNoiseCols[FBUS_NOISE_COLS] = { "q_v", "q_theta", "q_ba", "q_bg", "r_pos", "r_quat", "r_pix" };
// the table buffer, allocated once (the +inf gate table behind the fields written with it)
int ensure_noise(fbus_ekf_t h)
{
    if (h->d_noise) return FBUS_OK;
    const size_t nf = (size_t)FBUS_NOISE_COLS * h->B;
    double* d = nullptr;
    if (hipMalloc((void**)&d, (nf + FBUS_GATE_MAX_DOF + 1) * sizeof(double)) != hipSuccess)
        return fail(h, FBUS_ERR_NOMEM, "fbus_ekf_set_noise: device allocation");
    const std::vector<double> none(FBUS_GATE_MAX_DOF + 1, std::numeric_limits<double>::infinity());
    if (hipMemcpyAsync(d + nf, none.data(), none.size() * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
        (void)hipFree(d);
        return fail(h, FBUS_ERR_HIP, "fbus_ekf_set_noise: copy of the +inf gate table");
    }
    h->d_noise = d;
    return FBUS_OK;
}
// fbus_params' own row into every filter's table fields: what the likelihood kernels (always the tabled kind) read while the caller has
// set no table.  Stream-ordered; noise_on is not touched.
int lik_fill(fbus_ekf_t h)
{
    int rc = ensure_noise(h);
    if (rc != FBUS_OK) return rc;
    const fbus_params& p = h->prm;
    // (r_pix may be unset -- 0 -- on a handle that never runs the pixel rows: those entry points refuse it themselves)
    const double row[FBUS_NOISE_COLS] = { p.q_diag[0], p.q_diag[1], p.q_diag[2], p.q_diag[3], p.r_pos, p.r_quat, p.r_pix };
    launch_noise_own_row_k(h->stream, h->d_noise, h->B, row);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}
}  // namespace

int fbus_ekf_loglik_enable(fbus_ekf_t h, int on)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_loglik_enable: not between graph_begin and graph_end");
    if (!on) { h->lik_on = false; return FBUS_OK; }
    if (!h->d_lik) {
        double* d = nullptr;
        if (hipMalloc((void**)&d, 4 * (size_t)h->B * sizeof(double)) != hipSuccess)
            return fail(h, FBUS_ERR_NOMEM, "fbus_ekf_loglik_enable: device allocation");
        if (hipMemsetAsync(d, 0, 4 * (size_t)h->B * sizeof(double), h->stream) != hipSuccess) {
            (void)hipFree(d);
            return fail(h, FBUS_ERR_HIP, "fbus_ekf_loglik_enable: zeroing the sums");
        }
        h->d_lik = d;
    }
    if (!h->noise_on) {
        const int rc = lik_fill(h);
        if (rc != FBUS_OK) return rc;
    }
    h->lik_on = true;
    return FBUS_OK;
}

int fbus_ekf_loglik_reset(fbus_ekf_t h)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (!h->d_lik) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_loglik_reset: fbus_ekf_loglik_enable(h, 1) has not been called");
    HIP_TRY(h, hipMemsetAsync(h->d_lik, 0, 4 * (size_t)h->B * sizeof(double), h->stream));
    return FBUS_OK;
}

int fbus_ekf_loglik_get_dev(fbus_ekf_t h, double* ll, int64_t* rows, int32_t* applied, int32_t* rejected)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (!h->d_lik) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_loglik_get_dev: fbus_ekf_loglik_enable(h, 1) has not been called");
    if (!ll && !rows && !applied && !rejected) return FBUS_OK;
    launch_lik_export_k(h->stream, h->d_lik, h->B, ll, rows, applied, rejected);
    HIP_TRY(h, hipGetLastError());
    return FBUS_OK;
}

int fbus_ekf_loglik_get(fbus_ekf_t h, double* ll, int64_t* rows, int32_t* applied, int32_t* rejected)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (!h->d_lik) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_loglik_get: fbus_ekf_loglik_enable(h, 1) has not been called");
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_loglik_get: not between graph_begin and graph_end");
    const size_t B = (size_t)h->B;
    std::vector<double> acc(4 * B);
    HIP_TRY(h, hipMemcpyAsync(acc.data(), h->d_lik, acc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < B; ++b) {
        if (ll) ll[b] = acc[b];
        if (rows) rows[b] = (int64_t)acc[B + b];
        if (applied) applied[b] = (int32_t)acc[2 * B + b];
        if (rejected) rejected[b] = (int32_t)acc[3 * B + b];
    }
    return FBUS_OK;
}

int fbus_ekf_set_noise(fbus_ekf_t h, const double* table)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_noise: not between graph_begin and graph_end");
    if (!table) { h->noise_on = false; return h->lik_on ? lik_fill(h) : FBUS_OK; }
    const size_t B = (size_t)h->B;
    std::vector<double> fields((size_t)FBUS_NOISE_COLS * B);
    for (size_t b = 0; b < B; ++b)
        for (int c = 0; c < FBUS_NOISE_COLS; ++c) {
            const double v = table[b * FBUS_NOISE_COLS + c];
            const bool ok = std::isfinite(v) && (c < 4 ? v >= 0.0 : v > 0.0);     // as fbus_params_validate: q >= 0, r > 0
            if (!ok) {
                char msg[160];
                std::snprintf(msg, sizeof msg, "fbus_ekf_set_noise: row %zu column %d (%s) = %g: must be finite and %s", b, c,
                              kNoiseCols[c], v, c < 4 ? ">= 0" : "> 0");
                return fail(h, FBUS_ERR_INVALID, msg);
            }
            fields[(size_t)c * B + b] = v;
        }
    int rc = ensure_noise(h);
    if (rc != FBUS_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_noise, fields.data(), fields.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // (fields is a local)
    h->noise_on = true;
    return FBUS_OK;
}

int fbus_ekf_set_noise_dev(fbus_ekf_t h, const double* table)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_noise_dev: not between graph_begin and graph_end");
    if (!table) { h->noise_on = false; return h->lik_on ? lik_fill(h) : FBUS_OK; }
    int rc = ensure_noise(h);
    if (rc != FBUS_OK) return rc;
    launch_noise_fields_k(h->stream, table, h->d_noise, h->B);
    HIP_TRY(h, hipGetLastError());
    h->noise_on = true;
    return FBUS_OK;
}

int fbus_ekf_get_noise(fbus_ekf_t h, double* table)
{
    DeviceGuard guard_(h);
    if (!h || !table) return FBUS_ERR_INVALID;
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_get_noise: not between graph_begin and graph_end");
    if (!h->noise_on) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_get_noise: no noise table is set");
    const size_t B = (size_t)h->B;
    std::vector<double> fields((size_t)FBUS_NOISE_COLS * B);
    HIP_TRY(h, hipMemcpyAsync(fields.data(), h->d_noise, fields.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < B; ++b)
        for (int c = 0; c < FBUS_NOISE_COLS; ++c) table[b * FBUS_NOISE_COLS + c] = fields[(size_t)c * B + b];
    return FBUS_OK;
}

int fbus_ekf_group_fuse_dev(fbus_ekf_t h, int G, const double* logw, double* weight, int32_t* best, void* nominal, void* P, void* pdiag)
{
    return group_fuse_any(h, DEV, G, logw, weight, best, nominal, P, pdiag);
}
int fbus_ekf_group_fuse(fbus_ekf_t h, int G, const double* logw, double* weight, int32_t* best, void* nominal, void* P, void* pdiag)
{
    return group_fuse_any(h, STAGED, G, logw, weight, best, nominal, P, pdiag);
}
int fbus_ekf_group_collapse_dev(fbus_ekf_t h, int G, const int32_t* src) { return group_collapse_any(h, DEV, G, src); }
int fbus_ekf_group_collapse(fbus_ekf_t h, int G, const int32_t* src) { return group_collapse_any(h, STAGED, G, src); }
int fbus_ekf_group_mix_dev(fbus_ekf_t h, int G, const double* logw, const double* trans, double* weight, double* logc)
{
    return group_mix_any(h, DEV, G, logw, trans, weight, logc);
}
int fbus_ekf_group_mix(fbus_ekf_t h, int G, const double* logw, const double* trans, double* weight, double* logc)
{
    return group_mix_any(h, STAGED, G, logw, trans, weight, logc);
}

int fbus_ekf_set_depth_sensor(fbus_ekf_t h, const double axis[3], double offset, const double lever[3])
{
    if (!h) return FBUS_ERR_INVALID;
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_depth_sensor: not between graph_begin and graph_end");
    if (!axis) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_depth_sensor: axis must not be NULL");
    const double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    if (!std::isfinite(n) || !(n > 0.0)) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_depth_sensor: axis must be finite and not zero");
    if (!std::isfinite(offset)) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_depth_sensor: offset must be finite");
    if (lever && !(std::isfinite(lever[0]) && std::isfinite(lever[1]) && std::isfinite(lever[2])))
        return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_depth_sensor: lever must be finite");
    for (int i = 0; i < 3; ++i) {
        h->depth.axis[i] = axis[i] / n;
        h->depth.lever[i] = lever ? lever[i] : 0.0;
    }
    h->depth.offset = offset;
    h->depth_set = true;
    return FBUS_OK;
}
int fbus_ekf_correct_depth(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip)
{
    return depth_any(h, STAGED, false, z, var, var_per_filter, skip, nullptr, nullptr);
}
int fbus_ekf_correct_depth_dev(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip)
{
    return depth_any(h, DEV, false, z, var, var_per_filter, skip, nullptr, nullptr);
}
int fbus_ekf_correct_depth_async(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip)
{
    return depth_any(h, ASYNC, false, z, var, var_per_filter, skip, nullptr, nullptr);
}
int fbus_ekf_correct_depth_nis(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip, void* nis,
                               int32_t* dof)
{
    return depth_any(h, STAGED, true, z, var, var_per_filter, skip, nis, dof);
}
int fbus_ekf_correct_depth_nis_dev(fbus_ekf_t h, const void* z, const double* var, int var_per_filter, const uint8_t* skip, void* nis,
                                   int32_t* dof)
{
    return depth_any(h, DEV, true, z, var, var_per_filter, skip, nis, dof);
}
int fbus_ekf_screen_markers(fbus_ekf_t h, int kind, int M, const int32_t* ids, const void* a, const void* b, int geometry, const uint8_t* skip,
                            int32_t* ids_out, void* nis, int32_t* dof, int32_t* kept)
{
    return screen_any(h, STAGED, kind, M, ids, a, b, geometry, skip, ids_out, nis, dof, kept);
}
int fbus_ekf_screen_markers_dev(fbus_ekf_t h, int kind, int M, const int32_t* ids, const void* a, const void* b, int geometry, const uint8_t* skip,
                                int32_t* ids_out, void* nis, int32_t* dof, int32_t* kept)
{
    return screen_any(h, DEV, kind, M, ids, a, b, geometry, skip, ids_out, nis, dof, kept);
}
int fbus_ekf_nees(fbus_ekf_t h, const double* truth, const uint8_t* skip, double* nees, double* err, double* lnp)
{
    return nees_any(h, STAGED, truth, skip, nees, err, lnp);
}
int fbus_ekf_nees_dev(fbus_ekf_t h, const double* truth, const uint8_t* skip, double* nees, double* err, double* lnp)
{
    return nees_any(h, DEV, truth, skip, nees, err, lnp);
}
int fbus_ekf_sample(fbus_ekf_t h, int S, const double* xi, const uint8_t* skip, double* state, uint8_t* drawn)
{
    return sample_any(h, STAGED, S, xi, skip, state, drawn);
}
int fbus_ekf_sample_dev(fbus_ekf_t h, int S, const double* xi, const uint8_t* skip, double* state, uint8_t* drawn)
{
    return sample_any(h, DEV, S, xi, skip, state, drawn);
}
int fbus_ekf_project_markers(fbus_ekf_t h, int M, const int32_t* ids, int cameras, const uint8_t* skip, void* left, void* right,
                             double* cov_left, double* cov_right, uint8_t* view)
{
    return project_any(h, STAGED, M, ids, cameras, skip, left, right, cov_left, cov_right, view);
}
int fbus_ekf_project_markers_dev(fbus_ekf_t h, int M, const int32_t* ids, int cameras, const uint8_t* skip, void* left, void* right,
                                 double* cov_left, double* cov_right, uint8_t* view)
{
    return project_any(h, DEV, M, ids, cameras, skip, left, right, cov_left, cov_right, view);
}

int fbus_ekf_set_velocity_sensor(fbus_ekf_t h, const double mount[9], const double lever[3])
{
    if (!h) return FBUS_ERR_INVALID;
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_velocity_sensor: not between graph_begin and graph_end");
    VelocitySensor vs{};
    for (int i = 0; i < 9; ++i) vs.C[i] = mount ? mount[i] : (i % 4 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(vs.C[i])) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_velocity_sensor: mount must be finite");
    double dev = 0.0;                               // max |C C' - I|
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double cct = vs.C[3 * i] * vs.C[3 * j] + vs.C[3 * i + 1] * vs.C[3 * j + 1] + vs.C[3 * i + 2] * vs.C[3 * j + 2];
            dev = std::max(dev, std::fabs(cct - (i == j ? 1.0 : 0.0)));
        }
    if (!(dev <= 1e-6)) return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_velocity_sensor: mount must be a rotation (max |C C' - I| <= 1e-6)");
    if (lever && !(std::isfinite(lever[0]) && std::isfinite(lever[1]) && std::isfinite(lever[2])))
        return fail(h, FBUS_ERR_INVALID, "fbus_ekf_set_velocity_sensor: lever must be finite");
    for (int i = 0; i < 3; ++i) vs.lever[i] = lever ? lever[i] : 0.0;
    h->velocity = vs;
    h->velocity_set = true;
    return FBUS_OK;
}
int fbus_ekf_correct_velocity(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter, const uint8_t* skip)
{
    return velocity_any(h, STAGED, false, z, gyro, var, var_per_filter, skip, nullptr, nullptr);
}
int fbus_ekf_correct_velocity_dev(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter, const uint8_t* skip)
{
    return velocity_any(h, DEV, false, z, gyro, var, var_per_filter, skip, nullptr, nullptr);
}
int fbus_ekf_correct_velocity_async(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter, const uint8_t* skip)
{
    return velocity_any(h, ASYNC, false, z, gyro, var, var_per_filter, skip, nullptr, nullptr);
}
int fbus_ekf_correct_velocity_nis(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter, const uint8_t* skip,
                                  void* nis, int32_t* dof)
{
    return velocity_any(h, STAGED, true, z, gyro, var, var_per_filter, skip, nis, dof);
}
int fbus_ekf_correct_velocity_nis_dev(fbus_ekf_t h, const void* z, const void* gyro, const double* var, int var_per_filter,
                                      const uint8_t* skip, void* nis, int32_t* dof)
{
    return velocity_any(h, DEV, true, z, gyro, var, var_per_filter, skip, nis, dof);
}
int fbus_ekf_correct_rows(fbus_ekf_t h, int m, const void* res, const void* H, const double* var, int var_per_filter, const uint8_t* skip)
{
    return rows_any(h, STAGED, false, m, res, H, var, var_per_filter, skip, nullptr, nullptr);
}
int fbus_ekf_correct_rows_dev(fbus_ekf_t h, int m, const void* res, const void* H, const double* var, int var_per_filter, const uint8_t* skip)
{
    return rows_any(h, DEV, false, m, res, H, var, var_per_filter, skip, nullptr, nullptr);
}
int fbus_ekf_correct_rows_nis(fbus_ekf_t h, int m, const void* res, const void* H, const double* var, int var_per_filter, const uint8_t* skip,
                              void* nis, int32_t* dof)
{
    return rows_any(h, STAGED, true, m, res, H, var, var_per_filter, skip, nis, dof);
}
int fbus_ekf_correct_rows_nis_dev(fbus_ekf_t h, int m, const void* res, const void* H, const double* var, int var_per_filter,
                                  const uint8_t* skip, void* nis, int32_t* dof)
{
    return rows_any(h, DEV, true, m, res, H, var, var_per_filter, skip, nis, dof);
}

int fbus_ekf_correct_nis_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip,
                             void* nis, int32_t* dof)
{
    return correct_any(h, DEV, true, M, ids, pos, quat, mode, skip, nis, dof);
}

int fbus_ekf_correct_nis(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip,
                         void* nis, int32_t* dof)
{
    return correct_any(h, STAGED, true, M, ids, pos, quat, mode, skip, nis, dof);
}

int fbus_ekf_correct_pixels_nis_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, const uint8_t* skip,
                                    void* nis, int32_t* dof)
{
    return correct_pixels_any(h, DEV, true, M, ids, left, right, skip, nis, dof);
}

int fbus_ekf_correct_pixels_nis(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, const uint8_t* skip,
                                void* nis, int32_t* dof)
{
    return correct_pixels_any(h, STAGED, true, M, ids, left, right, skip, nis, dof);
}

int fbus_ekf_correct_corners_nis_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, int geometry,
                                     int mode, const uint8_t* skip, void* nis, int32_t* dof)
{
    return correct_corners_any(h, DEV, true, M, ids, left, right, geometry, mode, skip, nis, dof);
}

int fbus_ekf_correct_corners_nis(fbus_ekf_t h, int M, const int32_t* ids, const void* left, const void* right, int geometry,
                                 int mode, const uint8_t* skip, void* nis, int32_t* dof)
{
    return correct_corners_any(h, STAGED, true, M, ids, left, right, geometry, mode, skip, nis, dof);
}

int fbus_ekf_get_applied(fbus_ekf_t h, uint8_t* applied_host)
{
    DeviceGuard guard_(h);
    if (!h || !applied_host) return FBUS_ERR_INVALID;
    HIP_TRY(h, hipMemcpyAsync(applied_host, h->d_applied, (size_t)h->B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FBUS_OK;
}

int fbus_ekf_frame_fused_dev(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter,
                             int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip)
{
    return frame_any(h, true, K, accel, gyro, dt, dt_per_filter, M, ids, pos, quat, mode, skip);
}

int fbus_ekf_frame_meas_fused_dev(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter,
                                  int kind, int M, const int32_t* ids, const void* left, const void* right, int geometry, int mode,
                                  const uint8_t* skip)
{
    return frames_meas_any(h, "fbus_ekf_frame_meas_fused_dev", true, 1, &K, accel, gyro, dt, dt_per_filter, kind, M, ids, left, right,
                           geometry, mode, skip, nullptr);
}

int fbus_ekf_frames_meas_fused_dev(fbus_ekf_t h, int nframes, const int32_t* kcount, const void* accel, const void* gyro, const void* dt,
                                   int dt_per_filter, int kind, int M, const int32_t* ids, const void* left, const void* right, int geometry,
                                   int mode, const uint8_t* skip)
{
    return frames_meas_any(h, "fbus_ekf_frames_meas_fused_dev", false, nframes, kcount, accel, gyro, dt, dt_per_filter, kind, M, ids, left,
                           right, geometry, mode, skip, nullptr);
}

int fbus_ekf_frames_meas_fused_traj_dev(fbus_ekf_t h, int nframes, const int32_t* kcount, const void* accel, const void* gyro,
                                        const void* dt, int dt_per_filter, int kind, int M, const int32_t* ids, const void* left,
                                        const void* right, int geometry, int mode, const uint8_t* skip, void* out_nominal, void* out_pdiag,
                                        uint8_t* out_applied)
{
    const TrajDst tj{ out_nominal, out_pdiag, out_applied };
    const bool any = out_nominal || out_pdiag || out_applied;
    return frames_meas_any(h, "fbus_ekf_frames_meas_fused_traj_dev", false, nframes, kcount, accel, gyro, dt, dt_per_filter, kind, M, ids,
                           left, right, geometry, mode, skip, any ? &tj : nullptr);
}

int fbus_ekf_frames_fused_dev(fbus_ekf_t h, int nframes, const int32_t* kcount, const void* accel, const void* gyro,
                              const void* dt, int dt_per_filter, int M, const int32_t* ids, const void* pos,
                              const void* quat, int mode, const uint8_t* skip)
{
    return frames_any(h, "fbus_ekf_frames_fused_dev", nframes, kcount, accel, gyro, dt, dt_per_filter, M, ids, pos, quat, mode, skip,
                      nullptr);
}

int fbus_ekf_frames_fused_traj_dev(fbus_ekf_t h, int nframes, const int32_t* kcount, const void* accel, const void* gyro,
                                   const void* dt, int dt_per_filter, int M, const int32_t* ids, const void* pos,
                                   const void* quat, int mode, const uint8_t* skip, void* out_nominal, void* out_pdiag,
                                   uint8_t* out_applied)
{
    const TrajDst tj{ out_nominal, out_pdiag, out_applied };
    const bool any = out_nominal || out_pdiag || out_applied;
    return frames_any(h, "fbus_ekf_frames_fused_traj_dev", nframes, kcount, accel, gyro, dt, dt_per_filter, M, ids, pos, quat, mode, skip,
                      any ? &tj : nullptr);
}

int fbus_ekf_snapshot_dev(fbus_ekf_t h, void* nominal, void* pdiag, uint8_t* applied)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (!nominal && !pdiag && !applied) return FBUS_OK;
    const TrajDst tj{ nominal, pdiag, applied };
    int rc = check_traj(h, tj, 1, "fbus_ekf_snapshot_dev");
    return rc != FBUS_OK ? rc : do_snapshot(h, nominal, pdiag, applied);
}

int fbus_ekf_frame_dev(fbus_ekf_t h, int K, const void* accel, const void* gyro, const void* dt, int dt_per_filter,
                       int M, const int32_t* ids, const void* pos, const void* quat, int mode, const uint8_t* skip)
{
    return frame_any(h, false, K, accel, gyro, dt, dt_per_filter, M, ids, pos, quat, mode, skip);
}

int fbus_ekf_marker_pose_dev(fbus_ekf_t h, int n, int geometry, const void* left, const void* right, void* pos,
                             void* quat, void* corners3d)
{
    return marker_pose_any(h, DEV, n, geometry, left, right, pos, quat, corners3d);
}

int fbus_ekf_marker_pose(fbus_ekf_t h, int n, int geometry, const void* left, const void* right, void* pos,
                         void* quat, void* corners3d)
{
    return marker_pose_any(h, STAGED, n, geometry, left, right, pos, quat, corners3d);
}

int fbus_ekf_init_gravity_bias_dev(fbus_ekf_t h, int T, const void* accel, const void* gyro)
{
    return init_gravity_bias_any(h, DEV, T, accel, gyro);
}

int fbus_ekf_init_gravity_bias(fbus_ekf_t h, int T, const void* accel, const void* gyro)
{
    return init_gravity_bias_any(h, STAGED, T, accel, gyro);
}

int fbus_ekf_pose_init_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int what,
                           const uint8_t* mask)
{
    return pose_init_any(h, DEV, M, ids, pos, quat, what, mask, nullptr);
}

int fbus_ekf_vision_only_pose_dev(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat,
                                  void* out_pose)
{
    return pose_init_any(h, DEV, M, ids, pos, quat, POSE_VISION, nullptr, out_pose);
}

int fbus_ekf_pose_init(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, int what,
                       const uint8_t* mask)
{
    return pose_init_any(h, STAGED, M, ids, pos, quat, what, mask, nullptr);
}

int fbus_ekf_vision_only_pose(fbus_ekf_t h, int M, const int32_t* ids, const void* pos, const void* quat, void* out_pose)
{
    return pose_init_any(h, STAGED, M, ids, pos, quat, POSE_VISION, nullptr, out_pose);
}

int fbus_ekf_imu_ema_dev(fbus_ekf_t h, int T, void* accel, void* gyro, int restart)
{
    return imu_ema_any(h, DEV, T, accel, gyro, restart);
}

int fbus_ekf_imu_ema(fbus_ekf_t h, int T, void* accel, void* gyro, int restart)
{
    return imu_ema_any(h, STAGED, T, accel, gyro, restart);
}

int fbus_ekf_graph_begin(fbus_ekf_t h)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (h->capturing) return fail(h, FBUS_ERR_INVALID, "graph_begin: already capturing");
    const int rc = flush_events(h);
    if (rc != FBUS_OK) return rc;
    HIP_TRY(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    h->capturing = true;
    return FBUS_OK;
}

int fbus_ekf_graph_end(fbus_ekf_t h, int* graph_id)
{
    DeviceGuard guard_(h);
    if (!h || !graph_id) return FBUS_ERR_INVALID;
    if (!h->capturing) return fail(h, FBUS_ERR_INVALID, "graph_end: not capturing");
    h->capturing = false;
    hipGraph_t g = nullptr;
    HIP_TRY(h, hipStreamEndCapture(h->stream, &g));
    hipGraphExec_t ex = nullptr;
    const hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return fail(h, FBUS_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    h->graphs.push_back(ex);
    *graph_id = (int)h->graphs.size() - 1;
    return FBUS_OK;
}

int fbus_ekf_graph_launch(fbus_ekf_t h, int graph_id)
{
    DeviceGuard guard_(h);
    if (!h || graph_id < 0 || graph_id >= (int)h->graphs.size() || !h->graphs[graph_id]) return FBUS_ERR_INVALID;
    HIP_TRY(h, hipGraphLaunch(h->graphs[graph_id], h->stream));
    return FBUS_OK;
}

int fbus_ekf_graph_destroy(fbus_ekf_t h, int graph_id)
{
    DeviceGuard guard_(h);
    if (!h || graph_id < 0 || graph_id >= (int)h->graphs.size() || !h->graphs[graph_id]) return FBUS_ERR_INVALID;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipGraphExecDestroy(h->graphs[graph_id]));
    h->graphs[graph_id] = nullptr;
    return FBUS_OK;
}

int fbus_ekf_timing_enable(fbus_ekf_t h, int on)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    if (!on) { const int rc = flush_events(h); if (rc != FBUS_OK) return rc; }
    h->timing = on != 0;
    h->timing_stride = on > 1 ? on : 1;
    return FBUS_OK;
}

int fbus_ekf_timing_reset(fbus_ekf_t h)
{
    DeviceGuard guard_(h);
    if (!h) return FBUS_ERR_INVALID;
    const int rc = flush_events(h);
    if (rc != FBUS_OK) return rc;
    for (int i = 0; i < FBUS_KERNEL_COUNT; ++i) { h->t_ms[i] = 0; h->t_n[i] = 0; }
    h->frame_count = 0;                 // the first frame after a reset is a sampled one, whatever the stride
    return FBUS_OK;
}

int fbus_ekf_timing_read(fbus_ekf_t h, int kernel, double* total_ms, int64_t* launches)
{
    DeviceGuard guard_(h);
    if (!h || kernel < 0 || kernel >= FBUS_KERNEL_COUNT) return FBUS_ERR_INVALID;
    const int rc = flush_events(h);
    if (rc != FBUS_OK) return rc;
    if (total_ms) *total_ms = h->t_ms[kernel];
    if (launches) *launches = h->t_n[kernel];
    return FBUS_OK;
}

int fbus_ekf_l0_eval(fbus_ekf_t h, int op, int n, const void* a, const void* b, void* out)
{
    DeviceGuard guard_(h);
    static const int wa[] = { 4, 4, 4, 4, 3, 3, 1 }, wb[] = { 4, 0, 0, 0, 1, 0, 0 }, wo[] = { 4, 9, 9, 4, 9, 4, 4 };
    if (!h || op < 0 || op > FBUS_L0_SINCOS_HALF || n < 1 || !a || !out || (wb[op] && !b)) return FBUS_ERR_INVALID;
    const size_t es = esize(h);
    const void *da, *db;
    void* dout;
    Piece pc[3] = { in_piece(a, (size_t)n * wa[op] * es, &da), in_piece(wb[op] ? b : nullptr, (size_t)n * wb[op] * es, &db),
                    out_piece(out, (size_t)n * wo[op] * es, &dout) };
    return run_pieces(h, STAGED, pc, 3, [&] {
        if (h->dtype == 32) launch_l0_eval_k<float>(h->stream, op, n, (const float*)da, (const float*)db, (float*)dout);
        else launch_l0_eval_k<double>(h->stream, op, n, (const double*)da, (const double*)db, (double*)dout);
        HIP_TRY(h, hipGetLastError());
        return (int)FBUS_OK;
    });
}

}  // extern "C"
