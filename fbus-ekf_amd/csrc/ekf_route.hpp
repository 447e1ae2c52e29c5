// ekf_route.hpp -- which kernels a call runs: the launch policy of the handle as pure host functions.
//
// Plain C++17: nothing from HIP and nothing from the other headers here, so that a host compiler can build the policy alone
// (tests/test_route_cpu.py walks it).  fbus_ekf.hip fills a RouteKey from the handle (route_key), asks for the route of a frame or a
// window ONCE, after the arguments are checked and before the first launch, and switches on the answer; the launch functions are the
// bodies of single routes.  DESIGN.md 5.1 holds the table these functions compute.
#pragma once

namespace fbus {

// The values of include/fbus_ekf.h that the policy reads (fbus_ekf.hip asserts that they agree)
enum { ROUTE_MODE_NEAREST = 0, ROUTE_MODE_STACKED = 1 };
enum RouteKind { ROUTE_POSE = -1, ROUTE_PIXELS = 0, ROUTE_CORNERS = 1 };    // the rows of a frame: marker poses, corner pixels, stereo corners

// What the policy reads of a handle, and nothing else
struct RouteKey {
    int dtype = 32;                 // record type: 32 | 64
    bool joseph = false;            // covariance form: fbus_params::cov_form == FBUS_COV_JOSEPH
    bool noise_on = false;          // a per-filter noise table is set (fbus_ekf_set_noise)
    bool lik_on = false;            // the likelihood sums are on (fbus_ekf_loglik_enable)
    int tiles = 1;                  // the POLICY batch in 64-filter tiles (the handle's own batch unless fbus_ekf_set_policy_batch names the job)
    int simds = 1024;               // SIMDs of the device
    int team_predict = 0;           // fbus_ekf_set_team / FBUS_TEAM_PREDICT: 0 = by size, 1 = never, 2..4 = always with that many roles
    int team_correct = 0;           // ... / FBUS_TEAM_CORRECT
    int team_frame = 0;             // FBUS_TEAM_FRAME: 0 = follows team_predict, 1 = never, 2 = always
    int meas_split = -1;            // FBUS_MEAS_SPLIT: -1 auto, 0 never, 2 / 4 = always the divided-update pixel kernel with that many waves
    bool no_frame_meas = false;     // FBUS_NO_FRAME_MEAS=1: the measurement frames always as predict_n + the per-call update
    bool square_port = true;        // the port is square to the camera (port normal (0, 0, 1))
};

// How many waves should share one 64-filter tile?  One wave per tile (the lane-per-filter kernels) fills the chip from
// 1024 tiles on; below that the SIMDs that would idle can take a share of every filter's work instead (ekf_team.hpp).
// Measured (rocprofv3 kernel trace, profiles/r03_team_kernels.txt), one-wave -> team:
//   predict    4096 filters 4.52 -> 4.00 us (3 roles), 16 384: 4.80 -> 4.52, 32 768: 6.4 -> 8.8 (the roles' overlapping loads cost
//              more than the shorter instruction streams save once the launch moves 47 MB)            => up to 256 tiles
//   predict_n  K = 8: 4096 filters 18.8 -> 10.3 us, 16 384: 20.7 -> 17.5, 32 768: 23.2 -> 20.9                 => up to 512 tiles
//   correct    4096 filters 6.4 -> 7.6 us, 16 384: 7.2 -> 9.2, 32 768: 10.0 -> 18: the one-wave kernel folds its markers under
//              the load latency and the team pays two exchanges and a redundant 6 x 6 solve per role       => never by default
// (round 4) The thresholds are fractions of the device's SIMD count (256 / 512 tiles = a quarter / half of MI355X's 1024 SIMDs: what
// was measured is "how much of the chip a one-wave launch leaves idle"), and the batch they are compared with is the POLICY batch:
// the handle's own unless fbus_ekf_set_policy_batch names the whole job -- team and one-wave kernels agree to fp32 rounding only,
// so a job cut into shards (fbus::ShardedFilter) keys the choice on the total and gets the same kernels whatever the shard layout.
// RouteKey::tiles: all the policy sees of the batch -- the policy batch where one is set (fbus_ekf_set_policy_batch), else the handle's own
inline int tiles_of(int filters) { return (filters + 63) / 64; }
inline int policy_tiles_of(int policy_batch, int B) { return tiles_of(policy_batch > 0 ? policy_batch : B); }
// the measurement updates read the noise table: one set by the caller, or the handle's own row while the likelihood sums are on
inline bool tabled(const RouteKey& k) { return k.noise_on || k.lik_on; }
inline int policy_tiles(const RouteKey& k) { return k.tiles; }
inline int quarter_chip(const RouteKey& k) { return k.simds / 4; }
inline int half_chip(const RouteKey& k) { return k.simds / 2; }
// A noise table and the resident windows (frames_kernel / frame_meas_kernel with (TrajOut, NoiseIn): kernels_tu.hip families 19 / 20).
// The fused frames and the frame windows of a tabled handle take them exactly where an untabled handle of the same policy batch runs
// the ONE-WAVE resident kernels: fp32 records, more than half a chip of tiles.  A pure size rule on the policy batch (fbus_ekf_set_team
// stays ignored while a table is set; the shards of a job agree with the unsharded run).  At or below half a chip, where untabled
// handles take the team forms, and while the likelihood sums are on (no resident kernel feeds them): frame by frame through the per-call
// kernels.  What a single call can still exclude -- (Joseph, nearest) pose rows, M = 0, FBUS_NO_FRAME_MEAS -- is excluded as without a table.
inline bool noise_resident(const RouteKey& k) { return k.noise_on && !k.lik_on && k.dtype == 32 && policy_tiles(k) > half_chip(k); }
inline int team_roles_predict(const RouteKey& k, int K)
{
    if (k.dtype != 32 || k.team_predict == 1 || tabled(k)) return 1;        // (a noise table, likelihood sums: the one-wave forms only)
    if (k.team_predict >= 2) return K > 1 ? 4 : (k.team_predict > 4 ? 4 : k.team_predict);
    const int tiles = policy_tiles(k);
    if (K > 1) return tiles <= half_chip(k) ? 4 : 1;
    return tiles <= quarter_chip(k) ? 3 : 1;
}
// correct from stereo corners (stacked mode) / from corner pixels (ekf_meas.hpp: the markers of a filter divided among the roles; these
// kernels are bound by the VALU work per marker).  fbus_ekf_set_team's correct_roles: 1 = never, 2 = two roles, 3..4 = four;
// 0 = four up to a quarter of the chip, two up to half.  Both record types.
inline int team_roles_pixels(const RouteKey& k, int M)
{
    if (M < 2 || k.team_correct == 1 || tabled(k)) return 1;
    if (k.team_correct >= 2) return k.team_correct >= 3 ? 4 : 2;
    const int tiles = policy_tiles(k);
    return tiles <= quarter_chip(k) ? 4 : (tiles <= half_chip(k) ? 2 : 1);
}
// (round 5) correct_pixels with the UPDATE divided between the waves of a tile as well (ekf_meas_split.hpp: a solver and an updater wave,
// every wave below 256 registers): 0 = not this launch (the one-wave-tail kernel with team_roles_pixels' fold roles), 2 = two waves per
// tile (from a quarter of the chip on, full-chip launches included: two waves per SIMD there), 4 = four (small launches).  fp32
// records and the port square to the camera only; fbus_ekf_set_team's correct_roles = 1 keeps the one-wave kernel.
inline int meas_split_roles(const RouteKey& k, int M)
{
    if (k.dtype != 32 || M < 2 || k.team_correct == 1 || k.meas_split == 0 || tabled(k)) return 0;
    if (!k.square_port) return 0;
    if (k.meas_split > 0) return k.meas_split;
    if (k.team_correct >= 2) return k.team_correct >= 3 ? 4 : 2;
    const int tiles = policy_tiles(k);
    return tiles <= quarter_chip(k) ? 4 : (tiles <= half_chip(k) ? 2 : 0);
}
// fused frame / frame window (frames_team_kernel: the predict_n pipeline + the one-shot correct divided over the four roles).  Follows the predict
// setting (fbus_ekf_set_team: 1 = never, 2..4 = always); FBUS_TEAM_FRAME=1|2 overrides.  Two workgroups of four waves fit a CU
// (80 KiB of LDS, 250 registers), so the automatic choice ends at 512 tiles (profiles/logs/r03_team_frame.txt: +8 % / +12 % at
// 32 768 filters, 0.8x at 40 960).
inline bool team_frames(const RouteKey& k, int mode)
{
    if (k.dtype != 32 || k.joseph || tabled(k)) return false;
    if (mode != ROUTE_MODE_NEAREST && mode != ROUTE_MODE_STACKED) return false;
    if (k.team_frame == 1 || (k.team_frame == 0 && k.team_predict == 1)) return false;
    if (k.team_frame == 2 || k.team_predict >= 2) return true;
    return policy_tiles(k) <= half_chip(k);
}
// (round 4, measured and NOT kept: a batch of more than one wave per SIMD as launches of one round each.  The per-call kernels run
// 65 536 filters -- 52 MB of records, exactly one wave per SIMD -- at 7.7 TB/s because the records stay cache-resident from launch
// to launch; two such launches over the two halves of 131 072 filters do NOT run at twice 12.2 us (29.1 us against 28.0 us for the
// single launch, 60.7 against 55.8 at 262 144: tools/r4_by_batch.sh, profiles/r04_bench_by_batch.txt) -- what is lost past 65 536
// filters is the residency (56 MB, section 4.1 of DESIGN.md), not the launch shape, and beyond it the kernels stream at the
// 6.3-6.7 TB/s this part copies at.)

// ---- one camera frame ---------------------------------------------------------------------------------------------------------------------
// K predicts and the update of M marker slots: fbus_ekf_frame_fused_dev (pose rows), fbus_ekf_frame_meas_fused_dev (pixels, corners), and
// every frame of a window that runs frame by frame.
enum FrameRoute {
    FRAME_PER_CALL,         // predict_n (K > 0) + the per-call update (M > 0): two launches, the same arithmetic
    FRAME_F64_FUSED,        // frame2_kernel<double>: the one fused kernel of fp64 records
    FRAME_FUSED,            // the fp32 fused frame kernel, one wave per tile (K beyond a byte included)
    FRAME_TEAM,             // frames_team_kernel with F = 1
    FRAME_TABLED_RESIDENT,  // the resident WINDOW kernel with (TrajOut, NoiseIn) and F = 1: a tabled window is bit-equal to its frames by construction
    FRAME_MEAS_RESIDENT,    // frame_meas_kernel, F = 1
};
// The resident kernels count a frame's samples in a byte
constexpr int ROUTE_MAX_RESIDENT_K = 255;
// mode: of the pose rows and of the corner rows (the pixel rows have none).
inline FrameRoute frame_route(const RouteKey& k, RouteKind kind, int mode, int M, int K)
{
    const bool byte_k = K <= ROUTE_MAX_RESIDENT_K;
    // a tabled handle: the size rule alone (noise_resident), and what excludes the call without a table excludes it here too
    if (tabled(k) && !(noise_resident(k) && byte_k)) return FRAME_PER_CALL;
    if (kind == ROUTE_POSE) {
        // no fused kernel for fp64 outside (stacked, simple) and none for the Joseph form with the reference mode's 7 row-by-row
        // updates (it spilled)
        if (k.joseph && mode != ROUTE_MODE_STACKED) return FRAME_PER_CALL;
        if (k.dtype != 32) return (mode == ROUTE_MODE_STACKED && !k.joseph && K > 0 && byte_k) ? FRAME_F64_FUSED : FRAME_PER_CALL;
        if (tabled(k)) return FRAME_TABLED_RESIDENT;
        return team_frames(k, mode) && byte_k ? FRAME_TEAM : FRAME_FUSED;
    }
    // ONE launch (frame_meas_kernel: record resident, covariance parked in LDS across the fold) where the per-call update would run one
    // wave per tile anyway -- fp32 records, more than half a chip of tiles (or fbus_ekf_set_team(., 1)); otherwise predict_n + the
    // per-call update, whose team forms fill a small launch better than one resident wave per tile could (fp64 records: the resident
    // fold + covariance do not fit 512 registers)
    if (k.dtype != 32 || M <= 0 || k.no_frame_meas || !byte_k) return FRAME_PER_CALL;
    if (tabled(k)) return FRAME_TABLED_RESIDENT;
    const int roles = (kind == ROUTE_CORNERS && mode != ROUTE_MODE_STACKED) ? 1 : team_roles_pixels(k, M);
    return roles == 1 ? FRAME_MEAS_RESIDENT : FRAME_PER_CALL;
}

// ---- a window of frames -------------------------------------------------------------------------------------------------------------------
// fbus_ekf_frames_fused[_traj]_dev (pose rows) and fbus_ekf_frames_meas_fused[_traj]_dev (a measurement window of ONE frame is not asked:
// it runs as that frame).  Every kcount of a window fits a byte.
enum WindowRoute {
    WINDOW_ONE_WAVE,        // one resident launch, one wave per tile; writes the trajectory rows itself
    WINDOW_TEAM,            // one resident launch of the team kernel (no trajectory rows)
    WINDOW_TEAM_FRAMES,     // the team window with rows: one-frame team launches, each followed by the snapshot
    WINDOW_BY_FRAME,        // frame by frame through frame_route, each followed by the snapshot where rows are asked for
};
inline WindowRoute window_route(const RouteKey& k, RouteKind kind, int mode, int M, bool with_traj)
{
    // a window is resident exactly where every frame of it would be: the premise of window == frames, bit for bit
    const FrameRoute f = frame_route(k, kind, mode, M, 1);
    if (f == FRAME_PER_CALL || f == FRAME_F64_FUSED) return WINDOW_BY_FRAME;
    if (f == FRAME_TEAM) return with_traj ? WINDOW_TEAM_FRAMES : WINDOW_TEAM;
    return WINDOW_ONE_WAVE;
}

// The trailing pack of the one-wave window kernels (frames_kernel, frame_meas_kernel), asked with their routes only: (TrajOut, NoiseIn) on
// the tabled resident route (without rows: three null pointers), (TrajOut) when rows are asked for, else none.
enum WindowPack { PACK_NONE, PACK_TRAJ, PACK_TRAJ_NOISE };
inline WindowPack window_pack(const RouteKey& k, bool with_traj)
{
    return noise_resident(k) ? PACK_TRAJ_NOISE : (with_traj ? PACK_TRAJ : PACK_NONE);
}

}  // namespace fbus
