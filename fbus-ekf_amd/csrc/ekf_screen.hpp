// ekf_screen.hpp -- per-marker chi-square screening of a frame's marker slots (fbus_ekf_screen_markers*, include/fbus_ekf.h).
// Reference counterpart in PLACE, not in test: VISION::RejectInvalidMarker (C++/src/vision.cpp:825-853, called at :73) drops single
// detections in front of SetDetectionResult by their apparent motion; this drops them by their individual compatibility with the prior.
// Included by small_tu.hip's screen family only.  gfx950 only.
//
// Every marker slot m of every filter is judged ALONE: the rows the kind's stacked update would fold for slot m, at the current record,
//     nis_m = r_m' (H_m P H_m' + R_m)^-1 r_m = w sum res^2 - b_m' (P_JJ^-1 + Lam_m)^-1 b_m        (Lam_m, b_m: the fold's 6 x 6 sums)
// and the slot keeps its id iff nis_m <= thr[dof_m].  With P_JJ = C C' (once per filter) and K = I + C' Lam_m C = D D' the subtracted
// term is |D^-1 C' b_m|^2: pose_nis's arithmetic (ekf_device.hpp) with its first factorisation taken out of the slot loop.
//
// READ-ONLY: the kernels take the records as const, load the chunks of p, q, R and those that hold an element of P(J, J)
// (load_cov_chunks<SEL_JJ>) and store nothing but their four outputs, with plain vector stores, a tile's block of each output at once
// (ScreenStage / screen_flush).
// Mapping: one filter per lane, one wave per 64-filter tile at every batch size.  The ids of all M slots are requested in the prologue;
// a wave vote per slot then gives the wave-uniform set of ACTIVE slots -- those that carry a marker of the map on at least one live lane.
// A slot that is padding for the whole wave (16 slots with 4 in view) is passed through at once: no fetch of its measurement, no fold,
// and no load latency (the first version fetched every slot in turn and voted behind the fetch: 1.8 us per padding slot, all of it the
// round trip of a load nothing waited behind).  The loop runs over the active slots only, the next one's measurement in flight.
// ids_out may be ids: every load of the wave's ids precedes screen_flush, and a wave stores to its own tile's slots only.
#pragma once
#include "ekf_kernels.hpp"
#include "ekf_meas.hpp"

namespace {

// what depends on the filter alone: the Cholesky factor C (lower, row-major 6 x 6; a pivot that is not positive drops its column, as
// pose_nis does) of P_JJ, read from the chunks that hold it, and `poison`: 0, or NaN when P_JJ holds a non-finite value (a dropped
// pivot would otherwise hide a NaN on the diagonal)
template <typename T, int N>
__device__ __forceinline__ void screen_prior(const __amdgpu_buffer_rsrc_t rs, unsigned lane, double (&C)[36], double& poison)
{
    using RC = Rec<T, N>;
    constexpr int C_E = late_start<T, N>() / RC::EPC;
    T P[RC::NCOVP];
    load_cov_chunks<T, N, 0, C_E, SEL_JJ, AUX_NT>(rs, lane, P);
    double PJJ[36];
    poison = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double v = (double)P[pidx<N>(jcol(i), jcol(j))];
            PJJ[6 * i + j] = v; PJJ[6 * j + i] = v;
            poison = __builtin_fma(v, 0.0, poison);
        }
#pragma unroll
    for (int i = 0; i < 36; ++i) C[i] = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double piv = PJJ[6 * a + a];
#pragma unroll
        for (int k = 0; k < a; ++k) piv -= C[6 * a + k] * C[6 * a + k];
        const bool ok = piv > 0.0;
        const double is = ok ? md_rsq(piv) : 0.0;
        C[6 * a + a] = piv * is;
#pragma unroll
        for (int i = a + 1; i < 6; ++i) {
            double v = PJJ[6 * i + a];
#pragma unroll
            for (int k = 0; k < a; ++k) v -= C[6 * i + k] * C[6 * a + k];
            C[6 * i + a] = v * is;
        }
    }
}

// b' (P_JJ^-1 + Lam)^-1 b = |D^-1 C' b|^2,  D D' = I + C' Lam C  (eigenvalues >= 1: no pivoting).  Lam: upper triangle, lidx order
__device__ __forceinline__ double screen_quad(const double (&C)[36], const double* Lam, const double* b)
{
    double LC[36];                                        // Lam C
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = j; k < 6; ++k) v += Lam[i <= k ? lidx(i, k) : lidx(k, i)] * C[6 * k + j];
            LC[6 * i + j] = v;
        }
    double K[36];                                         // I + C' Lam C (lower triangle), then its Cholesky factor D in place
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double v = (i == j) ? 1.0 : 0.0;
#pragma unroll
            for (int k = i; k < 6; ++k) v += C[6 * k + i] * LC[6 * k + j];
            K[6 * i + j] = v;
        }
    double iD[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double piv = K[6 * a + a];
#pragma unroll
        for (int k = 0; k < a; ++k) piv -= K[6 * a + k] * K[6 * a + k];
        const double is = md_rsq(piv);
        iD[a] = is;
#pragma unroll
        for (int i = a + 1; i < 6; ++i) {
            double v = K[6 * i + a];
#pragma unroll
            for (int k = 0; k < a; ++k) v -= K[6 * i + k] * K[6 * a + k];
            K[6 * i + a] = v * is;
        }
    }
    double v[6], q = 0.0;                                 // v = D^-1 C' b
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double u = 0.0;
#pragma unroll
        for (int k = i; k < 6; ++k) u += C[6 * k + i] * b[k];
#pragma unroll
        for (int k = 0; k < i; ++k) u -= K[6 * i + k] * v[k];
        v[i] = u * iD[i];
        q += v[i] * v[i];
    }
    return q;
}

// The verdicts of a tile on their way out, in LDS: [slot][lane], rows padded to 65 (the flush reads them slot-fastest).  A lane's M
// values of an output are M x 4 bytes apart from its neighbour's: stored straight from the fold, every store instruction of a 16-slot
// frame touched 64 cache lines (36 such stores for 12 padding slots: 15 us of the first version's 42).  screen_flush writes the tile's
// 64 x M values of each output as one contiguous block instead, consecutive lanes to consecutive addresses.
template <typename T>
struct ScreenStage {
    static constexpr int LD = 65;
    int ids[FBUS_MAX_VISIBLE * LD], dof[FBUS_MAX_VISIBLE * LD];
    T nis[FBUS_MAX_VISIBLE * LD];
};
// the verdict of slot i of this lane's filter -> the stage.  judged: the slot's rows were formed; the decision is made on the double (a NaN
// is dropped).  Returns whether the slot is still usable
template <typename T>
__device__ __forceinline__ int screen_put(ScreenStage<T>& stg, const double* thr, int i, unsigned lane, int id, bool judged, double nis, int dof,
                                          bool in_map)
{
    const bool keep = !judged || nis <= thr[dof];
    const int o = i * ScreenStage<T>::LD + (int)lane;
    stg.ids[o] = keep ? id : -1;
    stg.nis[o] = judged ? (T)nis : T(0);
    stg.dof[o] = judged ? dof : 0;
    return keep && in_map ? 1 : 0;
}
// the stage -> ids_out, nis, dof of the tile's filters (one wave per tile: LDS operations of a wave are served in order, the barrier is
// the compiler's fence), plain vector stores
template <typename T>
__device__ __forceinline__ void screen_flush(const ScreenStage<T>& stg, const ScreenOut<T>& out, unsigned tile, unsigned lane, int B, int M)
{
    __syncthreads();
    const size_t base = (size_t)tile * 64u * (size_t)M;
    const int left = B - (int)(tile * 64u), nval = (left < 64 ? left : 64) * M;
#pragma unroll 1
    for (int e = (int)lane; e < nval; e += 64) {
        const int f = e / M, o = (e - f * M) * ScreenStage<T>::LD + f;
        if (out.ids) out.ids[base + e] = stg.ids[o];
        if (out.nis) out.nis[base + e] = stg.nis[o];
        if (out.dof) out.dof[base + e] = stg.dof[o];
    }
}

// The wave-uniform set of active slots (bit i: slot i carries a marker of the map on a live lane) from the ids IDV[16] requested in the
// prologue; the others are passed through here.  A macro for the kernels' two marker tables.  Declares nothing.
#define SCREEN_ACTIVE_SLOTS(ACT, IDV, TBL, M, LIVE, STG, THR, LANE)                                                                       \
    _Pragma("unroll") for (int i = 0; i < FBUS_MAX_VISIBLE; ++i) {                                                                        \
        if (i < M) {                                                                                                                      \
            const bool idok = IDV[i] >= 0 && IDV[i] <= FBUS_MAX_MARKER_ID;                                                                \
            const int sl = idok ? (int)TBL.id2slot[idok ? IDV[i] : 0] : -1;                                                               \
            if (__builtin_amdgcn_ballot_w64(LIVE && sl >= 0) != 0) ACT |= 1u << i;                                                        \
            else screen_put(STG, THR, i, LANE, IDV[i], false, 0.0, 0, false);                                                             \
        }                                                                                                                                 \
    }
#define SCREEN_IDS_LOAD(IDV, IDS, M, BC)                                                                                                  \
    int IDV[FBUS_MAX_VISIBLE];                                                                                                            \
    _Pragma("unroll") for (int i = 0; i < FBUS_MAX_VISIBLE; ++i) IDV[i] = IDS[(size_t)BC * M + (i < M ? i : M - 1)];

// ---- pixel rows (KIND = SCREEN_PIX_LEFT / SCREEN_PIX_STEREO) and corner rows (SCREEN_CORNERS) -------------------------------------------
// a, bb: left / right as the kind's update takes them; r_meas: r_pix / r_pos, or (noise != null: the handle's table [FBUS_NOISE_COLS][B])
// the lane's own field.  NZ: the port is square to the camera (pixel_fold_marker)
template <typename T, int N, int KIND, bool NZ>
__global__ void __launch_bounds__(64)
screen_meas_kernel(const T* __restrict__ recs, int B, int M, const int* ids, const T* __restrict__ a, const T* __restrict__ bb, int geometry,
                   double size, double r_meas, const double* __restrict__ noise, const unsigned char* __restrict__ skip,
                   const short* __restrict__ id2slot, MeasConst mc, VisConst<double> vc, VisConst<T> vct, ScreenOut<T> out)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    constexpr bool PIX = KIND != SCREEN_CORNERS;
    constexpr int CAM = KIND == SCREEN_PIX_LEFT ? 1 : 2;
    constexpr int NT = 64;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned tile = blockIdx.x;
    const int b = (int)(tile * 64u + lane);
    const bool live = b < B && !(skip && skip[b < B ? b : 0]);
    const int bc = b < B ? b : (int)(tile * 64u);
    const double rm = noise ? noise[(size_t)(PIX ? NOISE_RPIX : NOISE_RPOS) * (size_t)B + (size_t)bc] : r_meas;
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc<T, N>(recs, tile);
    __shared__ MeasLDS tbl;
    __shared__ ScreenStage<T> stg;
    using Meas = std::conditional_t<PIX, PixMeas<T, CAM>, CornerMeas<T>>;
    const bool c3d = !PIX && geometry == VIS_CORNERS3D;
    const int lw = c3d ? 12 : 8;
    auto fetch = [&](int i, Meas& mm) __attribute__((always_inline)) {
        const size_t o = (size_t)bc * M + i;
        if constexpr (PIX) { MEAS_FETCH_PIXELS(T, CAM, mm, ids, a, 8, CAM == 2 ? bb : a, o) }
        else { MEAS_FETCH_CORNERS(T, mm, ids, a, lw, c3d ? a : bb, c3d, o) }
    };
    auto corners = [&](const Meas& mm, double (&Cc)[4][3]) __attribute__((always_inline)) {
        if constexpr (!PIX) { MEAS_CORNERS_OF(T, NZ, geometry, vc, vct, mm, Cc) }
    };
    Meas cur, nxt;
    T pqr[L::NPQR];
    unsigned act = 0;
    {
        MEAS_MAP_LOAD(NT, id2slot, mc.mkc, tbl)
        order_fence();
        SCREEN_IDS_LOAD(idv, ids, M, bc)
        fetch(0, cur);                                              // (on the guess that slot 0 is active: the usual frame)
        order_fence();
        load_chunks<T, N, 0, RC::CH_PQR>(rs, lane, pqr);
        order_fence();
        MEAS_MAP_STORE(NT)
        order_fence();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        SCREEN_ACTIVE_SLOTS(act, idv, tbl, M, live, stg, out.thr, lane)
    }
    if (act && !(act & 1u)) fetch(__builtin_ctz(act), cur);         // (the guess was wrong: in flight under the factorisation)
    order_fence();
    // what depends on the filter alone
    double Cf[36], poison;
    screen_prior<T, N>(rs, lane, Cf, poison);
    double pd[3], Rd[9];
    MEAS_POSE_OF(L, pqr, mc, pd, Rd, pil)
#pragma unroll
    for (int i = 0; i < 3; ++i) poison = __builtin_fma(pd[i], 0.0, poison);
#pragma unroll
    for (int i = 0; i < 9; ++i) poison = __builtin_fma(Rd[i], 0.0, poison);
    double RM[9];                                                   // (the left-only fold of the square port runs in the camera frame)
    if constexpr (KIND == SCREEN_PIX_LEFT && NZ) PixAcc::camera_rotation(Rd, mc.McL, RM);
    const double w = 1.0 / rm;
    int kept = 0;
#pragma unroll 1
    while (act) {
        const int i = __builtin_ctz(act);
        act &= act - 1;
        fetch(act ? __builtin_ctz(act) : i, nxt);                   // always a fresh load (no conditional merge of the two records)
        const bool idok = cur.id >= 0 && cur.id <= FBUS_MAX_MARKER_ID;
        const int slot = idok ? (int)tbl.id2slot[idok ? cur.id : 0] : -1;
        const bool in_map = live && slot >= 0;
        PixAcc acc;
        acc.clear();
        acc.clear_nis();
        double Lam[21], bv[6];
        if constexpr (PIX) {
            double nfold = 0.0;
            MEAS_FOLD_PIXEL_SLOT(T, NZ, CAM, true, acc, nfold, tbl, cur, CAM == 2, pd, Rd, pil, mc, size)
            if constexpr (KIND == SCREEN_PIX_LEFT && NZ) { acc.to_imu_frame(mc.adjL); acc.finish(RM, w, Lam, bv); }
            else acc.finish(Rd, w, Lam, bv);
        } else {
            auto fold_marker = [&](const Meas& mm) __attribute__((always_inline)) {
                MEAS_FOLD_CORNER_SLOT(true, acc, tbl, mm, corners, pd, Rd, pil, mc, size)
            };
            if (in_map) fold_marker(cur);
            acc.expand_const(mc.NI);
            acc.finish(Rd, w, Lam, bv);
        }
        const double nisv = (w * acc.sr2 - screen_quad(Cf, Lam, bv)) + poison;
        const int dofv = (int)acc.nrow;
        // pixel rows: a marker wholly out of view has no rows and is not judged -- unless the record itself is not finite
        const bool judged = in_map && (dofv > 0 || poison != poison);
        kept += screen_put(stg, out.thr, i, lane, cur.id, judged, nisv, dofv, in_map);
        cur = nxt;
    }
    screen_flush(stg, out, tile, lane, B, M);
    if (b < B && out.kept) out.kept[b] = kept;
}

// ---- pose rows: 3 (Matlab dialect: all 7 rows in S, the quaternion residual zeroed) or 7 (C++ dialect) per marker ---------------------------
// noise: null, or the handle's table (this lane's r_pos / r_quat in place of dc's)
template <typename T, int N, int DIALECT>
__global__ void __launch_bounds__(64)
screen_pose_kernel(const T* __restrict__ recs, int B, int M, const int* ids, const T* __restrict__ pos, const T* __restrict__ quat,
                   const double* __restrict__ noise, const unsigned char* __restrict__ skip, DevConst<T> dc, ScreenOut<T> out)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    constexpr int ROWS = DIALECT == DIALECT_CPP ? 7 : 3;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned tile = blockIdx.x;
    const int b = (int)(tile * 64u + lane);
    const bool live = b < B && !(skip && skip[b < B ? b : 0]);
    const int bc = b < B ? b : (int)(tile * 64u);
    if (noise) {
        dc.r_pos = (T)noise[(size_t)NOISE_RPOS * (size_t)B + (size_t)bc];
        dc.r_quat = (T)noise[(size_t)NOISE_RQUAT * (size_t)B + (size_t)bc];
    }
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc<T, N>(recs, tile);
    __shared__ MarkerLDS<T> tbl;
    __shared__ ScreenStage<T> stg;
    T pqr[L::NPQR];
    struct Slot { int id; T y[7]; };
    auto fetch = [&](int i, Slot& s) __attribute__((always_inline)) {
        const size_t o = (size_t)bc * M + i;
        s.id = ids[o];
#pragma unroll
        for (int k = 0; k < 3; ++k) s.y[k] = ld_once(pos + 3 * o + k);
#pragma unroll
        for (int k = 0; k < 4; ++k) s.y[3 + k] = ld_once(quat + 4 * o + k);
    };
    Slot cur, nxt;
    unsigned act = 0;
    {
        MarkerTableRegs<T> treg;
        treg.load(dc);
        order_fence();
        SCREEN_IDS_LOAD(idv, ids, M, bc)
        fetch(0, cur);                                              // (on the guess that slot 0 is active: the usual frame)
        order_fence();
        load_chunks<T, N, 0, RC::CH_PQR>(rs, lane, pqr);
        order_fence();
        treg.to_lds(tbl);
        order_fence();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        SCREEN_ACTIVE_SLOTS(act, idv, tbl, M, live, stg, out.thr, lane)
    }
    if (act && !(act & 1u)) fetch(__builtin_ctz(act), cur);         // (the guess was wrong: in flight under the factorisation)
    order_fence();
    double Cf[36], poison;
    screen_prior<T, N>(rs, lane, Cf, poison);
#pragma unroll
    for (int i = 0; i < L::NPQR; ++i) poison = __builtin_fma((double)pqr[i], 0.0, poison);
    const double wp = (double)fb_rcp1(dc.r_pos), wq = (double)fb_rcp1(dc.r_quat);
    int kept = 0;
#pragma unroll 1
    while (act) {
        const int i = __builtin_ctz(act);
        act &= act - 1;
        fetch(act ? __builtin_ctz(act) : i, nxt);                   // always a fresh load (no conditional merge of the two records)
        const bool idok = cur.id >= 0 && cur.id <= FBUS_MAX_MARKER_ID;
        const int slot = idok ? (int)tbl.id2slot[idok ? cur.id : 0] : -1;
        const bool in_map = live && slot >= 0;
        POSE_SLOT_MK(T, mk, tbl, (slot >= 0 ? slot : 0))
        InfoAcc<T> acc;
        PoseFold<T, N, DIALECT, true> fold;
        POSE_FOLD_ONE_MARKER(T, N, true, acc, fold, mk, pqr, dc, cur.y)
        double Lam[21], bv[6];
#pragma unroll
        for (int k = 0; k < 21; ++k) Lam[k] = (double)acc.Lam[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) bv[k] = (double)acc.b[k];
        const double sumw = wp * fold.sr2p + (DIALECT == DIALECT_CPP ? wq * fold.sr2q : 0.0);
        const double nisv = (sumw - screen_quad(Cf, Lam, bv)) + poison;
        kept += screen_put(stg, out.thr, i, lane, cur.id, in_map, nisv, ROWS, in_map);
        cur = nxt;
    }
    screen_flush(stg, out, tile, lane, B, M);
    if (b < B && out.kept) out.kept[b] = kept;
}

}  // namespace

namespace fbus {
// grid: one wave per tile
template <typename T, int N, int KIND>
void launch_screen_meas_k(hipStream_t st, const T* recs, int B, int M, const int* ids, const T* a, const T* bb, int geometry, bool square_port,
                          double size, double r_meas, const double* noise, const unsigned char* skip, const short* id2slot,
                          const MeasConst& mc, const VisConst<double>& vc, const VisConst<T>& vct, const ScreenOut<T>& out)
{
    const dim3 grid((B + 63) / 64), block(64);
    if (square_port)
        hipLaunchKernelGGL((screen_meas_kernel<T, N, KIND, true>), grid, block, 0, st, recs, B, M, ids, a, bb, geometry, size, r_meas, noise,
                           skip, id2slot, mc, vc, vct, out);
    else
        hipLaunchKernelGGL((screen_meas_kernel<T, N, KIND, false>), grid, block, 0, st, recs, B, M, ids, a, bb, geometry, size, r_meas, noise,
                           skip, id2slot, mc, vc, vct, out);
}
template <typename T, int N, int DIALECT>
void launch_screen_pose_k(hipStream_t st, const T* recs, int B, int M, const int* ids, const T* pos, const T* quat, const double* noise,
                          const unsigned char* skip, const DevConst<T>& dc, const ScreenOut<T>& out)
{
    hipLaunchKernelGGL((screen_pose_kernel<T, N, DIALECT>), dim3((B + 63) / 64), dim3(64), 0, st, recs, B, M, ids, pos, quat, noise, skip, dc,
                       out);
}
}  // namespace fbus
