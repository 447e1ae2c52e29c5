// ekf_project.hpp -- where the corners of the map's markers appear in the images, and how uncertain that is (fbus_ekf_project_markers*,
// include/fbus_ekf.h): the flat-port measurement model h(x) of the pixel updates as an OUTPUT, with the innovation covariance
// S = H P_JJ H' + r_pix I of every projection and the per-corner visibility.
// Reference counterpart in PLACE, not in test: the front end searches the whole image and rejects detections by apparent motion
// (C++/src/vision.cpp:825-853); a filter with a covariance can say where to look.
// Included by small_tu.hip's screen family only.  gfx950 only.
//
// READ-ONLY: the kernels take the records as const, load the chunks of p, q, R and -- only when a covariance is asked for -- those that
// hold an element of P(J, J) (load_cov_chunks<SEL_JJ>), and store nothing but their outputs, with plain vector stores.
// Mapping (as ekf_screen.hpp): one filter per lane, one wave per 64-filter tile at every batch size.  The ids of all M slots are requested
// in the prologue; a wave vote per slot gives the wave-uniform set of ACTIVE slots -- those that carry a marker of the map on a live lane.
// A slot that is padding for the whole wave gets its zeros at once and no projection.
//
// The projection is a SECOND COPY of the geometry of pixel_fold_marker (ekf_meas.hpp), built from the same primitives (port_start_f32,
// port_eval_n, md_rsq_n, md_rcp_n, MeasConst) in the same order of operations: the update kernels sit at their register limits and are
// pinned bit for bit, so they are not touched here.  What differs: the image point and the rows are kept instead of folded, nothing is
// measured, and the rows are always the image-frame ones (the left-only update of the square port folds them rotated into the radial /
// tangential directions, which rotates S).  Four projections in lock step: the four corners of the left camera, or two corners x two
// cameras twice (as pixel_fold_marker_stereo_halves).
//
// The covariance: a row of H is [ -(R a)' | (a x ru)' ] with a = (J_q M_c)' in the IMU frame and ru = R'(c_w - p).  What depends on the
// filter alone is hoisted (project_prior): A = R' P_pp R, Bm = R' P_pt, Tt = P_tt.  With c = a x ru, g = A a - Bm c, k = Tt c - Bm' a,
//     S_rs = a_s . g_r + c_s . k_r + (r == s) r_pix
// -- two short quadratic forms per projection, in double for both record types.
//
// Stores: a lane stores its own filter's values straight from registers, 16 bytes per instruction: a slot's eight coordinates are 32 / 64
// contiguous bytes, a camera's twelve covariance entries 96.  (A tile's slot staged through LDS, as ScreenStage does for 4-byte values,
// cannot make them denser: the values of two filters are M x 32 bytes apart in memory whatever lane writes them, so an instruction
// touches as many 32-byte sectors either way)
#pragma once
#include "ekf_kernels.hpp"
#include "ekf_meas.hpp"

namespace {

// P_JJ in the frame the rows a live in: A = R' P_pp R (symmetric, 00 01 02 11 12 22), Bm = R' P_pt (row-major 3 x 3), Tt = P_tt (symmetric)
struct ProjPrior { double A[6], Bm[9], Tt[6]; };

template <typename T, int N>
__device__ __forceinline__ void project_prior(const __amdgpu_buffer_rsrc_t rs, unsigned lane, const double* R, ProjPrior& pri)
{
    using RC = Rec<T, N>;
    constexpr int C_E = late_start<T, N>() / RC::EPC;
    T P[RC::NCOVP];
    load_cov_chunks<T, N, 0, C_E, SEL_JJ, AUX_NT>(rs, lane, P);
    double Ppp[9], Ppt[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Ppp[3 * i + j] = (double)P[i <= j ? pidx<N>(jcol(i), jcol(j)) : pidx<N>(jcol(j), jcol(i))];
            Ppt[3 * i + j] = (double)P[pidx<N>(jcol(i), jcol(3 + j))];
        }
    {
        int o = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) pri.Tt[o++] = (double)P[pidx<N>(jcol(3 + i), jcol(3 + j))];
    }
    double T1[9];                                         // P_pp R
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T1[3 * i + j] = Ppp[3 * i] * R[j] + Ppp[3 * i + 1] * R[3 + j] + Ppp[3 * i + 2] * R[6 + j];
    {
        int o = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) pri.A[o++] = R[i] * T1[j] + R[3 + i] * T1[3 + j] + R[6 + i] * T1[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) pri.Bm[3 * i + j] = R[i] * Ppt[j] + R[3 + i] * Ppt[3 + j] + R[6 + i] * Ppt[6 + j];
}

// NV values of T (a multiple of 16 bytes) at dst, which is 16-byte aligned: 16 bytes per store
template <typename T, int NV>
__device__ __forceinline__ void project_store(T* dst, const T (&v)[NV])
{
    constexpr int EP = 16 / (int)sizeof(T);
    static_assert(NV % EP == 0, "whole 16-byte pieces");
#pragma unroll
    for (int c = 0; c < NV / EP; ++c) {
        u32x4 w;
        T* e = reinterpret_cast<T*>(&w);
#pragma unroll
        for (int k = 0; k < EP; ++k) e[k] = v[c * EP + k];
        reinterpret_cast<u32x4*>(dst)[c] = w;
    }
}

// NK corners (K0 .. K0 + NK - 1) x NCAM cameras of one marker, projection q = k NCAM + c as in pixel_fold_marker, whose stages these are.
// -> ok[q]: in view; uv[q]: the image point; S[q] = (S_uu, S_uv, S_vv) when cov.  Out of view: a harmless point is projected in its place
// (everything stays finite); the caller clears its outputs.
template <int NCAM, typename T, bool NZ, int NK, int K0>
__device__ __forceinline__ void project_corners(const double* p, const double* R, const double* pil, const MeasConst& mc, const double* mkc,
                                                double size, bool cov, const ProjPrior& pri, double rpix, bool (&ok)[NK * NCAM],
                                                double (&uv)[NK * NCAM][2], double (&S)[NK * NCAM][3])
{
    constexpr int NS = sizeof(T) == 8 ? 2 : 1;           // Newton steps behind v_rsq_f64 / v_rcp_f64
    constexpr int NP = NK * NCAM;
    double ru[4][3], rAx[3], rAy[3];
    {
        double u0[3], ru0[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) u0[i] = mkc[i] - p[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            ru0[i] = R[i] * u0[0] + R[3 + i] * u0[1] + R[6 + i] * u0[2];                                   // R'(C0 - p)
            rAx[i] = size * (R[i] * mkc[3] + R[3 + i] * mkc[4] + R[6 + i] * mkc[5]);
            rAy[i] = size * (R[i] * mkc[6] + R[3 + i] * mkc[7] + R[6 + i] * mkc[8]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            ru[0][i] = ru0[i];
            ru[1][i] = ru0[i] + rAy[i];
            ru[2][i] = ru0[i] + rAx[i] + rAy[i];
            ru[3][i] = ru0[i] + rAx[i];
        }
    }
    const double* n = mc.n;
    double lat[NP][3], rho[NP], irho[NP], Wd[NP], t[NP];
    bool offax[NP];
    {
        double X[NP][3], z[NP], r2[NP], zwq[NP], r2s[NP], xs[NP], ir0[NP], zsq[NP];
#pragma unroll
        for (int c = 0; c < NCAM; ++c) {
            const double* M = c ? mc.McR : mc.McL;
            const double tI[3] = { ru[0][0] - pil[0], ru[0][1] - pil[1], ru[0][2] - pil[2] };
            double X0[3], MAx[3], MAy[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                X0[i] = M[3 * i] * tI[0] + M[3 * i + 1] * tI[1] + M[3 * i + 2] * tI[2] + (c ? mc.tR[i] : 0.0);
                MAx[i] = M[3 * i] * rAx[0] + M[3 * i + 1] * rAx[1] + M[3 * i + 2] * rAx[2];
                MAy[i] = M[3 * i] * rAy[0] + M[3 * i + 1] * rAy[1] + M[3 * i + 2] * rAy[2];
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int kk = K0 + k;                   // corner 0: X0, 1: X0 + MAy, 2: (X0 + MAy) + MAx, 3: X0 + MAx
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    X[k * NCAM + c][i] = kk == 0 ? X0[i] : (kk == 1 ? X0[i] + MAy[i] : (kk == 2 ? X0[i] + MAy[i] + MAx[i] : X0[i] + MAx[i]));
            }
        }
        if constexpr (NZ) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                z[q] = X[q][2];
                lat[q][0] = X[q][0]; lat[q][1] = X[q][1]; lat[q][2] = 0.0;
                r2[q] = X[q][0] * X[q][0] + X[q][1] * X[q][1];
                zwq[q] = z[q] - (mc.d_air + mc.d_glass);
            }
        } else {
#pragma unroll
            for (int q = 0; q < NP; ++q) z[q] = X[q][0] * n[0] + X[q][1] * n[1] + X[q][2] * n[2];
#pragma unroll
            for (int q = 0; q < NP; ++q)
#pragma unroll
                for (int i = 0; i < 3; ++i) lat[q][i] = X[q][i] - z[q] * n[i];
#pragma unroll
            for (int q = 0; q < NP; ++q) { r2[q] = lat[q][0] * lat[q][0] + lat[q][1] * lat[q][1] + lat[q][2] * lat[q][2]; zwq[q] = z[q] - mc.d_air - mc.d_glass; }
        }
        // in front of the port and inside its field of view (both comparisons are false for a NaN)
        const double klim = mc.klim;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            ok[q] = (zwq[q] > 0.0) & (r2[q] < klim * zwq[q] * zwq[q]);
            r2s[q] = ok[q] ? r2[q] : 0.0;
            zsq[q] = ok[q] ? zwq[q] : 1.0;
            Wd[q] = zsq[q] * mc.a1;
            xs[q] = r2s[q] > 0.0 ? r2s[q] : 1.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) lat[q][i] = ok[q] ? lat[q][i] : 0.0;
        }
        md_rsq_n<NS, NP>(xs, ir0);
#pragma unroll
        for (int q = 0; q < NP; ++q) { offax[q] = r2s[q] > 0.0; irho[q] = ir0[q]; rho[q] = r2s[q] * irho[q]; }
        port_start_f32<NP>(mc, rho, zsq, t);
    }
    double iLt[NP], c2[NP];
    {
        constexpr int NFIN = sizeof(T) == 8 ? 2 : 1;
        PortEvalN<double, NP> f;
        const double Gd = mc.d_glass * mc.a0;
#pragma unroll
        for (int rep = 0; rep < NFIN; ++rep) {
            port_eval_n<NS, double, NP>(mc.a0, mc.a1, mc.d_air, Gd, Wd, rho, t, f);
#pragma unroll
            for (int q = 0; q < NP; ++q) t[q] = fmax(t[q] + f.dt[q], 0.0);
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) { f.Lt[q] += f.Ltt[q] * f.dt[q]; f.Lz[q] += f.Lzt[q] * f.dt[q]; }
        md_rcp_n<NS, NP>(f.Lt, iLt);
#pragma unroll
        for (int q = 0; q < NP; ++q) c2[q] = f.Lz[q] * iLt[q];
    }
    double kk[NP], a[NP][2][3];
#pragma unroll
    for (int q = 0; q < NP; ++q) kk[q] = offax[q] ? t[q] * irho[q] : iLt[q];                 // t / rho; on the axis its limit 1 / L_t
    if constexpr (NZ) {
        double e[NP][2], eM[NP][3];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            uv[q][0] = kk[q] * lat[q][0];
            uv[q][1] = kk[q] * lat[q][1];
            e[q][0] = lat[q][0] * irho[q];
            e[q][1] = lat[q][1] * irho[q];
        }
        if (!cov) return;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const double* M = (q % NCAM) ? mc.McR : mc.McL;
#pragma unroll
            for (int j = 0; j < 3; ++j) eM[q][j] = e[q][0] * M[j] + e[q][1] * M[3 + j];
        }
        // a_r = c1 e_r (e'M) + k M_r - c2 e_r M_z
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const double* M = (q % NCAM) ? mc.McR : mc.McL;
            const double c1v = iLt[q] - kk[q], c2v = c2[q], kv = kk[q];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const double w1 = c1v * e[q][r], w3 = -c2v * e[q][r];
#pragma unroll
                for (int j = 0; j < 3; ++j) a[q][r][j] = w1 * eM[q][j] + kv * M[3 * r + j] + w3 * M[6 + j];
            }
        }
    } else {
        double Dz[NP], iDz[NP], e[NP][3], eM[NP][3];
#pragma unroll
        for (int q = 0; q < NP; ++q) Dz[q] = n[2] + kk[q] * lat[q][2];
        md_rcp_n<NS, NP>(Dz, iDz);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            uv[q][0] = (n[0] + kk[q] * lat[q][0]) * iDz[q];
            uv[q][1] = (n[1] + kk[q] * lat[q][1]) * iDz[q];
#pragma unroll
            for (int i = 0; i < 3; ++i) e[q][i] = lat[q][i] * irho[q];
        }
        if (!cov) return;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const double* M = (q % NCAM) ? mc.McR : mc.McL;
#pragma unroll
            for (int j = 0; j < 3; ++j) eM[q][j] = e[q][0] * M[j] + e[q][1] * M[3 + j] + e[q][2] * M[6 + j];
        }
        // rows: J_r = alpha e' + beta n' + k g',  g = (unit_r - uv_r unit_z) / D_z;  a = (J_r Mc)'
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int c = q % NCAM;
            const double* M = c ? mc.McR : mc.McL;
            const double* nM = c ? mc.nMR : mc.nML;
            const double c1 = iLt[q] - kk[q];
            const double kz = kk[q] * iDz[q];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const double ge = (e[q][r] - uv[q][r] * e[q][2]) * iDz[q], gn = (n[r] - uv[q][r] * n[2]) * iDz[q];
                const double am = ge * c1, bm = -(c2[q] * ge + kk[q] * gn);
#pragma unroll
                for (int j = 0; j < 3; ++j) a[q][r][j] = am * eM[q][j] + bm * nM[j] + kz * (M[3 * r + j] - uv[q][r] * M[6 + j]);
            }
        }
    }
    // S = H P_JJ H' + r_pix I per projection, H = [ -(R a)' | (a x ru)' ] (see the head of this file)
    const double* A = pri.A; const double* Bm = pri.Bm; const double* Tt = pri.Tt;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const double* r = ru[K0 + q / NCAM];
        double c[2][3], g[2][3], k[2][3];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double* as = a[q][s];
            c[s][0] = as[1] * r[2] - as[2] * r[1];
            c[s][1] = as[2] * r[0] - as[0] * r[2];
            c[s][2] = as[0] * r[1] - as[1] * r[0];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double* as = a[q][s];
            const double* cs = c[s];
            g[s][0] = A[0] * as[0] + A[1] * as[1] + A[2] * as[2] - (Bm[0] * cs[0] + Bm[1] * cs[1] + Bm[2] * cs[2]);
            g[s][1] = A[1] * as[0] + A[3] * as[1] + A[4] * as[2] - (Bm[3] * cs[0] + Bm[4] * cs[1] + Bm[5] * cs[2]);
            g[s][2] = A[2] * as[0] + A[4] * as[1] + A[5] * as[2] - (Bm[6] * cs[0] + Bm[7] * cs[1] + Bm[8] * cs[2]);
            k[s][0] = Tt[0] * cs[0] + Tt[1] * cs[1] + Tt[2] * cs[2] - (Bm[0] * as[0] + Bm[3] * as[1] + Bm[6] * as[2]);
            k[s][1] = Tt[1] * cs[0] + Tt[3] * cs[1] + Tt[4] * cs[2] - (Bm[1] * as[0] + Bm[4] * as[1] + Bm[7] * as[2]);
            k[s][2] = Tt[2] * cs[0] + Tt[4] * cs[1] + Tt[5] * cs[2] - (Bm[2] * as[0] + Bm[5] * as[1] + Bm[8] * as[2]);
        }
        const double* a0 = a[q][0]; const double* a1 = a[q][1];
        S[q][0] = (a0[0] * g[0][0] + a0[1] * g[0][1] + a0[2] * g[0][2]) + (c[0][0] * k[0][0] + c[0][1] * k[0][1] + c[0][2] * k[0][2]) + rpix;
        S[q][1] = (a1[0] * g[0][0] + a1[1] * g[0][1] + a1[2] * g[0][2]) + (c[1][0] * k[0][0] + c[1][1] * k[0][1] + c[1][2] * k[0][2]);
        S[q][2] = (a1[0] * g[1][0] + a1[1] * g[1][1] + a1[2] * g[1][2]) + (c[1][0] * k[1][0] + c[1][1] * k[1][1] + c[1][2] * k[1][2]) + rpix;
    }
}

// NK corners from K0 of slot o (= filter * M + slot) of one camera's outputs: the image points rounded once to T, the covariance entries;
// a projection that is not `on` gets zeros
template <typename T, int NCAM, int NK, int K0>
__device__ __forceinline__ void project_put(T* pts, double* cv, size_t o, int c, const bool (&on)[NK * NCAM], const double (&uv)[NK * NCAM][2],
                                            const double (&S)[NK * NCAM][3])
{
    if (pts) {
        T v[2 * NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int q = k * NCAM + c;
            v[2 * k] = on[q] ? (T)uv[q][0] : T(0);
            v[2 * k + 1] = on[q] ? (T)uv[q][1] : T(0);
        }
        project_store<T, 2 * NK>(pts + o * 8 + 2 * K0, v);
    }
    if (cv) {
        double v[3 * NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int q = k * NCAM + c;
#pragma unroll
            for (int j = 0; j < 3; ++j) v[3 * k + j] = on[q] ? S[q][j] : 0.0;
        }
        project_store<double, 3 * NK>(cv + o * 12 + 3 * K0, v);
    }
}

// a slot that produces nothing: zeros in every output
template <typename T, int CAM>
__device__ __forceinline__ void project_zero_slot(const ProjectOut<T>& out, size_t o)
{
    const T zp[8] = { T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0) };
    const double zc[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    if (out.left) project_store<T, 8>(out.left + o * 8, zp);
    if (out.cov_left) project_store<double, 12>(out.cov_left + o * 12, zc);
    if constexpr (CAM == 2) {
        if (out.right) project_store<T, 8>(out.right + o * 8, zp);
        if (out.cov_right) project_store<double, 12>(out.cov_right + o * 12, zc);
    }
    if (out.view) out.view[o] = 0;
}

// CAM: 1 = left camera, 2 = stereo.  NZ: the port is square to the camera.  r_pix: the handle's, or (noise != null: the handle's table
// [FBUS_NOISE_COLS][B]) the lane's own field
template <typename T, int N, int CAM, bool NZ>
__global__ void __launch_bounds__(64)
project_kernel(const T* __restrict__ recs, int B, int M, const int* __restrict__ ids, double size, double r_pix,
               const double* __restrict__ noise, const unsigned char* __restrict__ skip, const short* __restrict__ id2slot, MeasConst mc,
               ProjectOut<T> out)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    constexpr int NT = 64;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned tile = blockIdx.x;
    const int b = (int)(tile * 64u + lane);
    const bool live = b < B && !(skip && skip[b < B ? b : 0]);
    const int bc = b < B ? b : (int)(tile * 64u);
    const double rm = noise ? noise[(size_t)NOISE_RPIX * (size_t)B + (size_t)bc] : r_pix;
    const bool cov = out.cov_left != nullptr || (CAM == 2 && out.cov_right != nullptr);
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc<T, N>(recs, tile);
    __shared__ MeasLDS tbl;
    T pqr[L::NPQR];
    unsigned act = 0;
    {
        MEAS_MAP_LOAD(NT, id2slot, mc.mkc, tbl)
        order_fence();
        int idv[FBUS_MAX_VISIBLE];
#pragma unroll
        for (int i = 0; i < FBUS_MAX_VISIBLE; ++i) idv[i] = ids[(size_t)bc * M + (i < M ? i : M - 1)];
        order_fence();
        load_chunks<T, N, 0, RC::CH_PQR>(rs, lane, pqr);
        order_fence();
        MEAS_MAP_STORE(NT)
        order_fence();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // the wave-uniform set of active slots; the others get their zeros here
#pragma unroll
        for (int i = 0; i < FBUS_MAX_VISIBLE; ++i) {
            if (i < M) {
                const bool idok = idv[i] >= 0 && idv[i] <= FBUS_MAX_MARKER_ID;
                const int sl = idok ? (int)tbl.id2slot[idok ? idv[i] : 0] : -1;
                if (__builtin_amdgcn_ballot_w64(live && sl >= 0) != 0) act |= 1u << i;
                else if (b < B) project_zero_slot<T, CAM>(out, (size_t)b * M + i);
            }
        }
    }
    int cur_id = act ? ids[(size_t)bc * M + __builtin_ctz(act)] : -1;
    order_fence();
    // what depends on the filter alone
    double pd[3], Rd[9];
    MEAS_POSE_OF(L, pqr, mc, pd, Rd, pil)
    ProjPrior pri;
    if (cov) project_prior<T, N>(rs, lane, Rd, pri);
    else {
#pragma unroll
        for (int i = 0; i < 6; ++i) { pri.A[i] = 0.0; pri.Tt[i] = 0.0; }
#pragma unroll
        for (int i = 0; i < 9; ++i) pri.Bm[i] = 0.0;
    }
#pragma unroll 1
    while (act) {
        const int i = __builtin_ctz(act);
        act &= act - 1;
        const int nxt_id = ids[(size_t)bc * M + (act ? __builtin_ctz(act) : i)];        // (the next slot's id in flight under this one)
        const bool idok = cur_id >= 0 && cur_id <= FBUS_MAX_MARKER_ID;
        const int slot = idok ? (int)tbl.id2slot[idok ? cur_id : 0] : -1;
        const bool in_map = live && slot >= 0;
        const int sl = slot >= 0 ? slot : 0;                                            // (an unknown id: slot 0's frame, outputs cleared)
        double mk[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) mk[q] = tbl.mkc[sl * MKC_STRIDE + q];
        const size_t o = (size_t)(b < B ? b : 0) * M + i;
        unsigned bits = 0;
        if constexpr (CAM == 1) {
            bool ok[4];
            double uv[4][2], S[4][3];
            project_corners<1, T, NZ, 4, 0>(pd, Rd, pil, mc, mk, size, cov, pri, rm, ok, uv, S);
#pragma unroll
            for (int q = 0; q < 4; ++q) { ok[q] = ok[q] && in_map; bits |= ok[q] ? 1u << q : 0u; }
            if (b < B) project_put<T, 1, 4, 0>(out.left, out.cov_left, o, 0, ok, uv, S);
        } else {
            {
                bool ok[4];
                double uv[4][2], S[4][3];
                project_corners<2, T, NZ, 2, 0>(pd, Rd, pil, mc, mk, size, cov, pri, rm, ok, uv, S);
#pragma unroll
                for (int q = 0; q < 4; ++q) { ok[q] = ok[q] && in_map; bits |= ok[q] ? 1u << ((q & 1) * 4 + (q >> 1)) : 0u; }
                if (b < B) {
                    project_put<T, 2, 2, 0>(out.left, out.cov_left, o, 0, ok, uv, S);
                    project_put<T, 2, 2, 0>(out.right, out.cov_right, o, 1, ok, uv, S);
                }
            }
            order_fence();
            {
                bool ok[4];
                double uv[4][2], S[4][3];
                project_corners<2, T, NZ, 2, 2>(pd, Rd, pil, mc, mk, size, cov, pri, rm, ok, uv, S);
#pragma unroll
                for (int q = 0; q < 4; ++q) { ok[q] = ok[q] && in_map; bits |= ok[q] ? 1u << ((q & 1) * 4 + 2 + (q >> 1)) : 0u; }
                if (b < B) {
                    project_put<T, 2, 2, 2>(out.left, out.cov_left, o, 0, ok, uv, S);
                    project_put<T, 2, 2, 2>(out.right, out.cov_right, o, 1, ok, uv, S);
                }
            }
        }
        if (b < B && out.view) out.view[o] = (unsigned char)bits;
        cur_id = nxt_id;
    }
}

}  // namespace

namespace fbus {
// grid: one wave per tile
template <typename T, int N, int CAM>
void launch_project_k(hipStream_t st, const T* recs, int B, int M, const int* ids, bool square_port, double size, double r_pix,
                      const double* noise, const unsigned char* skip, const short* id2slot, const MeasConst& mc, const ProjectOut<T>& out)
{
    const dim3 grid((B + 63) / 64), block(64);
    if (square_port)
        hipLaunchKernelGGL((project_kernel<T, N, CAM, true>), grid, block, 0, st, recs, B, M, ids, size, r_pix, noise, skip, id2slot, mc, out);
    else
        hipLaunchKernelGGL((project_kernel<T, N, CAM, false>), grid, block, 0, st, recs, B, M, ids, size, r_pix, noise, skip, id2slot, mc, out);
}
}  // namespace fbus
