// ekf_sample.hpp -- draws from every filter's own Gaussian N(estimate, P) (fbus_ekf_sample*, include/fbus_ekf.h): the inverse of NEES.
// No reference counterpart; the model is stated in the header.  Included by small_tu.hip's report family only.  gfx950 only.
//
// With L L' = Pi P Pi' in the factorisation order of nees_kernel (p, theta, v, ba, bg, g: nees_ord) a draw is delta = Pi' L xi, injected
// into the record's nominal state in double: plain sums, and q <- normalize(q (x) dq(delta_theta)) -- inject() of ekf_device.hpp in double,
// and so the inverse of group_delta's Log.  The factor is nees_kernel's factor, applied forwards instead of solved backwards.
//
// READ-ONLY, and the stream of nees_kernel: one filter per lane, one wave per 64-filter tile at every batch size, the nominal chunks
// requested first, then the covariance in storage order with the non-temporal policy.  The factorisation runs column by column with
// compile-time indices (static_for, pidx<N>, nees_tri<N>) and leaves L -- with its diagonal, 171 doubles for N = 18 -- in registers; P is
// dead behind it.  Then a runtime loop over the S draws of the call: the lane's N coordinates, N (N + 1) / 2 multiply-adds row by row
// (a row of delta goes into its output as soon as it is formed: what stays live beside L is xi), the injection, 19 stores.
// A filter that is skipped or has a pivot that is not > 0 (false for NaN) stores its own nominal row by a select, whatever L holds.
// The xi loads have a lane stride of 8 N bytes and the stores one of 152 bytes, as truth and err have in nees_kernel.
#pragma once
#include "ekf_nees.hpp"

namespace {

template <typename T, int N>
__global__ void __launch_bounds__(BLOCK, 1)
sample_kernel(const T* __restrict__ recs, int B, int S, const double* __restrict__ xi, const unsigned char* __restrict__ skip, SampleOut out)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    constexpr int NP = L::NP;
    int b, bc;
    bool in;
    unsigned char skin;
    T nom[L::NNOM], P[RC::NCOVP];
    factor_stream<T, N>(recs, B, skip, b, in, bc, skin, nom, P, [](int) {});

    // ---- the factorisation of nees_kernel, kept whole: L(i, a) at nees_tri<N>(a, i), the diagonal included ------------------------------
    double Lf[NP];
    bool ok = true;
    static_for<0, N>([&](auto a_) {
        constexpr int a = decltype(a_)::value, sa = nees_ord(a);
        double piv = (double)P[pidx<N>(sa, sa)];
        static_for<0, a>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            piv -= Lf[nees_tri<N>(k, a)] * Lf[nees_tri<N>(k, a)];
        });
        const bool pos = piv > 0.0;
        ok = ok && pos;
        const double is = nees_rsqrt(piv, pos);
        Lf[nees_tri<N>(a, a)] = pos ? sqrt(pos ? piv : 1.0) : 0.0;
        factor_below<T, N, a>(P, Lf, is);
    });
    const bool dr = ok && !skin;
    if (in && out.drawn) out.drawn[b] = dr ? (unsigned char)1 : (unsigned char)0;
    if (!out.state) return;

    // the nominal state as doubles, in the order of fbus_ekf_get_state
    double x0[19];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        x0[ApiOrder::OFF_P3 + i] = (double)nom[L::OFF_P3 + i];
        x0[ApiOrder::OFF_V + i] = (double)nom[L::OFF_V + i];
        x0[ApiOrder::OFF_BA + i] = (double)nom[L::OFF_BA + i];
        x0[ApiOrder::OFF_BG + i] = (double)nom[L::OFF_BG + i];
        x0[ApiOrder::OFF_G + i] = (double)nom[L::OFF_G + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) x0[ApiOrder::OFF_Q + i] = (double)nom[L::OFF_Q + i];

    // ---- the draws: delta = Pi' L xi_s, injected in double --------------------------------------------------------------------------------
    for (int s = 0; s < S; ++s) {
        const double* xr = xi + ((size_t)s * B + bc) * N;
        double x[N];
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = ld_once(xr + i);
        double row[19], th[3];
        static_for<0, N>([&](auto i_) {
            constexpr int i = decltype(i_)::value;
            double d = 0.0;
            static_for<0, i + 1>([&](auto a_) {
                constexpr int a = decltype(a_)::value;
                d += Lf[nees_tri<N>(a, i)] * x[a];
            });
            // position i of the factorisation order is state nees_ord(i) of the error state: its place in the row
            if constexpr (i < 3) row[ApiOrder::OFF_P3 + i] = x0[ApiOrder::OFF_P3 + i] + d;
            else if constexpr (i < 6) th[i - 3] = d;
            else if constexpr (i < 9) row[ApiOrder::OFF_V + (i - 6)] = x0[ApiOrder::OFF_V + (i - 6)] + d;
            else if constexpr (i < 12) row[ApiOrder::OFF_BA + (i - 9)] = x0[ApiOrder::OFF_BA + (i - 9)] + d;
            else if constexpr (i < 15) row[ApiOrder::OFF_BG + (i - 12)] = x0[ApiOrder::OFF_BG + (i - 12)] + d;
            else row[ApiOrder::OFF_G + (i - 15)] = x0[ApiOrder::OFF_G + (i - 15)] + d;
        });
        if constexpr (N == 15) {
#pragma unroll
            for (int i = 0; i < 3; ++i) row[ApiOrder::OFF_G + i] = x0[ApiOrder::OFF_G + i];
        }
        {   // q <- normalize(q (x) dq(dtheta)), dq = (cos |dtheta|/2, sin(|dtheta|/2) / |dtheta| dtheta): inject() in double
            const double nn = sqrt(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
            double sh, ch;
            sincos(0.5 * nn, &sh, &ch);
            const bool zero = nn == 0.0;
            const double k = zero ? 0.0 : sh / nn;
            const double dq[4] = { zero ? 1.0 : ch, th[0] * k, th[1] * k, th[2] * k };
            double qn[4];
            quat_mul(x0 + ApiOrder::OFF_Q, dq, qn);
            const double n = sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
#pragma unroll
            for (int i = 0; i < 4; ++i) row[ApiOrder::OFF_Q + i] = qn[i] / n;
        }
        if (in) {
            double* o = out.state + ((size_t)s * B + b) * 19;
#pragma unroll
            for (int i = 0; i < 19; ++i) o[i] = dr ? row[i] : x0[i];       // a select, not a branch: a filter that is not drawn is its nominal
        }
    }
}

}  // namespace

namespace fbus {
// grid: one wave per tile
template <typename T, int N>
void launch_sample_k(hipStream_t st, const T* recs, int B, int S, const double* xi, const unsigned char* skip, const SampleOut& out)
{
    hipLaunchKernelGGL((sample_kernel<T, N>), dim3((B + 63) / 64), dim3(BLOCK), 0, st, recs, B, S, xi, skip, out);
}
}  // namespace fbus
