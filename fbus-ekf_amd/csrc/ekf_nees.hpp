// ekf_nees.hpp -- NEES, error and log-density of every filter against a truth state (fbus_ekf_nees*, include/fbus_ekf.h).  No reference
// counterpart: the reference runs one filter and is judged off line; the model is stated in the header.
// Included by small_tu.hip's report family only, through ekf_sample.hpp.  gfx950 only.
//
// With delta = truth (-) estimate (step 3 of fbus_ekf_group_fuse with the record as the chart: group_delta, ekf_group.hpp) a column of
// `nees` is delta_J' (P_JJ)^-1 delta_J = |L^-1 delta_J|^2, L L' = P_JJ, in double for both record types.
//
// READ-ONLY: the kernel takes the records as const, loads every chunk of a record once and stores nothing but its three outputs.
// Mapping: one filter per lane, one wave per 64-filter tile at every batch size.  The truth row, the skip byte and the nominal chunks
// are requested first, then the covariance chunks in storage order: delta and the Log are formed while the covariance arrives.
// The covariance is factorised in the order p, theta, v, ba, bg, g (nees_ord): the leading k entries of y = L^-1 delta depend on the
// leading k x k block alone, so P and POSE are the prefix sums |y(0..2)|^2 and |y(0..5)|^2 of FULL's own solve, and the other four
// 3 x 3 marginals are factorised on their own from the same registers (nees_block3).  The solve runs along with the factorisation (row a
// of y when column a of L is done); no inverse is formed.  Every index into the packed triangle and into L is a compile-time constant
// (static_for, pidx<N>, nees_tri<N>): P and L live in registers, widened to double where they are used -- 171 doubles of L for N = 18.
// A pivot that is not > 0 (false for NaN) or a delta component that is not finite marks the columns that contain it and no other;
// the factorisation runs on with that column of L zeroed, so nothing it poisons is read by a column that is still clean.
#pragma once
#include "ekf_group.hpp"
#include "ekf_launch.hpp"        // NeesOut, SampleOut

namespace {

// the state behind position k of the factorisation order p, theta, v, ba, bg, g
__host__ __device__ constexpr int nees_ord(int k) { return k < 3 ? k : k < 6 ? k + 3 : k < 9 ? k - 3 : k; }
// L(i, a), a <= i in that order: the row-major upper triangle of L'
template <int N>
__host__ __device__ constexpr int nees_tri(int a, int i) { return a * N - a * (a - 1) / 2 + (i - a); }

// A value made opaque where it is formed: the outputs are used behind the NULL tests alone, and the compiler otherwise sinks their
// arithmetic -- and the covariance elements it reads -- down to the stores, beside the full factor (fp64, N = 18: 204 B of scratch)
__device__ __forceinline__ void nees_pin(double& x) { asm volatile("" : "+v"(x)); }

// 1 / sqrt(piv) for a pivot that is > 0, else 0 (that column of L is dropped).  Without a branch: the square root and the division run on
// a harmless 1 for a bad pivot and a select follows -- as `pos ? 1 / sqrt(piv) : 0` every pivot is a basic block of its own, 33 of them,
// and the register allocator's moves out of the AGPRs the late chunks were loaded into pile up in front of the first, behind a wait
// for the whole stream
__device__ __forceinline__ double nees_rsqrt(double piv, bool pos)
{
    const double r = 1.0 / sqrt(pos ? piv : 1.0);
    return pos ? r : 0.0;
}

// delta_J' (P_JJ)^-1 delta_J of the 3 x 3 marginal J = {I0, I0 + 1, I0 + 2}; NaN by the column rule
template <typename T, int N, int I0>
__device__ __forceinline__ double nees_block3(const T* P, const double* dl)
{
    const double a00 = (double)P[pidx<N>(I0, I0)], a01 = (double)P[pidx<N>(I0, I0 + 1)], a02 = (double)P[pidx<N>(I0, I0 + 2)];
    const double a11 = (double)P[pidx<N>(I0 + 1, I0 + 1)], a12 = (double)P[pidx<N>(I0 + 1, I0 + 2)], a22 = (double)P[pidx<N>(I0 + 2, I0 + 2)];
    bool ok = __builtin_isfinite(dl[I0]) && __builtin_isfinite(dl[I0 + 1]) && __builtin_isfinite(dl[I0 + 2]);
    ok = ok && a00 > 0.0;
    const double i0 = nees_rsqrt(a00, a00 > 0.0);
    const double l10 = a01 * i0, l20 = a02 * i0, y0 = dl[I0] * i0;
    const double p1 = a11 - l10 * l10;
    ok = ok && p1 > 0.0;
    const double i1 = nees_rsqrt(p1, p1 > 0.0);
    const double l21 = (a12 - l20 * l10) * i1, y1 = (dl[I0 + 1] - l10 * y0) * i1;
    const double p2 = a22 - l20 * l20 - l21 * l21;
    ok = ok && p2 > 0.0;
    const double i2 = nees_rsqrt(p2, p2 > 0.0);
    const double y2 = (dl[I0 + 2] - l20 * y0 - l21 * y1) * i2;
    double r = ok ? y0 * y0 + y1 * y1 + y2 * y2 : __builtin_nan("");
    nees_pin(r);
    return r;
}

// ---- what nees_kernel and sample_kernel (ekf_sample.hpp) share: one stream and one sub-diagonal step, so that the two cannot drift apart ----
// The prologue of both: the lane's filter b, in = b < B, the clamped index bc (lanes past B run along on the last filter's inputs and
// store nothing), the kernel's own loads own(bc), the skip byte, the nominal chunks (the carried rotation between q and v is not
// read), then the covariance chunks in storage order, non-temporally.  nom and P are the caller's own arrays.
template <typename T, int N, typename OWN>
__device__ __forceinline__ void factor_stream(const T* __restrict__ recs, int B, const unsigned char* __restrict__ skip, int& b, bool& in,
                                              int& bc, unsigned char& skin, T* nom, T* P, OWN own)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    static_assert(BLOCK == 64, "one wave per 64-filter tile");
    b = blockIdx.x * BLOCK + threadIdx.x;
    in = b < B;
    bc = in ? b : B - 1;
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc<T, N>(recs, my_tile());
    own(bc);
    skin = skip ? skip[bc] : (unsigned char)0;
    order_fence();
    constexpr int C_PQ = RC::CH_PQ, C_V = L::OFF_V / RC::EPC;
    static_assert(L::OFF_V % RC::EPC == 0, "v, ba, bg, g start on a chunk boundary");
    load_chunks<T, N, 0, C_PQ>(rs, my_lane(), nom);
    load_chunks<T, N, C_V, RC::CH_NOM>(rs, my_lane(), nom + L::OFF_V);
    order_fence();
    load_chunks<T, N, RC::CH_NOM, RC::NCH, AUX_NT>(rs, my_lane(), P);
    order_fence();
}

// The rows of column a of L below its pivot, `is` = nees_rsqrt of the pivot (0: the column is dropped): L(i, a) at nees_tri<N>(a, i)
template <typename T, int N, int a>
__device__ __forceinline__ void factor_below(const T* P, double* Lf, double is)
{
    constexpr int sa = nees_ord(a);
    static_for<a + 1, N>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        double v = (double)P[pidx<N>(sa, nees_ord(i))];
        static_for<0, a>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            v -= Lf[nees_tri<N>(k, i)] * Lf[nees_tri<N>(k, a)];
        });
        Lf[nees_tri<N>(a, i)] = v * is;
    });
    __builtin_amdgcn_sched_barrier(0);                  // column by column: what is live stays the triangle (P ahead, L behind)
}

template <typename T, int N>
__global__ void __launch_bounds__(BLOCK, 1)
nees_kernel(const T* __restrict__ recs, int B, const double* __restrict__ truth, const unsigned char* __restrict__ skip, NeesOut out)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    constexpr int NP = L::NP;
    int b, bc;
    bool in;
    unsigned char skin;
    double tr[19];
    T nom[L::NNOM], P[RC::NCOVP];
    factor_stream<T, N>(recs, B, skip, b, in, bc, skin, nom, P, [&](int row) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 19; ++i) tr[i] = ld_once(truth + (size_t)row * 19 + i);
    });

    // ---- delta: q_true normalised in double, then group_delta with the record as the chart ---------------------------------------------
    {
        const double n = sqrt(tr[6] * tr[6] + tr[7] * tr[7] + tr[8] * tr[8] + tr[9] * tr[9]);
#pragma unroll
        for (int i = 6; i < 10; ++i) tr[i] = tr[i] / n;         // (a zero or non-finite q_true: NaN in every theta entry)
    }
    double dl[N];
    group_delta<T, N, ApiOrder>(tr, nom, dl);
    // err goes out here, not behind the factorisation: delta's registers are then free as the solve consumes it
    if (in && out.err) {
#pragma unroll
        for (int i = 0; i < N; ++i) out.err[(size_t)b * N + i] = skin ? 0.0 : dl[i];
    }

    // A row of nees is four 16-byte stores, each as soon as its two columns are known: nothing waits in registers beside the factor
    const double nanv = __builtin_nan("");
    auto put = [&](int pair, double c0, double c1) __attribute__((always_inline)) {
        if (in && out.nees)
            reinterpret_cast<double2*>(out.nees + (size_t)b * FBUS_NEES_COLS)[pair] = double2{ skin ? 0.0 : c0, skin ? 0.0 : c1 };
    };
    static_assert(FBUS_NEES_FULL == 0 && FBUS_NEES_POSE == 1 && FBUS_NEES_P == 2 && FBUS_NEES_V == 3 && FBUS_NEES_THETA == 4 &&
                  FBUS_NEES_BA == 5 && FBUS_NEES_BG == 6 && FBUS_NEES_G == 7, "the pairs below are the header's columns");

    // ---- the full factorisation, the solve along with it --------------------------------------------------------------------------------
    double Lf[NP], y[N];
    double acc = 0.0, logdet = 0.0, pose = 0.0, cp = 0.0, th = 0.0, bg = 0.0;
    bool ok = true;
    static_for<0, N>([&](auto a_) {
        constexpr int a = decltype(a_)::value, sa = nees_ord(a);
        // the 3 x 3 marginals that are no prefix, each in front of the column that is the first to read its rows: its elements have
        // landed by then and die right behind it, and the columns in front of it run while the rest of the stream arrives
        if constexpr (a == 3) th = nees_block3<T, N, 6>(P, dl);
        if constexpr (a == 6) put(1, cp, nees_block3<T, N, 3>(P, dl));
        if constexpr (a == 9) put(2, th, nees_block3<T, N, 9>(P, dl));
        if constexpr (a == 12) {
            bg = nees_block3<T, N, 12>(P, dl);
            if constexpr (N == 15) put(3, bg, 0.0);
        }
        if constexpr (a == 15) put(3, bg, nees_block3<T, N, 15>(P, dl));
        double piv = (double)P[pidx<N>(sa, sa)];
        double u = dl[sa];
        static_for<0, a>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            piv -= Lf[nees_tri<N>(k, a)] * Lf[nees_tri<N>(k, a)];
            u -= Lf[nees_tri<N>(k, a)] * y[k];
        });
        const bool pos = piv > 0.0;
        ok = ok && pos && __builtin_isfinite(dl[sa]);
        const double is = nees_rsqrt(piv, pos);
        logdet += log(piv);
        y[a] = u * is;
        acc += y[a] * y[a];
        nees_pin(y[a]);
        nees_pin(acc);
        nees_pin(logdet);
        factor_below<T, N, a>(P, Lf, is);
        if constexpr (a == 2) cp = ok ? acc : nanv;
        if constexpr (a == 5) pose = ok ? acc : nanv;
    });
    put(0, ok ? acc : nanv, pose);
    const double lnp = ok ? -0.5 * (acc + logdet + (double)N * 1.8378770664093453) : nanv;      // ln 2 pi
    if (in && out.lnp) out.lnp[b] = skin ? 0.0 : lnp;
}

}  // namespace

namespace fbus {
// grid: one wave per tile
template <typename T, int N>
void launch_nees_k(hipStream_t st, const T* recs, int B, const double* truth, const unsigned char* skip, const NeesOut& out)
{
    hipLaunchKernelGGL((nees_kernel<T, N>), dim3((B + 63) / 64), dim3(BLOCK), 0, st, recs, B, truth, skip, out);
}
}  // namespace fbus
