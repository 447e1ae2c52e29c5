// ekf_depth.hpp -- the depth (pressure) sensor update (fbus_ekf_correct_depth*, include/fbus_ekf.h).  No reference counterpart: the
// reference names the sensor (`namespace FBUSEKF // Underwater Vision IMU Depth EKF`, C++/include/common.hpp:16) and has no update for it.
// Included by small_tu.hip's sensor family only.  gfx950 only.
//
// One scalar row on the index set J = {p, theta} of the pose rows, with R the record's carried rotation:
//     h(x) = axis . (p + R lever) + offset      H_p = axis'      H_theta = (lever x (R' axis))'
//     res = z - h      S = H P H' + var      u = P H'      dx = u res / S -> inject()      P <- P - u u' / S
// For one row (I - K H) P, its Joseph form and P - u u' / S are the same matrix: one symmetric form for both cov_form settings.
// fp32 records do this arithmetic -- u, S, the gain, the rank-1 term -- in DOUBLE and round every covariance element once, as
// correct_velocity_kernel does: the update takes the variance along its row from the prior's to the sensor's, and P - u u' / S in fp32 keeps
// eps32 x prior / posterior of it (a position prior of 1 m beside var = 1e-4: 2e-3 of the posterior variance, 2e-1 at 10 m).
// fp64 records do it in the record type.
//
// Mapping: one filter per lane, one wave per 64-filter tile, one buffer descriptor per tile -- at every batch size.
// A stream, as predict_kernel (K = 1) is: z, var and skip are requested first, then every record chunk in use order (nominal state,
// covariance in storage order).  u = P H' reads P(:, J) only, and every such element sits in the first DepthCut::C_J chunks (storage rows
// 0..8 and, for even N, the odd-row diagonals collected behind them); the arithmetic starts when THOSE have landed -- vector memory
// operations retire in issue order and the waits in front of each use are the compiler's counted s_waitcnt vmcnt(n), n = the operations
// issued behind the chunk -- forms u, S, the gate and dx, stores the injected nominal state, and then gives every covariance chunk its
// rank-1 term and stores it, in storage order: the chunks past C_J are still arriving while the first ones go out.
// The gate -- S > 0 and nis <= thr[1], both false for a NaN: the rule of correct_velocity_kernel and correct_rows_kernel with one pivot --
// is decided before the first store; a lane that is skipped, has a non-finite z or a var that is not a finite number > 0, or is not
// applied (a record of NaN and one with a negated covariance among them), leaves before it and stores nothing to its record.  No early
// exit in front of the loads (the compiler would sink loads into the live branch, behind the stream; correct_kernel's reason).
#pragma once
#include "ekf_sensor.hpp"       // the exits and the gate rule, store_nominal, the two covariance passes, pin_chunk, launch_tile_k

namespace {

template <typename T, int N>
struct DepthCut {
    // one past the last record chunk that holds an element P(i, j), j in J
    static constexpr int early_end()
    {
        int m = 0;
        for (int i = 0; i < N; ++i)
            for (int k = 0; k < 6; ++k)
                if (pidx<N>(i, jcol(k)) > m) m = pidx<N>(i, jcol(k));
        return Rec<T, N>::CH_NOM + m / Rec<T, N>::EPC + 1;
    }
    static constexpr int C_J = early_end();
    static_assert(C_J <= Rec<T, N>::NCH, "the J columns lie inside the record");
};

// fp64: 171 covariance doubles are 342 of the 512 registers; the nominal state, u, the row and the double scalars fit on top (474 / 350
// registers for N = 18 / 15, no scratch: DESIGN 4.3.5), so both record types run the one unsplit form and no LDS is used.
// nis / dof (each may be null), lik (null while the likelihood sums are off: the handle's [4][B] accumulator) and thr (the handle's gate
// table, +inf without one) are arguments of the one instantiation: the plain, _nis and likelihood-on calls run the same code object.
template <typename T, int N>
__global__ void __launch_bounds__(BLOCK, 1)
correct_depth_kernel(T* recs /* not __restrict__: order_fence()'s memory clobber must cover the records, see below */, int B,
                     const T* __restrict__ z, const double* __restrict__ var, int var_stride, const unsigned char* __restrict__ skip, unsigned char* __restrict__ applied, DepthSensor ds,
                     const double* __restrict__ thr, T* __restrict__ nis, int* __restrict__ dof, double* __restrict__ lik)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    constexpr int EPC = RC::EPC, CN = RC::CH_NOM, C_J = DepthCut<T, N>::C_J;
    // The waits are the compiler's: it counts the vector memory operations issued behind the one a use needs.  The largest count of the
    // fp32 forms is the wait for z, var and skip behind the NCH record loads (52 for N = 18), the stream's own waits count the late loads
    // and the stores issued since (47): both fit the 6-bit vmcnt field, so every fp32 wait is exact.  The fp64 records have 100 / 77
    // chunks: there the compiler clamps a larger count to 63, which waits early, never late.
    static_assert(sizeof(T) == 8 || RC::NCH + 3 <= 63, "fp32: every counted wait of the stream must fit the 6-bit vmcnt field");
    static_assert(BLOCK == 64, "one wave per 64-filter tile");
    const int b = blockIdx.x * BLOCK + threadIdx.x;
    const bool in = b < B;
    const int bc = in ? b : B - 1;                      // lanes past B run along on the last filter's inputs and store nothing
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc<T, N>(recs, my_tile());
    T nom[L::NNOM], P[RC::NCOVP];
    // the call's inputs first, without a branch (a conditional skip load is waited for in front of the record stream): a call without
    // skip reads a byte of z in its place
    const T zin = ld_once(z + bc);
    const double vin = ld_once(var + (var_stride ? bc : 0));
    const unsigned char skin = *(skip ? skip + bc : reinterpret_cast<const unsigned char*>(z + bc));
    const double gate = thr[1];
    order_fence();
    load_chunks<T, N, 0, CN>(rs, my_lane(), nom);
    order_fence();
    load_chunks<T, N, CN, C_J, FBUS_X_CORRECT_LD>(rs, my_lane(), P);
    order_fence();
    load_chunks<T, N, C_J, RC::NCH, FBUS_X_CORRECT_LD>(rs, my_lane(), P + (C_J - CN) * EPC);
    order_fence();
    // The inputs become known to the compiler HERE, behind the loads: whether a lane is usable does not depend on its record, and a test
    // the compiler can make earlier is hoisted above the record loads, which then wait for z and var inside the live branch (seen in the
    // ISA of the first version: a vmcnt(0) in front of the first buffer load).  For the same reason `recs` is not __restrict__: an asm
    // cannot touch memory that only a noalias argument reaches, so loads through one move across order_fence() and sink into the branch.
    T zv = zin;
    double varv = vin;
    unsigned skv = skip ? (unsigned)skin : 0u;
    asm volatile("" : "+v"(zv), "+v"(varv), "+v"(skv));
    const SensorOut<T> o{ applied, nis, dof, lik, B, b };
    // untouched lanes  (x > 0 is false for a NaN)
    const bool usable = in && skv == 0u && isfinite((double)zv) && isfinite(varv) && varv > 0.0;
    if (!usable) return leave_untouched(o, in);

    // h, the innovation and the row in double (a handful of scalars per filter); the row is rounded once to the record type
    const T* R = nom + L::OFF_R;
    double Rl[3], Rta[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        Rl[i] = (double)R[3 * i] * ds.lever[0] + (double)R[3 * i + 1] * ds.lever[1] + (double)R[3 * i + 2] * ds.lever[2];
        Rta[i] = (double)R[i] * ds.axis[0] + (double)R[3 + i] * ds.axis[1] + (double)R[6 + i] * ds.axis[2];
    }
    double hx = ds.offset;
#pragma unroll
    for (int i = 0; i < 3; ++i) hx += ds.axis[i] * ((double)nom[L::OFF_P3 + i] + Rl[i]);
    const double res = (double)zv - hx;
    const T H[6] = { (T)ds.axis[0], (T)ds.axis[1], (T)ds.axis[2],
                     (T)(ds.lever[1] * Rta[2] - ds.lever[2] * Rta[1]), (T)(ds.lever[2] * Rta[0] - ds.lever[0] * Rta[2]),
                     (T)(ds.lever[0] * Rta[1] - ds.lever[1] * Rta[0]) };
#define PS(i, j) P[pidx<N>((i), (j))]
    // A: the type of the arithmetic -- double for both record types (see the head of the file).  fp32: N doubles beside the covariance
    using A = SensorArith<T>;
    A u[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        A acc = (A)PS(i, jcol(0)) * (A)H[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) acc += (A)PS(i, jcol(k)) * (A)H[k];
        u[i] = acc;
    }
#undef PS
    double hph = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) hph += (double)H[k] * (double)u[jcol(k)];
    const double S = hph + varv;
    const RowSums g{ res * res / S, S, S > 0.0 };       // nis, det S and the one pivot
    report(o, g, 1);
    if (gate_shut(g, gate)) return leave_rejected(o, g, 1);
    const double is = 1.0 / S;
    const A gn = (A)(res * is);
    const T dk = (T)is;
    {
        T dx[N];
#pragma unroll
        for (int i = 0; i < N; ++i) dx[i] = (T)(u[i] * gn);
        inject<T, N>(nom, dx);
    }
    if constexpr (sizeof(T) == 4) {
        // y = u / sqrt(S): the rank-1 term is y y', symmetric to the bit
        const double rsq = sqrt(is);
#pragma unroll
        for (int i = 0; i < N; ++i) u[i] *= rsq;
        // The chunks that hold P(:, J) are made opaque in front of the pass: the compiler otherwise keeps the columns it widened for u
        // alive for it, two registers each beside the covariance they were converted from (364 registers for N = 18; 281 with it).  The
        // EARLY chunks only -- they have landed; an asm that names a late chunk would wait for it in front of the first store.
        static_for<0, C_J - CN>([&](auto cc) { pin_chunk(P + EPC * decltype(cc)::value); });
    }
    store_nominal<T, N>(rs, nom);
    // every covariance chunk takes its rank-1 term and goes out, in storage order
    if constexpr (sizeof(T) == 4) joint_pass<T, N, 1>(rs, P, &u);
    else rank1_pass<T, N, true>(rs, P, u, dk);
    leave_applied(o, g, 1);
}

}  // namespace

namespace fbus {
template <typename T, int N>
void launch_depth_k(hipStream_t s, T* recs, int B, const T* z, const double* var, int var_stride, const unsigned char* skip,
                    unsigned char* applied, const DepthSensor& ds, const double* thr, T* nis, int* dof, double* lik)
{
    launch_tile_k(correct_depth_kernel<T, N>, s, B, recs, B, z, var, var_stride, skip, applied, ds, thr, nis, dof, lik);
}
}  // namespace fbus
