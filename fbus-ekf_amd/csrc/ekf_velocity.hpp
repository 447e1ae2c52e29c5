// ekf_velocity.hpp -- the body-velocity (DVL, zero-velocity) update (fbus_ekf_correct_velocity*, include/fbus_ekf.h).  No reference
// counterpart: the reference has no velocity measurement, the model is stated in the header.  Included by small_tu.hip's sensor family
// only.  gfx950 only.
//
// Three rows on the index set V = {v, theta, bg} (columns 3..8 and 12..14), with R the record's carried rotation, C the mount and
// w = gyro - bg:
//     h(x) = C (R' v + w x lever)      H_v = C R'      H_theta = C [R' v]x      H_bg = C [lever]x
//     res = z - h      S = H P H' + diag(var)      dx = P H' S^-1 res -> inject()      P <- P - P H' S^-1 H P
// Processing the rows one after the other AT THE ONE linearisation point gives the same dx, P, nis and log det S as the joint solve:
//     u = P h_k      s_k = h_k . u + var_k      r_k = res_k - h_k . dx      dx += u r_k / s_k      P -= u u' / s_k
//     nis = sum r_k^2 / s_k      det S = prod s_k        (the s_k are the squares of the Cholesky pivots of S)
// The two record types take the two forms of it:
//   fp64  the sequential rows as written, in the record type: one u is alive at a time.  Rows one and two update P in registers, the third
//         rank-1 term is applied chunk by chunk, each chunk stored behind its own arithmetic.  N = 18 passes 512 registers (636 B scratch).
//   fp32  the joint form with its arithmetic in DOUBLE and one rounding per covariance element.  The update takes the velocity block from
//         the prior's 0.1 (m/s)^2 to the sensor's 1e-4, and P - u u' / s in fp32 keeps eps32 x prior / posterior of that (4e-4 block-wise
//         where the gate is 1e-5).  The rows are orthogonalised against each other from the ORIGINAL P -- the same u_k, s_k, r_k -- and P
//         takes  P - sum u_k u_k' / s_k  in one streamed pass.  3 N doubles beside the fp32 covariance; no scratch.
//
// Mapping and stream as correct_depth_kernel: one filter per lane, one wave per 64-filter tile, one buffer descriptor per tile -- at
// every batch size.  z, gyro, var and skip are requested first, then every record chunk in use order.  P(:, V) reaches into the LAST
// covariance chunk of every layout (VelocityCut::C_V is NCH, or NCH - 1 where the last chunk holds prev_id alone: (14, 15) of N = 18 is
// packed element 168 of 171, (14, 14) of N = 15 is the last element): the arithmetic waits for the whole record (the compiler's counted
// waits still let the first row's sums start on the early chunks).  The gate -- three pivots > 0 and nis <= thr[3] -- is decided behind
// the third row's s and r, before the first store; then the injected nominal state goes out and the covariance chunks follow in storage
// order.  A lane that is skipped, has a non-finite z or gyro or a var that is not a finite number > 0, or is not applied, stores nothing
// to its record.  No early exit in front of the loads (correct_depth_kernel's reason).
#pragma once
#include "ekf_sensor.hpp"       // the exits and the gate rule, store_nominal, the two row steps and covariance passes, launch_tile_k

namespace {

__host__ __device__ constexpr int vcol(int k) { return k < 6 ? k + 3 : k + 6; }          // V-position -> state column
// the column set of a row of H (ekf_sensor.hpp): its 9 entries on V
struct VCols {
    static constexpr int n = 9;
    static constexpr int col(int k) { return vcol(k); }
};

template <typename T, int N>
struct VelocityCut {
    // one past the last record chunk that holds an element P(i, j), j in V
    static constexpr int early_end()
    {
        int m = 0;
        for (int i = 0; i < N; ++i)
            for (int k = 0; k < 9; ++k)
                if (pidx<N>(i, vcol(k)) > m) m = pidx<N>(i, vcol(k));
        return Rec<T, N>::CH_NOM + m / Rec<T, N>::EPC + 1;
    }
    static constexpr int C_V = early_end();
    static_assert(C_V >= Rec<T, N>::NCH - 1 && C_V <= Rec<T, N>::NCH,
                  "the V columns reach into the last chunk that holds a covariance element: nothing starts before the whole record has landed");
};

// nis / dof (each may be null), lik (null while the likelihood sums are off) and thr (the handle's gate table, +inf without one) are
// arguments of the one instantiation, as in correct_depth_kernel: the plain, _nis and likelihood-on calls run the same code object.
// gyro may be null: the w x lever term and H_bg are then exactly zero.
template <typename T, int N>
__global__ void __launch_bounds__(BLOCK, 1)
correct_velocity_kernel(T* recs /* not __restrict__: see correct_depth_kernel */, int B, const T* __restrict__ z, const T* __restrict__ gyro,
                        const double* __restrict__ var, int var_stride, const unsigned char* __restrict__ skip,
                        unsigned char* __restrict__ applied, VelocitySensor vs, const double* __restrict__ thr, T* __restrict__ nis,
                        int* __restrict__ dof, double* __restrict__ lik)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    constexpr int CN = RC::CH_NOM;
    // The waits are the compiler's counted vmcnt.  The largest count of the fp32 forms is the wait for the ten input loads behind the NCH
    // record loads (60 for N = 18); the fp64 records have 100 / 77 chunks, there a larger count is clamped to 63: early, never late.
    static_assert(sizeof(T) == 8 || RC::NCH + 10 <= 63, "fp32: every counted wait of the stream must fit the 6-bit vmcnt field");
    static_assert(BLOCK == 64, "one wave per 64-filter tile");
    static_assert(VelocityCut<T, N>::C_V >= RC::NCH - 1, "no early cut: see VelocityCut");
    const int b = blockIdx.x * BLOCK + threadIdx.x;
    const bool in = b < B;
    const size_t bc = in ? b : B - 1;                   // lanes past B run along on the last filter's inputs and store nothing
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc<T, N>(recs, my_tile());
    T nom[L::NNOM], P[RC::NCOVP];
    // the call's inputs first, without a branch: a call without gyro reads z in its place, one without skip
    // its applied flag (a byte of z is what the compiler takes out of the z load it already has, behind a wait)
    const T* gsrc = gyro ? gyro : z;
    T zin[3], gin[3];
    double vin[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        zin[i] = ld_once(z + 3 * bc + i);
        gin[i] = ld_once(gsrc + 3 * bc + i);
        vin[i] = ld_once(var + (var_stride ? 3 * bc : 0) + i);
    }
    const unsigned char skin = *(skip ? skip + bc : applied + bc);
    const double gate = thr[3];
    order_fence();
    load_chunks<T, N, 0, CN>(rs, my_lane(), nom);
    order_fence();
    load_chunks<T, N, CN, RC::NCH, FBUS_X_CORRECT_LD>(rs, my_lane(), P);
    order_fence();
    // the inputs become known to the compiler HERE, behind the loads (correct_depth_kernel says why)
    T zv[3] = { zin[0], zin[1], zin[2] }, gv[3] = { gin[0], gin[1], gin[2] };
    double varv[3] = { vin[0], vin[1], vin[2] };
    unsigned skv = skip ? (unsigned)skin : 0u;
    asm volatile("" : "+v"(zv[0]), "+v"(zv[1]), "+v"(zv[2]), "+v"(gv[0]), "+v"(gv[1]), "+v"(gv[2]));
    asm volatile("" : "+v"(varv[0]), "+v"(varv[1]), "+v"(varv[2]), "+v"(skv));
    const SensorOut<T> o{ applied, nis, dof, lik, B, b };
    // untouched lanes  (x > 0 is false for a NaN)
    bool usable = in && skv == 0u;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        usable = usable && isfinite((double)zv[i]) && isfinite(varv[i]) && varv[i] > 0.0;
        if (gyro) usable = usable && isfinite((double)gv[i]);
    }
    if (!usable) return leave_untouched(o, in);

    // h and the innovation in double; without gyro the lever does not enter (H_bg = C [0]x = 0)
    const T* R = nom + L::OFF_R;
    const double lv[3] = { gyro ? vs.lever[0] : 0.0, gyro ? vs.lever[1] : 0.0, gyro ? vs.lever[2] : 0.0 };
    double w[3], om[3], res[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        w[m] = (double)R[m] * (double)nom[L::OFF_V] + (double)R[3 + m] * (double)nom[L::OFF_V + 1] + (double)R[6 + m] * (double)nom[L::OFF_V + 2];
        om[m] = gyro ? (double)gv[m] - (double)nom[L::OFF_BG + m] : 0.0;
    }
    {
        const double y[3] = { w[0] + (om[1] * lv[2] - om[2] * lv[1]), w[1] + (om[2] * lv[0] - om[0] * lv[2]),
                              w[2] + (om[0] * lv[1] - om[1] * lv[0]) };
#pragma unroll
        for (int k = 0; k < 3; ++k) res[k] = (double)zv[k] - (vs.C[3 * k] * y[0] + vs.C[3 * k + 1] * y[1] + vs.C[3 * k + 2] * y[2]);
    }
    // row k of H on the V columns, rounded once to the record type: c R', c [w]x, c [lever]x with c = row k of C (the last is uniform)
    auto row = [&](int k, T* Hk) __attribute__((always_inline)) {
        const double c0 = vs.C[3 * k], c1 = vs.C[3 * k + 1], c2 = vs.C[3 * k + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) Hk[j] = (T)(c0 * (double)R[3 * j] + c1 * (double)R[3 * j + 1] + c2 * (double)R[3 * j + 2]);
        Hk[3] = (T)(c1 * w[2] - c2 * w[1]);
        Hk[4] = (T)(c2 * w[0] - c0 * w[2]);
        Hk[5] = (T)(c0 * w[1] - c1 * w[0]);
        Hk[6] = (T)(c1 * lv[2] - c2 * lv[1]);
        Hk[7] = (T)(c2 * lv[0] - c0 * lv[2]);
        Hk[8] = (T)(c0 * lv[1] - c1 * lv[0]);
    };
    // The two forms of the rows (the head of the file; the steps and their reasons: ekf_sensor.hpp).  fp32: P stays as loaded until its
    // one pass, 3 N doubles y_k beside it; fp64: rows one and two update P in registers, the third row's pass stores
    constexpr bool joint = sizeof(T) == 4;
    using A = SensorArith<T>;
    double Y[3][N], q[3];                                // fp32: y_k, q_k and the signs of s_k
    bool neg[3];
    T u[N], dk = T(0), dx[N];                            // fp64: the u and 1 / s of the row at hand; both: dx
    RowSums g;
    static_for<0, 3>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        __builtin_amdgcn_sched_barrier(0);
        T Hk[9];
        row(k, Hk);
        // P h_k by output row over the 9 V columns: P(:, V) is all a row reads
        A* w;
        if constexpr (joint) w = Y[k];
        else w = u;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            A acc = (A)P[pidx<N>(i, vcol(0))] * (A)Hk[0];
#pragma unroll
            for (int j = 1; j < 9; ++j) acc += (A)P[pidx<N>(i, vcol(j))] * (A)Hk[j];
            w[i] = acc;
        }
        if constexpr (joint) {
            joint_row<k, VCols, false>(Y, q, neg, dx, g, Hk, res[k], varv[k]);
        } else {
            seq_row<k, VCols>(u, dx, dk, g, Hk, res[k], varv[k], [](double&) {});
            if constexpr (k < 2) rank1_pass<T, N, false>(rs, P, u, dk);
        }
    });
    // the gate is decided behind the third row's s and r, before the first store
    report(o, g, 3);
    if (gate_shut(g, gate)) return leave_rejected(o, g, 3);
    inject<T, N>(nom, dx);
    store_nominal<T, N>(rs, nom);
    if constexpr (joint) {
        fresh<T, N>(P);
        joint_pass<T, N, 3>(rs, P, Y);
    } else {
        rank1_pass<T, N, true>(rs, P, u, dk);
    }
    leave_applied(o, g, 3);
}

}  // namespace

namespace fbus {
template <typename T, int N>
void launch_velocity_k(hipStream_t s, T* recs, int B, const T* z, const T* gyro, const double* var, int var_stride,
                       const unsigned char* skip, unsigned char* applied, const VelocitySensor& vs, const double* thr, T* nis, int* dof,
                       double* lik)
{
    launch_tile_k(correct_velocity_kernel<T, N>, s, B, recs, B, z, gyro, var, var_stride, skip, applied, vs, thr, nis, dof, lik);
}
}  // namespace fbus
