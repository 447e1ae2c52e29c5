// ekf_rows.hpp -- the general linearised measurement update (fbus_ekf_correct_rows*, include/fbus_ekf.h): the caller hands over the
// innovation and the Jacobian rows, the library does the gain, the injection, the covariance, the NIS, the gate and the likelihood.
// No reference counterpart (the reference has its pose rows and nothing else); the algebra is stated in the header.  Included by
// small_tu.hip's sensor family only.  gfx950 only.
//
// M rows (1..FBUS_ROWS_MAX) with DENSE H, every column of the error state p v theta ba bg [g] may be in play:
//     S = H P H' + diag(var)      U = P H'      dx = U S^-1 res -> inject()      P <- P - U S^-1 U'
// The rows are processed one after the other at the caller's one linearisation point, exactly as correct_velocity_kernel does it, and
// the two record types take the same two forms of it:
//   fp64  the sequential rows in the record type: u = P h_k, s_k = h_k . u + var_k, r_k = res_k - h_k . dx, dx += u r_k / s_k,
//         P -= u u' / s_k; the last row's rank-1 term is applied chunk by chunk, each chunk stored behind its own arithmetic.
//   fp32  the joint form with its arithmetic in DOUBLE and one rounding per covariance element: the rows are orthogonalised against each
//         other from the ORIGINAL P (y_k = w_k / sqrt(s_k), w_k = P h_k - sum_{j<k} y_j (y_j . h_k)) and P takes P - sum y_k y_k' in one
//         streamed pass.  M N doubles beside the fp32 covariance.
// nis = sum r_k^2 / s_k and det S = prod s_k in both; the s_k are the squares of the Cholesky pivots of S.
//
// Mapping and stream as correct_velocity_kernel: one filter per lane, one wave per 64-filter tile, one buffer descriptor per tile -- at
// every batch size.  res, var and skip are requested first, then every record chunk in use order: the covariance, and the nominal state
// last (below).  u = P h reads ALL of P: nothing starts before the whole covariance has landed.
//
// Where the loads of H go.  Row k (N elements of the record type, natural alignment only: N scalar loads) is needed only while row k is
// formed.  Requested with the inputs, in front of the record stream, M N loads would stand in front of NCH record loads and the wait for
// the first of them would count NCH + M N + ... operations: 104 for fp32 N = 18, M = 3, past the 6-bit vmcnt field.  Requested where it
// is used, a row would expose a trip to L2 / HBM behind the stream.  So:
//   row 0      is requested BEHIND the record loads, after the wait for res / var / skip (which were requested first and are back long
//              before the records: that wait counts the covariance loads behind them -- 43 for fp32 N = 18 -- and costs nothing).  It travels while the record stream
//              arrives and is there when the last chunk is.
//   row k + 1  fp32: is requested at the head of row k's arithmetic (N^2 double multiply-adds and their conversions: some thousands of
//              cycles), which hides it; at most two rows, 2 N registers, are alive at once.  fp64, where the covariance alone is 342
//              registers: behind row k's pivot, when row k has been used up; it travels behind row k's rank-1 pass over the covariance.
// Every counted wait is then small: the covariance chunks at the inputs, N (the one row in flight) at a row, the stores' own counts in
// the pass (largest in the fp32 ISA: 45).
// Where the loads of the nominal state go.  The rows do not read it: it is needed for the injection behind the gate and nowhere else, so
// "use order" puts its chunks LAST, and they are requested late: fp32 at the head of the last row's arithmetic (hidden behind it), fp64
// behind the last row's pivot, where the row of H has been used up (exposed: one trip to memory per wave in front of the gate).  The
// first version requested them with the covariance, as correct_velocity_kernel must (it forms H from R and v), and carried 28 / 56
// registers of nominal state across every row: the fp64 N = 18, M = 1 and N = 15, M = 3 code objects then came out of the register
// allocator with one dword of a nominal chunk lost -- the chunk split into a 12-byte scratch slot and a register copy that nothing read
// again, the injection taking q_w's high half from a register that held a covariance element (read in the ISA; the parity test showed a
// wrong quaternion in every lane, the N = 15 test a g_z that was not bit-equal).  Nothing of the nominal state is alive across a row now.
// A lane that is skipped, has a non-finite residual or a var that is not a finite number > 0 leaves behind the wait for the inputs;
// one with a non-finite entry of H is found row by row and leaves at the gate: none of them stores to its record.  The gate -- M
// pivots > 0 and nis <= thr[M] -- is decided behind the last row's s and r, before the first store; then the injected nominal state goes
// out and the covariance chunks follow in storage order.  No early exit in front of the record loads (correct_depth_kernel's reason).
#pragma once
#include "ekf_sensor.hpp"       // the exits and the gate rule, store_nominal, the two row steps and covariance passes, launch_tile_k

namespace {

// nis / dof (each may be null), lik (null while the likelihood sums are off) and thr (the handle's gate table, +inf without one) are
// arguments of the one instantiation, as in correct_velocity_kernel: the plain, _nis and likelihood-on calls run the same code object.
// H is not __restrict__: its loads stand behind order_fence(), whose memory clobber must cover them (see correct_depth_kernel on recs).
template <typename T, int N, int M>
__global__ void __launch_bounds__(BLOCK, 1)
correct_rows_kernel(T* recs /* not __restrict__: see correct_depth_kernel */, int B, const T* __restrict__ res, const T* H,
                    const double* __restrict__ var, int var_stride, const unsigned char* __restrict__ skip,
                    unsigned char* __restrict__ applied, const double* __restrict__ thr, T* __restrict__ nis, int* __restrict__ dof,
                    double* __restrict__ lik)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    constexpr int CN = RC::CH_NOM;
    static_assert(M >= 1 && M <= 3, "FBUS_ROWS_MAX");
    // The waits are the compiler's counted vmcnt.  The largest count of the fp32 forms is the wait for the 2 M + 1 input loads behind the
    // record loads (at most NCH: 57 for N = 18, M = 3); a row of H waits behind at most the one row requested after it (N).  The fp64 records have
    // 100 / 77 chunks, there a larger count is clamped to 63: early, never late.
    static_assert(sizeof(T) == 8 || RC::NCH + 2 * M + 1 <= 63, "fp32: every counted wait of the stream must fit the 6-bit vmcnt field");
    static_assert(N <= 63, "a row of H in flight behind the row in use");
    static_assert(BLOCK == 64, "one wave per 64-filter tile");
    const int b = blockIdx.x * BLOCK + threadIdx.x;
    const bool in = b < B;
    const size_t bc = in ? b : B - 1;                   // lanes past B run along on the last filter's inputs and store nothing
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc<T, N>(recs, my_tile());
    T nom[L::NNOM], P[RC::NCOVP];
    // the call's inputs first, without a branch: a call without skip reads its applied flag in its place
    T rin[M];
    double vin[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        rin[i] = ld_once(res + M * bc + i);
        vin[i] = ld_once(var + (var_stride ? M * bc : 0) + i);
    }
    const unsigned char skin = *(skip ? skip + bc : applied + bc);
    const double gate = thr[M];
    order_fence();
    load_chunks<T, N, CN, RC::NCH, FBUS_X_CORRECT_LD>(rs, my_lane(), P);
    order_fence();
    // the nominal chunks are NOT requested here: the rows do not read them (res and H are the caller's), see request_nom below
    auto request_nom = [&]() __attribute__((always_inline)) {
        // (without the chunks that hold only the carried rotation: nothing here reads R, and a measurement update does not store it)
        load_chunks<T, N, 0, RC::CH_PQ>(rs, my_lane(), nom);
        load_chunks<T, N, RC::CH_PQR, CN>(rs, my_lane(), nom + L::NPQR);
        order_fence();
    };
    // the inputs become known to the compiler HERE, behind the record loads (correct_depth_kernel says why)
    T rv[M];
    double varv[M];
    unsigned skv = skip ? (unsigned)skin : 0u;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        rv[i] = rin[i];
        varv[i] = vin[i];
        asm volatile("" : "+v"(rv[i]), "+v"(varv[i]));
    }
    asm volatile("" : "+v"(skv));
    // row 0 of H: behind the record stream, in front of the branch
    const T* Hb = H + bc * (size_t)(M * N);
    T Hr[M][N];
    auto request = [&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
#pragma unroll
        for (int j = 0; j < N; ++j) Hr[k][j] = ld_once(Hb + k * N + j);
    };
    request(std::integral_constant<int, 0>{});
    order_fence();
    const SensorOut<T> o{ applied, nis, dof, lik, B, b };
    // untouched lanes  (x > 0 is false for a NaN)
    bool usable = in && skv == 0u;
#pragma unroll
    for (int i = 0; i < M; ++i) usable = usable && isfinite((double)rv[i]) && isfinite(varv[i]) && varv[i] > 0.0;
    if (!usable) return leave_untouched(o, in);

    // The two forms of the rows (the head of the file; the steps and their reasons: ekf_sensor.hpp).  fp32: P stays as loaded until its
    // one pass, M N doubles y_k beside it; fp64: every row but the last updates P in registers, the last row's pass stores
    constexpr bool joint = sizeof(T) == 4;
    double Y[M][N], q[M];                                // fp32: y_k, q_k and the signs of s_k
    bool neg[M];
    T u[N], dk = T(0), dx[N];                            // fp64: the u and 1 / s of the row at hand; both: dx
    RowSums g;
    bool hfin = true;
    static_for<0, M>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (joint) {
            if constexpr (k + 1 < M) {
                request(std::integral_constant<int, k + 1>{});
                order_fence();
            }
            if constexpr (k == M - 1) request_nom();       // behind this row's N^2 multiply-adds
            if constexpr (k > 0) fresh<T, N>(P);           // in front of every row but the first
        }
        const T* Hk = Hr[k];
#pragma unroll
        for (int j = 0; j < N; ++j) hfin = hfin && isfinite(Hk[j]);
        if constexpr (joint) {
            // w = P h_k, element by packed element in storage order: each is widened ONCE and goes to the two sums it belongs to (one on
            // the diagonal).  A scheduling barrier per chunk: the scheduler otherwise widens the whole covariance ahead of the sums, two
            // registers an element (fp32 N = 18, M = 3 by output row: 1172 B of scratch)
#pragma unroll
            for (int i = 0; i < N; ++i) Y[k][i] = 0.0;
            static_for<0, (L::NP + 3) / 4>([&](auto cc) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    constexpr int e0 = 4 * decltype(cc)::value;
                    const int e = e0 + t;
                    if (e < L::NP) {
                        const double a = (double)P[e];
                        Y[k][pk_row<N>(e)] += a * (double)Hk[pk_col<N>(e)];
                        if (pk_row<N>(e) != pk_col<N>(e)) Y[k][pk_col<N>(e)] += a * (double)Hk[pk_row<N>(e)];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            });
            // finished behind q[k]: without it the compiler sinks every row's sums behind the requests of all the rows of H and of the
            // nominal state (seen in the ISA: 15 global loads and the nominal chunks in front of the first row, 54 + 28 registers carried
            // through all of it)
            joint_row<k, DenseCols<N>, true>(Y, q, neg, dx, g, Hk, (double)rv[k], varv[k]);
        } else {
            static_for<0, N>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                T acc = P[pidx<N>(i, 0)] * Hk[0];
#pragma unroll
                for (int j = 1; j < N; ++j) acc += P[pidx<N>(i, j)] * Hk[j];
                u[i] = acc;
            });
            seq_row<k, DenseCols<N>>(u, dx, dk, g, Hk, (double)rv[k], varv[k], [&](double& is) __attribute__((always_inline)) {
                // The row of H is done with, and the next request takes its registers: row k + 1 (it travels behind this row's rank-1
                // pass), or the nominal state.  One row, N values, is alive at a time beside a covariance of 342 registers.  The row's
                // sums are finished here, in front of the request (see the fp32 rows)
                asm volatile("" : "+v"(is));
                if constexpr (k + 1 < M) {
                    request(std::integral_constant<int, k + 1>{});
                    order_fence();
                } else {
                    request_nom();
                }
            });
            if constexpr (k + 1 < M) rank1_pass<T, N, false>(rs, P, u, dk);
        }
    });
    // a lane with a non-finite entry of H is untouched too; it is known once the last row is in
    if (!hfin) return leave_untouched(o);
    report(o, g, M);
    if (gate_shut(g, gate)) return leave_rejected(o, g, M);
    inject<T, N>(nom, dx);
    store_nominal<T, N>(rs, nom);
    if constexpr (joint) {
        fresh<T, N>(P);
        joint_pass<T, N, M>(rs, P, Y);
    } else {
        rank1_pass<T, N, true>(rs, P, u, dk);
    }
    leave_applied(o, g, M);
}

}  // namespace

namespace fbus {
template <typename T, int N>
void launch_rows_k(hipStream_t s, T* recs, int B, int m, const T* res, const T* H, const double* var, int var_stride,
                   const unsigned char* skip, unsigned char* applied, const double* thr, T* nis, int* dof, double* lik)
{
    const auto go = [&](auto mc) {
        launch_tile_k(correct_rows_kernel<T, N, decltype(mc)::value>, s, B, recs, B, res, H, var, var_stride, skip, applied, thr, nis, dof, lik);
    };
    switch (m) {
    case 1: go(std::integral_constant<int, 1>{}); break;
    case 2: go(std::integral_constant<int, 2>{}); break;
    default: go(std::integral_constant<int, 3>{}); break;
    }
}
}  // namespace fbus
