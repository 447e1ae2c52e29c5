// ekf_sensor.hpp -- the steps the streamed sensor updates share: correct_depth_kernel (ekf_depth.hpp), correct_velocity_kernel
// (ekf_velocity.hpp) and correct_rows_kernel (ekf_rows.hpp).  Each kernel keeps its own stream -- what it loads, in which order, and how
// it forms P h_k -- and takes from here, each written once: the exits and the gate rule, the store of the nominal state, the two row steps
// (fp32: joint form in double; fp64: sequential rows in the record type), the two covariance passes and the launch.  gfx950 only.
#pragma once
#include "ekf_group.hpp"        // pk_row / pk_col: (row, column) of a packed covariance element
#include "ekf_kernels.hpp"
#include "ekf_launch.hpp"        // DepthSensor, VelocitySensor and the launchers' declarations

namespace {

// one 16-byte chunk of registers made opaque where it stands (an empty asm): what was computed from it earlier is not kept alive for a
// later use of it, and a pass over it is finished where it is written
__device__ __forceinline__ void pin_chunk(float* p) { asm volatile("" : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3])); }
__device__ __forceinline__ void pin_chunk(double* p) { asm volatile("" : "+v"(p[0]), "+v"(p[1])); }

// The whole fp32 covariance made opaque, in front of a row or of the streamed pass: the compiler otherwise keeps the elements it widened
// for one row alive for the next and for the pass, two registers each beside the covariance they were converted from (fp32 velocity,
// N = 18: 188 B of scratch; 0 B with it)
template <typename T, int N>
__device__ __forceinline__ void fresh(T* P)
{
    static_for<0, (Lay<N>::NP + 3) / 4>([&](auto cc) { pin_chunk(P + 4 * decltype(cc)::value); });
}

// the type of the rows' arithmetic: double for both record types
template <typename T> using SensorArith = typename std::conditional<sizeof(T) == 4, double, T>::type;

// the columns of the error state a row of H has entries in: `n` of them, the k-th is state column col(k).  A row is stored on its
// set (n values).  VCols (ekf_velocity.hpp) is the other one.
template <int N>
struct DenseCols {
    static constexpr int n = N;
    static constexpr int col(int k) { return k; }
};

// ---- the exits -------------------------------------------------------------------------------------------------------------------------
// where lane b reports: the call's outputs (nis, dof and lik may be null), and what the rows have summed up for the gate
template <typename T>
struct SensorOut { unsigned char* applied; T* nis; int* dof; double* lik; int B, b; };
struct RowSums { double nisv = 0.0, detS = 1.0; bool pivots = true; };       // sum r_k^2 / s_k, prod s_k, every s_k > 0

// untouched: no store to the record, no likelihood term.  in: lanes past B report nothing
template <typename T>
__device__ __forceinline__ void leave_untouched(const SensorOut<T>& o, bool in = true)
{
    if (in) {
        o.applied[o.b] = 0;
        if (o.nis) o.nis[o.b] = T(0);
        if (o.dof) o.dof[o.b] = 0;
    }
}
// every usable lane reports nis and dof, in front of the gate
template <typename T>
__device__ __forceinline__ void report(const SensorOut<T>& o, const RowSums& g, int rows)
{
    if (o.nis) o.nis[o.b] = (T)g.nisv;
    if (o.dof) o.dof[o.b] = rows;
}
// THE gate rule: every pivot > 0 and nis <= gate = thr[rows].  Both comparisons are false for a NaN: a record of NaN and one with a
// negated covariance are not applied.  Decided before the first store to the record.  Stated as its negation, the test the kernels
// branch on: as `if (!gate_open(...))` the branch came out the other way round, and every code object with other registers
__device__ __forceinline__ bool gate_shut(const RowSums& g, double gate) { return !(g.pivots && g.nisv <= gate); }
// reported but not applied: nothing is stored to the record, the likelihood sums count a rejection
template <typename T>
__device__ __forceinline__ void leave_rejected(const SensorOut<T>& o, const RowSums& g, int rows)
{
    o.applied[o.b] = 0;
    if (o.lik) lik_add(LikOut{ o.lik, o.B }, o.b, false, g.nisv, 0.0, g.detS, rows);
}
template <typename T>
__device__ __forceinline__ void leave_applied(const SensorOut<T>& o, const RowSums& g, int rows)
{
    o.applied[o.b] = 1;
    if (o.lik) lik_add(LikOut{ o.lik, o.B }, o.b, true, g.nisv, 0.0, g.detS, rows);
}

// the injected nominal state goes out.  The carried rotation is NOT refreshed by a measurement update: chunks holding only R are left alone
template <typename T, int N>
__device__ __forceinline__ void store_nominal(__amdgpu_buffer_rsrc_t rs, const T* nom)
{
    store_chunks<T, N, 0, Rec<T, N>::CH_PQ, FBUS_X_CORRECT_ST>(rs, my_lane(), nom);
    store_chunks<T, N, Rec<T, N>::CH_PQR, Rec<T, N>::CH_NOM, FBUS_X_CORRECT_ST>(rs, my_lane(), nom + Lay<N>::NPQR);
    __builtin_amdgcn_sched_barrier(0);
}

// ---- fp32 records: THE JOINT FORM, its arithmetic in double, every covariance element rounded once ---------------------------------------
// An update that takes the velocity block from a prior of 0.1 (m/s)^2 to the sensor's 1e-4 subtracts numbers that agree in their first
// three digits: P - u u' / s in fp32 keeps eps32 x prior / posterior of the result (4e-4 block-wise on the suite's states, sequential
// and joint alike), and fp32 roundings of P between the rows still leave 3e-5.  So P stays as loaded until its one pass
// and the rows are orthogonalised instead: w_k = P h_k - sum_{j<k} w_j (w_j . h_k) / s_j is the sequential form's u_k, from the ORIGINAL P.
// Kept as y_k = w_k / sqrt(s_k):  P+ = P - sum y_k y_k',  dx = sum y_k q_k,  q_k = r_k / sqrt(s_k),  r_k = res_k - sum_{j<k} (h_k . y_j) q_j,
// nis = sum q_k^2.  M N doubles beside the fp32 covariance (velocity, N = 18: 256 + 186 registers, no scratch).
// A pivot that is not > 0 (a record whose covariance is not positive definite) ends in "not applied", and its lane still reports
// nis = sum r_k^2 / s_k as the fp64 form and the header have it: the roots are taken of |s_k| and the sign of s_k goes with the
// products -- w_j (w_j . h_k) / s_j = sgn_j y_j (y_j . h_k), r_k^2 / s_k = sgn_k q_k^2.  With every pivot > 0 each sign is a
// select that keeps its operand: the same bits as without them.
// Row k, behind the kernel's own Y[k] = P h_k (from the P as loaded).  Hk: the row on Cols; r: res_k; q[k] = r_k / sqrt(|s_k|); neg[k]: s_k < 0.
// Y, q, neg and dx are arrays of the kernel's own, each handed over by itself: as members of one struct the compiler knows that a store
// to Y leaves q alone, keeps q[k] in a register across the last loop, and the fp32 code objects come out with the operands of that loop's
// products the other way round.
// FINISH: the row is finished HERE, behind q[k] -- arithmetic is not tied to its place by order_fence(), and a kernel that requests rows
// of H or the nominal state between its rows needs it (correct_rows_kernel says what happened without)
template <int k, typename Cols, bool FINISH, typename T, int N, int M>
__device__ __forceinline__ void joint_row(double (&Y)[M][N], double (&q)[M], bool (&neg)[M], T (&dx)[N], RowSums& g, const T* Hk, double r,
                                          double vark)
{
#pragma unroll
    for (int j = 0; j < k; ++j) {
        double c = 0.0;
#pragma unroll
        for (int m = 0; m < Cols::n; ++m) c += (double)Hk[m] * Y[j][Cols::col(m)];
        c = neg[j] ? -c : c;
#pragma unroll
        for (int i = 0; i < N; ++i) Y[k][i] -= Y[j][i] * c;
        r -= c * q[j];
    }
    double hph = 0.0;
#pragma unroll
    for (int m = 0; m < Cols::n; ++m) hph += (double)Hk[m] * Y[k][Cols::col(m)];
    const double s = hph + vark, rsq = 1.0 / sqrt(fabs(s));
    g.pivots = g.pivots && s > 0.0;
    neg[k] = s < 0.0;
    q[k] = r * rsq;
    if constexpr (FINISH) asm volatile("" : "+v"(q[k]));
    // nisv += sgn_k q_k^2, written out in the order the plain sum q_0^2 + q_1^2 + q_2^2 contracts to (ll keeps its last bit):
    // q_0^2 is fused into the rounded q_1^2, every later term is fused into the sum
    auto sq = [&](int j) __attribute__((always_inline)) { return neg[j] ? -q[j] : q[j]; };
    if constexpr (k == 0 && M == 1) g.nisv = sq(0) * q[0];
    if constexpr (k == 1) g.nisv = fma(sq(0), q[0], sq(1) * q[1]);
    if constexpr (k >= 2) g.nisv = fma(sq(k), q[k], g.nisv);
    g.detS *= s;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        Y[k][i] *= rsq;
        dx[i] = k > 0 ? dx[i] + (T)(Y[k][i] * q[k]) : (T)(Y[k][i] * q[k]);
    }
}
// The streamed pass: chunk c takes its elements' M terms, one rounding, then its store (prev_id and the padding behind it go back as
// they came).  Y: M rows y_k; the depth update is M = 1.  The scheduling barrier keeps one chunk's work together
template <typename T, int N, int M>
__device__ __forceinline__ void joint_pass(__amdgpu_buffer_rsrc_t rs, T* P, const double (*Y)[N])
{
    using RC = Rec<T, N>;
    static_for<RC::CH_NOM, RC::NCH>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
#pragma unroll
        for (int k = 0; k < RC::EPC; ++k) {
            constexpr int e0 = (c - RC::CH_NOM) * RC::EPC;
            const int e = e0 + k;
            if (e < Lay<N>::NP) {
                double a = (double)P[e];
#pragma unroll
                for (int m = 0; m < M; ++m) a -= Y[m][pk_row<N>(e)] * Y[m][pk_col<N>(e)];
                P[e] = (T)a;
            }
        }
        store_chunks<T, N, c, c + 1, FBUS_X_CORRECT_ST>(rs, my_lane(), P + (c - RC::CH_NOM) * RC::EPC);
        __builtin_amdgcn_sched_barrier(0);
    });
}

// ---- fp64 records: the sequential rows, in the record type: one u is alive at a time -------------------------------------------------------
// Row k, behind the kernel's own u = P h_k (from the P the earlier rows left); dk: 1 / s_k for the row's rank-1 pass.  row_done(is):
// called with 1 / s_k once the row of H has been used up, in front of the sums -- where a kernel places its next request
template <int k, typename Cols, typename T, int N, typename F>
__device__ __forceinline__ void seq_row(T (&u)[N], T (&dx)[N], T& dk, RowSums& g, const T* Hk, double resk, double vark, F&& row_done)
{
    double hph = 0.0, hdx = 0.0;
#pragma unroll
    for (int j = 0; j < Cols::n; ++j) {
        hph += (double)Hk[j] * (double)u[Cols::col(j)];
        if (k > 0) hdx += (double)Hk[j] * (double)dx[Cols::col(j)];
    }
    const double s = hph + vark, r = resk - hdx;
    double is = 1.0 / s;
    row_done(is);
    g.pivots = g.pivots && s > 0.0;
    g.nisv += r * r * is;
    g.detS *= s;
    const T gn = (T)(r * is);
    dk = (T)is;
#pragma unroll
    for (int i = 0; i < N; ++i) dx[i] = k > 0 ? dx[i] + u[i] * gn : u[i] * gn;
    __builtin_amdgcn_sched_barrier(0);
}
// Chunks C0..C1 of the covariance take the rank-1 term u u' dk of the row at hand.  STORE: the last row's pass, each chunk stored behind
// its own arithmetic (prev_id and the padding behind it go back as they came); otherwise the chunk is pinned where the pass leaves it: a
// pass whose result only the applied branch uses is sunk behind the gate by the compiler, and its u vector with it.  The scheduling
// barriers keep one row's work, and one chunk's, together: without them the scheduler forms all three rows of H and the scaled u of
// every chunk ahead of their use, and the fp32 N = 18 velocity kernel spilled 704 B
template <typename T, int N, bool STORE, int C0 = Rec<T, N>::CH_NOM, int C1 = Rec<T, N>::NCH>
__device__ __forceinline__ void rank1_pass(__amdgpu_buffer_rsrc_t rs, T* P, const T* u, T dk)
{
    using RC = Rec<T, N>;
    static_for<C0, C1>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
#pragma unroll
        for (int k = 0; k < RC::EPC; ++k) {
            constexpr int e0 = (c - RC::CH_NOM) * RC::EPC;
            const int e = e0 + k;
            if (e < Lay<N>::NP) P[e] -= (u[pk_row<N>(e)] * dk) * u[pk_col<N>(e)];
        }
        if constexpr (STORE) store_chunks<T, N, c, c + 1, FBUS_X_CORRECT_ST>(rs, my_lane(), P + (c - RC::CH_NOM) * RC::EPC);
        else pin_chunk(P + (c - RC::CH_NOM) * RC::EPC);
        __builtin_amdgcn_sched_barrier(0);
    });
}

// grid: one wave per 64-filter tile; args: the kernel's arguments
template <typename... KP, typename... A>
void launch_tile_k(void (*kernel)(KP...), hipStream_t st, int B, A... args)
{
    hipLaunchKernelGGL(kernel, dim3((B + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, args...);
}

}  // namespace
