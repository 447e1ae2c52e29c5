// ekf_group.hpp -- hypothesis groups: evidence-weighted fusion, collapse and IMM mixing (fbus_ekf_group_fuse / fbus_ekf_group_collapse /
// fbus_ekf_group_mix, include/fbus_ekf.h).  No reference counterpart: the reference runs one filter on one thread (C++/src/filter.cpp:190-250).
// Its kernels are instantiated by small_tu.hip's group family only; the sensor and report headers take pk_row / pk_col and group_delta from
// here.  gfx950 only.
//
// Mapping: ONE FILTER PER LANE, as everywhere.  Group j = filters j G .. j G + G - 1; a wave serves floor(64 / G) whole groups: lane l is
// member l % G of its (l / G)-th group, lanes past floor(64 / G) * G idle.  A group never spans two waves, which is what makes collapse
// race-free in place: a wave loads chunk c of its sources before it stores chunk c, and no other wave touches its filters.  For G not
// dividing 64 a wave's filters straddle two 64-filter tiles: the buffer descriptor covers the two tiles from the first filter's on
// (cut at the end of the records) and lane offsets are (b / 64) NCH 1024 + c 1024 + (b % 64) 16 relative to it -- every access is still
// a run of contiguous 16-byte chunks.
//
// Every cross-lane sum goes through LDS in MEMBER ORDER (group_reduce): the lanes write their terms, then one lane per (group, element)
// adds the G terms of its group from member 0 up.  The order does not depend on the batch or on where the group sits in the wave, so two
// calls on the same inputs are bit-identical.  A workgroup is one wave: LDS accesses of a wave complete in issue order, so a
// wavefront-scope fence (no instruction, no wait on the record loads in flight) orders writers and readers.
#pragma once
#include "ekf_kernels.hpp"

namespace {

static_assert(BLOCK == 64, "the group kernels are one wave per workgroup");
static_assert(FBUS_GROUP_MAX == 64, "a group never spans two waves");

__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the wave's place in the batch: b0 = its first filter, a descriptor over the (up to) two tiles its filters lie in, and the lane's
// byte offset of chunk 0 inside it
template <typename T, int N>
struct GroupMap {
    static constexpr unsigned TILE_BYTES = Rec<T, N>::NCH * 1024u;
    int lane, ngw, mem, gbase;          // groups per wave; this lane's member index and its group's first lane
    long long b;                        // this lane's filter
    long long g0;                       // the wave's first group
    int nvg;                            // whole groups of this wave inside the batch
    bool act;                           // the lane has a filter
    unsigned voff;
    __amdgpu_buffer_rsrc_t rs;
    __device__ __forceinline__ GroupMap(const T* recs, size_t rec_bytes, int B, int G)
    {
        lane = (int)threadIdx.x;
        ngw = 64 / G;
        const long long b0 = (long long)blockIdx.x * (ngw * G);
        b = b0 + lane;
        act = lane < ngw * G && b < B;
        mem = act ? lane % G : 0;
        gbase = act ? lane - mem : 0;
        g0 = b0 / G;
        const long long left = ((long long)B - b0) / G;
        nvg = (int)(left < ngw ? left : ngw);
        const size_t t0 = (size_t)(b0 >> 6);
        const size_t base = t0 * TILE_BYTES;
        const size_t span = rec_bytes - base < 2 * (size_t)TILE_BYTES ? rec_bytes - base : 2 * (size_t)TILE_BYTES;
        const unsigned r = (unsigned)(b0 & 63) + (unsigned)lane;               // < 128
        // (idle lanes past the records read zeros through the descriptor's bound and store nothing)
        voff = (r >> 6) * TILE_BYTES + (r & 63u) * 16u;
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(recs)) + base, 0, (int)span, 0x00020000);
    }
    template <int C0, int C1>
    __device__ __forceinline__ void load(T* dst) const
    {
        constexpr int EPC = Rec<T, N>::EPC;
#pragma unroll
        for (int c = C0; c < C1; ++c) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff + (unsigned)c * 1024u, 0, AUX_DEFAULT);
            const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int k = 0; k < EPC; ++k) dst[(c - C0) * EPC + k] = e[k];
        }
    }
};

// (row, column) of packed covariance element q (the inverse of pidx<N>), -1 for the previous-marker id and the padding behind it
template <int N>
struct PkInv {
    static constexpr int NQ = Lay<N>::NP + 8;
    signed char row[NQ], col[NQ];
    constexpr PkInv() : row{}, col{}
    {
        for (int q = 0; q < NQ; ++q) row[q] = col[q] = -1;
        for (int i = 0; i < N; ++i)
            for (int j = i; j < N; ++j) { row[pidx<N>(i, j)] = (signed char)i; col[pidx<N>(i, j)] = (signed char)j; }
    }
};
template <int N> inline constexpr PkInv<N> pk_inv{};
template <int N> __host__ __device__ constexpr int pk_row(int q) { return pk_inv<N>.row[q]; }
template <int N> __host__ __device__ constexpr int pk_col(int q) { return pk_inv<N>.col[q]; }
// does 16-byte chunk c (counted from the first covariance chunk) hold a diagonal element?
template <typename T, int N>
__host__ __device__ constexpr bool chunk_has_diag(int c)
{
    for (int k = 0; k < Rec<T, N>::EPC; ++k) {
        const int q = c * Rec<T, N>::EPC + k;
        if (q < Lay<N>::NP && pk_row<N>(q) == pk_col<N>(q)) return true;
    }
    return false;
}

constexpr int GROUP_EB = 16;            // covariance elements per reduction batch
constexpr int GROUP_ROWS = 18;          // rows of the term buffer: a batch, or the N entries of mu
constexpr int GROUP_TP = 65;            // pitch of one element's 64 terms (odd: the readers of neighbouring elements hit different banks)

// The packed covariance in batches of GROUP_EB elements, as group_fuse_kernel (full covariance) and group_mix_kernel walk it: batch k is
// the chunks c0(k) .. c1(k) - 1 of the record; fetch<k> requests it into pb[k] and does nothing behind the last batch
template <typename T, int N>
struct GroupBatches {
    static constexpr int EPC = Rec<T, N>::EPC, CN = Rec<T, N>::CH_NOM;
    static constexpr int CB = GROUP_EB / EPC;                               // chunks per batch
    static constexpr int NCC = (Lay<N>::NP + EPC - 1) / EPC;                // covariance chunks that hold an element of P
    static constexpr int NB = (NCC + CB - 1) / CB;
    static constexpr int c0(int k) { return CN + k * CB; }
    static constexpr int c1(int k) { return (k + 1) * CB < NCC ? CN + (k + 1) * CB : CN + NCC; }
    template <int k>
    static __device__ __forceinline__ void fetch(const GroupMap<T, N>& gm, T (*pb)[GROUP_EB])
    {
        if constexpr (k < NB) gm.template load<c0(k), c1(k)>(pb[k]);
    }
};

// term[e * GROUP_TP + lane], e < ECNT, written by every lane  ->  sink(group, e, sum over the group's members in member order).
// A lane without a share wrote -0.0, which changes no sum (not even one that is -0.0 itself).
template <int ECNT, typename SINK>
__device__ __forceinline__ void group_reduce(const double* term, int lane, int ngw, int G, SINK sink)
{
    wave_lds_fence();
    for (int o = lane; o < ngw * ECNT; o += 64) {
        const int g = o / ECNT, e = o - g * ECNT;
        const double* t = term + e * GROUP_TP + g * G;
        double acc = -0.0;
        for (int j = 0; j < G; ++j) acc += t[j];
        sink(g, e, acc);
    }
    wave_lds_fence();
}

// steps 1, 2 of fuse as mix takes them: this lane's weight in double -- exactly 0 for a member that is not usable and for an idle lane --
// and bi, the group's best member (-1: no usable member, or an idle lane).  wsh: 64 doubles of LDS, free again on return.
// (group_fuse_kernel keeps the same lines inline: calling this from it changes its instruction stream, group_delta does not.)
template <typename GM>
__device__ __forceinline__ double group_weight(const GM& gm, const double* __restrict__ logw, double* wsh, int G, int& bi)
{
    const int lane = gm.lane;
    const double lw = gm.act ? logw[gm.b] : __builtin_nan("");
    const bool usable = gm.act && __builtin_isfinite(lw);
    wsh[lane] = lw;
    wave_lds_fence();
    double m = 0.0;
    bi = -1;
    for (int j = 0; j < G; ++j) {
        const double v = wsh[gm.gbase + j];
        if (__builtin_isfinite(v) && (bi < 0 || v > m)) { m = v; bi = j; }      // (strict: ties go to the first member)
    }
    if (!gm.act) bi = -1;
    const double ew = usable ? exp(lw - m) : 0.0;
    wave_lds_fence();
    wsh[lane] = ew;
    wave_lds_fence();
    double s = 0.0;
    for (int j = 0; j < G; ++j) s += wsh[gm.gbase + j];
    return (usable && bi >= 0) ? ew / s : 0.0;
}

// where a member's components sit: in a record (Lay<N>), or in an array in the order of fbus_ekf_get_state (p3 v3 q4 ba3 bg3 g3)
struct ApiOrder { static constexpr int OFF_P3 = 0, OFF_V = 3, OFF_Q = 6, OFF_BA = 10, OFF_BG = 13, OFF_G = 16; };
// step 3: this member's error state dl (order p v theta ba bg [g]) against the chart xs, in double for both record types.
// The member is nom, of type TM and laid out as ML says: a record's nominal part, or (ekf_nees.hpp) a truth row in double
template <typename T, int N, typename ML = Lay<N>, typename TM = T>
__device__ __forceinline__ void group_delta(const TM* nom, const T* xs, double* dl)
{
    using L = Lay<N>;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        dl[i] = (double)nom[ML::OFF_P3 + i] - (double)xs[L::OFF_P3 + i];
        dl[3 + i] = (double)nom[ML::OFF_V + i] - (double)xs[L::OFF_V + i];
        dl[9 + i] = (double)nom[ML::OFF_BA + i] - (double)xs[L::OFF_BA + i];
        dl[12 + i] = (double)nom[ML::OFF_BG + i] - (double)xs[L::OFF_BG + i];
        if constexpr (N == 18) dl[15 + i] = (double)nom[ML::OFF_G + i] - (double)xs[L::OFF_G + i];
    }
    {   // dtheta = Log(conj(q*) (x) q), in double for both record types: the inverse of inject()'s q <- normalize(q (x) dq(dtheta))
        const double qc[4] = { (double)xs[L::OFF_Q], -(double)xs[L::OFF_Q + 1], -(double)xs[L::OFF_Q + 2], -(double)xs[L::OFF_Q + 3] };
        const double qi[4] = { (double)nom[ML::OFF_Q], (double)nom[ML::OFF_Q + 1], (double)nom[ML::OFF_Q + 2], (double)nom[ML::OFF_Q + 3] };
        double d[4];
        quat_mul(qc, qi, d);
        if (d[0] < 0.0) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; d[3] = -d[3]; }
        const double n = sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
        const double k = n == 0.0 ? 0.0 : 2.0 * atan2(n, d[0]) / n;
        dl[6] = k * d[1]; dl[7] = k * d[2]; dl[8] = k * d[3];
    }
}

// dynamic LDS of group_fuse_kernel in bytes (the launcher passes it)
template <typename T, int N>
__host__ __device__ constexpr size_t group_fuse_lds(int ngw)
{
    return (size_t)(GROUP_ROWS * GROUP_TP + 64 + ngw * N) * sizeof(double) + (size_t)ngw * (Lay<N>::NP | 1) * sizeof(T) + (size_t)N * N * sizeof(short);
}

// FULL: the dense covariance (and pdiag from it); otherwise the diagonal alone, from the chunks that hold one.
template <typename T, int N, bool FULL>
__global__ void __launch_bounds__(BLOCK)
group_fuse_kernel(const T* __restrict__ recs, size_t rec_bytes, int B, int G, const double* __restrict__ logw, double* __restrict__ weight,
                  int* __restrict__ best, T* __restrict__ nominal, T* __restrict__ P, T* __restrict__ pdiag)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    using IO = TileIO<T, N>;
    constexpr int CN = RC::CH_NOM, EPC = RC::EPC, NP = L::NP, PKP = NP | 1;
    extern __shared__ double group_lds[];
    const GroupMap<T, N> gm(recs, rec_bytes, B, G);
    const int lane = gm.lane, ngw = gm.ngw;
    double* term = group_lds;                               // [GROUP_ROWS][GROUP_TP]
    double* wsh = term + GROUP_ROWS * GROUP_TP;             // [64]
    double* mu = wsh + 64;                                  // [ngw][N]
    T* pk = reinterpret_cast<T*>(mu + ngw * N);             // [ngw][PKP]: the fused packed covariance (the diagonal alone: [ngw][PKP] by row)
    short* tab = reinterpret_cast<short*>(pk + ngw * PKP);  // [N * N] -> packed index

    // the nominal chunks are requested first: the weights below cover their latency
    T nom[L::NNOM];
    gm.template load<0, CN>(nom);

    // ---- steps 1, 2: weights and the best member, in double -------------------------------------------------------------------------
    const double lw = gm.act ? logw[gm.b] : __builtin_nan("");
    const bool usable = gm.act && __builtin_isfinite(lw);
    wsh[lane] = lw;
    wave_lds_fence();
    double m = 0.0;
    int bi = -1;
    for (int j = 0; j < G; ++j) {
        const double v = wsh[gm.gbase + j];
        if (__builtin_isfinite(v) && (bi < 0 || v > m)) { m = v; bi = j; }      // (strict: ties go to the first member)
    }
    if (!gm.act) bi = -1;
    const double ew = usable ? exp(lw - m) : 0.0;
    wave_lds_fence();
    wsh[lane] = ew;
    wave_lds_fence();
    double s = 0.0;
    for (int j = 0; j < G; ++j) s += wsh[gm.gbase + j];
    const bool none = bi < 0;                               // no usable member: member 0's own values are copied
    const double w = (usable && !none) ? ew / s : 0.0;
    if (gm.act && weight) weight[gm.b] = w;
    if (gm.act && best && gm.mem == 0) best[gm.b / G] = bi;
    const double weff = !gm.act ? 0.0 : (none ? (gm.mem == 0 ? 1.0 : 0.0) : w);
    const bool share = weff != 0.0;                         // step 6: everything a weightless member would add is replaced by a select
    const int src = gm.gbase + (none ? 0 : bi);

    // ---- step 3: the chart x* from the best lane, this member's error state against it ----------------------------------------------
    T xs[L::NNOM];
#pragma unroll
    for (int e = 0; e < L::NNOM; ++e) xs[e] = (e >= L::OFF_R && e < L::OFF_R + 9) ? T(0) : __shfl(nom[e], src);
    double dl[N];
    group_delta<T, N>(nom, xs, dl);

    // ---- step 4: mu = sum w_i delta_i, the fused nominal state ----------------------------------------------------------------------
#pragma unroll
    for (int a = 0; a < N; ++a) term[a * GROUP_TP + lane] = share ? weff * dl[a] : -0.0;
    group_reduce<N>(term, lane, ngw, G, [&](int g, int a, double acc) { mu[g * N + a] = acc; });
    double d[N];                                            // delta_i - mu
    T dx[N];
#pragma unroll
    for (int a = 0; a < N; ++a) {
        const double ma = mu[(gm.gbase / G) * N + a];
        d[a] = dl[a] - ma;
        dx[a] = (T)ma;
    }
    if (nominal) {
        T xf[L::NNOM];
#pragma unroll
        for (int e = 0; e < L::NNOM; ++e) xf[e] = xs[e];
        inject<T, N>(xf, dx);                               // x* + mu, q = normalize(q* (x) dq(mu_theta)); g untouched for N = 15
        if (gm.act && gm.mem == 0) {
            T* out = nominal + (size_t)(gm.b / G) * 19;
#pragma unroll
            for (int i = 0; i < 19; ++i) {
                const int e = i < 3 ? L::OFF_P3 + i : i < 6 ? L::OFF_V + (i - 3) : i < 10 ? L::OFF_Q + (i - 6)
                            : i < 13 ? L::OFF_BA + (i - 10) : i < 16 ? L::OFF_BG + (i - 13) : L::OFF_G + (i - 16);
                out[i] = none ? xs[e] : xf[e];
            }
        }
    }

    // ---- step 5: Pbar = sum w_i (P_i + (delta_i - mu)(delta_i - mu)'), element by element through the record ------------------------
    // (each P_i stays in its own member's tangent space: no transport to the chart, as in standard IMM mixing)
    const auto one = [&](auto ac, auto bc, T pe) -> double {
        constexpr int a = decltype(ac)::value, bb = decltype(bc)::value;
        const double v = none ? (double)pe : weff * ((double)pe + d[a] * d[bb]);
        return share ? v : -0.0;
    };
    if constexpr (FULL) {
        if (!P && !pdiag) return;
        for (int r = lane; r < N * N; r += BLOCK) tab[r] = (short)(IO::cov_elem(r) - L::OFF_COV);
        using GB = GroupBatches<T, N>;
        constexpr int NB = GB::NB;
        constexpr int PF = sizeof(T) == 4 ? 4 : 2;          // batches requested ahead of the one being reduced (16 chunks)
        T pb[NB][GROUP_EB];
        static_for<0, PF>([&](auto kc) { GB::template fetch<decltype(kc)::value>(gm, pb); });
        static_for<0, NB>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            GB::template fetch<k + PF>(gm, pb);
            constexpr int q0 = k * GROUP_EB;
            constexpr int ECNT = NP - q0 < GROUP_EB ? NP - q0 : GROUP_EB;
            static_for<0, ECNT>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                term[e * GROUP_TP + lane] = one(std::integral_constant<int, pk_row<N>(q0 + e)>{},
                                                std::integral_constant<int, pk_col<N>(q0 + e)>{}, pb[k][e]);
            });
            group_reduce<ECNT>(term, lane, ngw, G, [&](int g, int e, double acc) { pk[g * PKP + q0 + e] = (T)acc; });
        });
        // the dense rows through LDS, lane-consecutive (unpack_kernel's path); both halves read the same packed element
        if (P) {
            T* out = P + (size_t)gm.g0 * N * N;
            for (int o = lane; o < gm.nvg * N * N; o += BLOCK) {
                const int f = o / (N * N), r = o - f * (N * N);
                out[o] = pk[f * PKP + tab[r]];
            }
        }
        if (pdiag) {
            T* out = pdiag + (size_t)gm.g0 * N;
            for (int o = lane; o < gm.nvg * N; o += BLOCK) {
                const int f = o / N, i = o - f * N;
                out[o] = pk[f * PKP + tab[i * N + i]];
            }
        }
    } else {
        if (!pdiag) return;
        constexpr int NCC = (NP + EPC - 1) / EPC;
        static_for<0, NCC>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            if constexpr (chunk_has_diag<T, N>(c)) {
                T pe[EPC];
                gm.template load<CN + c, CN + c + 1>(pe);
                static_for<0, EPC>([&](auto kc) {
                    constexpr int q = c * EPC + decltype(kc)::value;
                    if constexpr (q < NP && pk_row<N>(q) == pk_col<N>(q)) {
                        constexpr int a = pk_row<N>(q);
                        term[a * GROUP_TP + lane] = one(std::integral_constant<int, a>{}, std::integral_constant<int, a>{}, pe[decltype(kc)::value]);
                    }
                });
            }
        });
        group_reduce<N>(term, lane, ngw, G, [&](int g, int a, double acc) { pk[g * PKP + a] = (T)acc; });
        T* out = pdiag + (size_t)gm.g0 * N;
        for (int o = lane; o < gm.nvg * N; o += BLOCK) {
            const int f = o / N, i = o - f * N;
            out[o] = pk[f * PKP + i];
        }
    }
}

// Every member's whole record <- the record of member src[group], bit for bit; a group whose src is outside 0..G-1 keeps its bytes (the
// value is compared, never used to form an address).  In place: chunk c of the whole wave is in registers before chunk c is stored.
template <typename T, int N>
__global__ void __launch_bounds__(BLOCK)
group_collapse_kernel(T* __restrict__ recs, size_t rec_bytes, int B, int G, const int* __restrict__ src)
{
    using RC = Rec<T, N>;
    const GroupMap<T, N> gm(recs, rec_bytes, B, G);
    const int s = gm.act ? src[gm.b / G] : -1;
    const bool ok = gm.act && s >= 0 && s < G;
    const int from = ok ? gm.gbase + s : gm.lane;           // a lane of this wave either way
    const bool put = ok && gm.mem != s;                     // the source member keeps its bytes
    constexpr int CK = 8;                                   // chunks in flight
#pragma unroll
    for (int c0 = 0; c0 < RC::NCH; c0 += CK) {
        u32x4 v[CK];
#pragma unroll
        for (int k = 0; k < CK; ++k)
            if (c0 + k < RC::NCH) v[k] = __builtin_amdgcn_raw_buffer_load_b128(gm.rs, gm.voff + (unsigned)(c0 + k) * 1024u, 0, AUX_DEFAULT);
#pragma unroll
        for (int k = 0; k < CK; ++k)
            if (c0 + k < RC::NCH) {
                u32x4 o;
                o.x = (unsigned)__shfl((int)v[k].x, from);
                o.y = (unsigned)__shfl((int)v[k].y, from);
                o.z = (unsigned)__shfl((int)v[k].z, from);
                o.w = (unsigned)__shfl((int)v[k].w, from);
                // (the whole offset in the VGPR, soffset 0: see the hazard note at store_chunks)
                if (put) __builtin_amdgcn_raw_buffer_store_b128(o, gm.rs, gm.voff + (unsigned)(c0 + k) * 1024u, 0, AUX_DEFAULT);
            }
    }
}

// dynamic LDS of group_mix_kernel in bytes: a batch of packed covariance elements of every lane, every lane's delta, the 64 weights and
// the mixing weights W[i][lane] = the share of source member i in this lane's filter (G rows: 32 KB of the 50 KB at G = 64)
__host__ __device__ constexpr size_t group_mix_lds(int G)
{
    return (size_t)((GROUP_EB + GROUP_ROWS) * GROUP_TP + 64 + G * 64) * sizeof(double);
}

// IMM mixing in place (fbus_ekf_group_mix, include/fbus_ekf.h): every lane is a source AND a target.  Lane j holds column j of the mixing
// matrix of its group, W_ij = trans[i][j] mu_i / c_j; every lane publishes its delta_i against the chart and, batch by batch, its packed
// covariance elements to LDS, and lane j adds its own G terms from member 0 up.  A source with W_ij == 0 is skipped, not multiplied.
// In place and race-free by collapse's argument: the nominal chunks of the whole wave are in registers (and every delta in LDS) before
// any nominal chunk is stored, a batch of covariance chunks of the whole wave is in LDS before that batch is stored, the batches
// requested ahead are other chunks, and no other wave owns these filters.
template <typename T, int N>
__global__ void __launch_bounds__(BLOCK)
group_mix_kernel(T* __restrict__ recs, size_t rec_bytes, int B, int G, const double* __restrict__ logw, const double* __restrict__ trans,
                 double* __restrict__ weight, double* __restrict__ logc)
{
    using L = Lay<N>;
    using RC = Rec<T, N>;
    constexpr int CN = RC::CH_NOM, EPC = RC::EPC, NP = L::NP;
    extern __shared__ double group_lds[];
    const GroupMap<T, N> gm(recs, rec_bytes, B, G);
    const int lane = gm.lane;
    double* term = group_lds;                               // [GROUP_EB][GROUP_TP]: P_i,e of the batch
    double* dsh = term + GROUP_EB * GROUP_TP;               // [N][GROUP_TP]: delta_i
    double* wsh = dsh + GROUP_ROWS * GROUP_TP;              // [64]
    double* wmix = wsh + 64;                                // [G][64]: W_ij of lane j

    T nom[L::NNOM];
    gm.template load<0, CN>(nom);

    // ---- steps 1, 2: mu as in fuse, c_j and this lane's column of W, in double ----------------------------------------------------------
    int bi;
    const double mu = group_weight(gm, logw, wsh, G, bi);
    const bool none = bi < 0;
    if (gm.act && weight) weight[gm.b] = mu;
    wave_lds_fence();
    wsh[lane] = mu;
    wave_lds_fence();
    double c = 0.0;
    for (int i = 0; i < G; ++i) {
        const double t = trans[i * G + gm.mem] * wsh[gm.gbase + i];
        wmix[i * 64 + lane] = t;
        c += t;
    }
    const bool reach = gm.act && !none && c > 0.0;          // otherwise the target keeps its bytes
    if (gm.act && logc) logc[gm.b] = reach ? log(c) : -__builtin_inf();
    double wjj = 0.0;
    for (int i = 0; i < G; ++i) {
        const double wv = reach ? wmix[i * 64 + lane] / c : 0.0;
        wmix[i * 64 + lane] = wv;
        if (i == gm.mem) wjj = wv;
    }
    const bool put = reach && wjj != 1.0;                   // W_jj == 1: the target is its own only source

    // ---- step 3: the chart x* (carried rotation included) from the best lane, every member's delta to LDS -------------------------------
    const int src = gm.gbase + (none ? 0 : bi);
    T xs[L::NNOM];
#pragma unroll
    for (int e = 0; e < L::NNOM; ++e) xs[e] = __shfl(nom[e], src);
    {
        double dl[N];
        group_delta<T, N>(nom, xs, dl);
#pragma unroll
        for (int a = 0; a < N; ++a) dsh[a * GROUP_TP + lane] = dl[a];
    }
    wave_lds_fence();

    // ---- step 4: m_j = sum_i W_ij delta_i in member order; x* (+) m_j, the chart's rotation (and g for N = 15) kept -----------------------
    double mj[N];
#pragma unroll
    for (int a = 0; a < N; ++a) mj[a] = 0.0;
    for (int i = 0; i < G; ++i) {
        const double wv = wmix[i * 64 + lane];
        if (wv != 0.0) {                                    // step 6: one branch per source -- a weightless source's lanes are masked
#pragma unroll
            for (int a = 0; a < N; ++a) mj[a] += wv * dsh[a * GROUP_TP + gm.gbase + i];
        }
    }
    {
        T dx[N];
#pragma unroll
        for (int a = 0; a < N; ++a) dx[a] = (T)mj[a];
        inject<T, N>(xs, dx);
#pragma unroll
        for (int cc = 0; cc < CN; ++cc) {
            u32x4 v;
            T* e = reinterpret_cast<T*>(&v);
#pragma unroll
            for (int k = 0; k < EPC; ++k) e[k] = xs[cc * EPC + k];
            // (the whole offset in the VGPR, soffset 0: see the hazard note at store_chunks)
            if (put) __builtin_amdgcn_raw_buffer_store_b128(v, gm.rs, gm.voff + (unsigned)cc * 1024u, 0, AUX_DEFAULT);
        }
    }

    // ---- step 5: P0_j = sum_i W_ij (P_i + (delta_i - m_j)(delta_i - m_j)'), a batch of packed elements at a time ------------------------
    using GB = GroupBatches<T, N>;
    constexpr int NB = GB::NB;
    constexpr int PF = 2;                                   // batches requested ahead of the one being mixed
    T pb[NB][GROUP_EB];
    static_for<0, PF>([&](auto kc) { GB::template fetch<decltype(kc)::value>(gm, pb); });
    static_for<0, NB>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        GB::template fetch<k + PF>(gm, pb);
        constexpr int q0 = k * GROUP_EB;
        constexpr int ECNT = NP - q0 < GROUP_EB ? NP - q0 : GROUP_EB;
        constexpr int c0 = GB::c0(k), c1 = GB::c1(k);
#pragma unroll
        for (int e = 0; e < ECNT; ++e) term[e * GROUP_TP + lane] = (double)pb[k][e];
        wave_lds_fence();
        double acc[ECNT];
#pragma unroll
        for (int e = 0; e < ECNT; ++e) acc[e] = 0.0;
        for (int i = 0; i < G; ++i) {
            const double wv = wmix[i * 64 + lane];
            if (wv == 0.0) continue;                        // (one branch per source and batch: a select per element made the compiler
                                                            //  branch around every element's LDS read, each waiting for its own)
            double d[N];                                    // (only the rows and columns of this batch are read)
#pragma unroll
            for (int a = 0; a < N; ++a) d[a] = dsh[a * GROUP_TP + gm.gbase + i] - mj[a];
            static_for<0, ECNT>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                acc[e] += wv * (term[e * GROUP_TP + gm.gbase + i] + d[pk_row<N>(q0 + e)] * d[pk_col<N>(q0 + e)]);
            });
        }
        wave_lds_fence();                                   // (the next batch overwrites term)
        // rounded once to the record type; prev_id and the padding behind the last element keep the lane's own bytes
#pragma unroll
        for (int e = 0; e < ECNT; ++e) pb[k][e] = (T)acc[e];
#pragma unroll
        for (int cc = c0; cc < c1; ++cc) {
            u32x4 v;
            T* e = reinterpret_cast<T*>(&v);
#pragma unroll
            for (int kk = 0; kk < EPC; ++kk) e[kk] = pb[k][(cc - c0) * EPC + kk];
            if (put) __builtin_amdgcn_raw_buffer_store_b128(v, gm.rs, gm.voff + (unsigned)cc * 1024u, 0, AUX_DEFAULT);
        }
    });
}

}  // namespace

namespace fbus {
// grid: one wave per floor(64 / G) whole groups
template <typename T, int N>
void launch_group_fuse_k(hipStream_t s, const T* recs, size_t rec_bytes, int B, int G, const double* logw, double* weight, int* best,
                         T* nominal, T* P, T* pdiag)
{
    const int ngw = 64 / G, grid = (B / G + ngw - 1) / ngw;
    const size_t lds = group_fuse_lds<T, N>(ngw);
    if (P)
        hipLaunchKernelGGL((group_fuse_kernel<T, N, true>), dim3(grid), dim3(BLOCK), lds, s, recs, rec_bytes, B, G, logw, weight, best, nominal,
                           P, pdiag);
    else
        hipLaunchKernelGGL((group_fuse_kernel<T, N, false>), dim3(grid), dim3(BLOCK), lds, s, recs, rec_bytes, B, G, logw, weight, best, nominal,
                           (T*)nullptr, pdiag);
}
template <typename T, int N>
void launch_group_collapse_k(hipStream_t s, T* recs, size_t rec_bytes, int B, int G, const int* src)
{
    const int ngw = 64 / G, grid = (B / G + ngw - 1) / ngw;
    hipLaunchKernelGGL((group_collapse_kernel<T, N>), dim3(grid), dim3(BLOCK), 0, s, recs, rec_bytes, B, G, src);
}
template <typename T, int N>
void launch_group_mix_k(hipStream_t s, T* recs, size_t rec_bytes, int B, int G, const double* logw, const double* trans, double* weight,
                        double* logc)
{
    const int ngw = 64 / G, grid = (B / G + ngw - 1) / ngw;
    hipLaunchKernelGGL((group_mix_kernel<T, N>), dim3(grid), dim3(BLOCK), group_mix_lds(G), s, recs, rec_bytes, B, G, logw, trans, weight, logc);
}
}  // namespace fbus
