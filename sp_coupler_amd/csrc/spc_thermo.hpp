// spc_thermo.hpp -- K12: saturation adjustment of the device-resident LES fields (Qsat, QL and T of every cell from THL, QT
// and the pressure) and the slab means of QL and T in ONE pass, kernel and host side.  spc_hip.hip includes it twice, like
// spc_advance.hpp: with the kernel among the device headers, and -- SPC_THERMO_HOST defined -- after spc_launch.hpp and the
// host side of spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule
// (include/spc.h) per cell, in T, one rounding per operation, never an fma (the build has FP contraction off):
//   Tl = thl * ex[l][k];   Tk = Tl
//   n_iter times:  qs, dqs = th_sat(Tk);   Tk = qt > qs ? Tk - ((Tk - Tl) - c * (qt - qs)) / (T(1) + c * dqs) : Tl
//   qs = th_sat(Tk);   dq = qt - qs;   q = dq > 0 ? dq : (dq != dq ? dq : +0.0);   t = Tl + (rlv * q) / cp
// th_sat is a linear interpolation in a saturation-pressure table the caller hands in: no transcendental function is called,
// so every output has one right answer in T.  3 n_iter + 2 IEEE divisions per cell.
// The means follow K11's scheme (k_slab_means' rule): a lane owns V adjacent k of one LES (spc_chain.hpp), walks the (i, j) rows
// in row-major order and carries the two sums; their bits do not depend on the grid.  The loads do not depend on the arithmetic: the loads of TH_U rows are issued
// before the arithmetic of the TH_U rows before them.  ex, p and eps * p are per (l, k): formed once per lane (eps * p is an
// operand of the rule as it stands, so hoisting it keeps the operation order).
// The table (n_tab entries, 16 KB of doubles at the 2 000 of thermo.py) is read by every lane at data-dependent indices:
// LDS_TAB stages it once per workgroup in LDS; otherwise it is read from global memory (it stays in the caches).
#ifndef SPC_THERMO_HOST

constexpr int TH_THREADS = 256;
constexpr int TH_U = 4;            // rows per batch of a lane (two input streams)

template <typename T> struct LesThermoP {
    const T *thl, *qt, *presf, *ex, *es;
    T *qsat, *ql, *temp, *ql_mean, *t_mean;
    int64_t chains;                // n_les * (ktot / V)
    int64_t pitch_prof, pitch_mean;
    T t_lo, t_hi, inv_step;
    int32_t nij, ktot, n_tab, n_iter;
};

template <typename T> struct ThermoK {
    static constexpr T eps = K<T>::rd / K<T>::rv, om = T(1) - eps, c = K<T>::rlv / K<T>::cp;
};

// qs (and dqs = d qs / d T where DQS) at temperature Tk and pressure p; epsp = eps * p
template <typename T, bool DQS> __device__ __forceinline__ T th_sat(const LesThermoP<T> &P, const T *es, T Tk, T p, T epsp, T &dqs)
{
    const T Tc = Tk < P.t_lo ? P.t_lo : (Tk > P.t_hi ? P.t_hi : Tk);     // NaN passes through
    const T x = (Tc - P.t_lo) * P.inv_step;
    const int m = x >= (T)0 ? min((int)x, P.n_tab - 2) : 0;              // NaN: m = 0, and w below stays NaN
    const T w = x - (T)m;
    const T e0 = es[m];
    const T d = es[m + 1] - e0;
    const T e = e0 + w * d;
    const T den = p - ThermoK<T>::om * e;
    if (DQS) dqs = (epsp * (d * P.inv_step)) / (den * den);
    return (ThermoK<T>::eps * e) / den;
}

// one cell: qs, q and t of the rule
template <typename T> __device__ __forceinline__ void th_cell(const LesThermoP<T> &P, const T *es, T thl, T qt, T ex, T p, T epsp, T &qs, T &q, T &t)
{
    const T Tl = thl * ex;
    T Tk = Tl, dqs;
    for (int it = 0; it < P.n_iter; ++it) {
        const T s = th_sat<T, true>(P, es, Tk, p, epsp, dqs);
        const T step = ((Tk - Tl) - ThermoK<T>::c * (qt - s)) / ((T)1 + ThermoK<T>::c * dqs);
        Tk = qt > s ? Tk - step : Tl;
    }
    qs = th_sat<T, false>(P, es, Tk, p, epsp, dqs);
    const T dq = qt - qs;
    q = dq > (T)0 ? dq : (dq != dq ? dq : (T)0);                         // NaN stays NaN; -0.0 and negatives give +0.0
    t = Tl + (K<T>::rlv * q) / K<T>::cp;
}

// one row of one lane: V cells, their stores and the two sums
template <typename T, int V>
__device__ __forceinline__ void th_row(const LesThermoP<T> &P, const T *es, const SlabVec<T, V> &a, const SlabVec<T, V> &b, const SlabVec<T, V> &ex,
                                       const SlabVec<T, V> &pr, const SlabVec<T, V> &epsp, int64_t off, SlabVec<T, V> &accq, SlabVec<T, V> &acct)
{
    using Vec = SlabVec<T, V>;
    Vec qs, q, t;
#pragma unroll
    for (int v = 0; v < V; ++v) th_cell<T>(P, es, a.v[v], b.v[v], ex.v[v], pr.v[v], epsp.v[v], qs.v[v], q.v[v], t.v[v]);
    *reinterpret_cast<Vec *>(P.qsat + off) = qs;
    *reinterpret_cast<Vec *>(P.ql + off) = q;
    if (P.temp) *reinterpret_cast<Vec *>(P.temp + off) = t;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        accq.v[v] += q.v[v];
        acct.v[v] += t.v[v];
    }
}

// grid ceil(chains / TH_THREADS); dynamic LDS: T table[n_tab] where LDS_TAB
template <typename T, int V, bool LDS_TAB> __global__ __launch_bounds__(TH_THREADS) void k_les_thermo(const LesThermoP<T> P)
{
    extern __shared__ __align__(16) unsigned char th_smem[];
    using Vec = SlabVec<T, V>;
    const T *es = P.es;
    if (LDS_TAB) {
        T *tab = reinterpret_cast<T *>(th_smem);
        for (int i = threadIdx.x; i < P.n_tab; i += TH_THREADS) tab[i] = P.es[i];
        __syncthreads();
        es = tab;
    }
    const int64_t g = (int64_t)blockIdx.x * TH_THREADS + threadIdx.x;
    if (g >= P.chains) return;
    constexpr int U = TH_U;
    const ChainLane<V> lane(g, P.ktot);
    const int64_t ktot = P.ktot;
    const int nij = P.nij;
    int64_t off = lane.cell(nij, ktot);
    const T *thl = P.thl + off, *qt = P.qt + off;
    const Vec ex = *reinterpret_cast<const Vec *>(lane.row(P.ex, P.pitch_prof));
    const Vec pr = *reinterpret_cast<const Vec *>(lane.row(P.presf, P.pitch_prof));
    Vec epsp, accq, acct;
#pragma unroll
    for (int v = 0; v < V; ++v) accq.v[v] = acct.v[v] = (T)0;      // numpy starts a sum from add's identity, +0.0
#pragma unroll
    for (int v = 0; v < V; ++v) epsp.v[v] = ThermoK<T>::eps * pr.v[v];
    Vec a[U], b[U];
    int r = 0;
    if (U <= nij) {
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const Vec *>(thl + u * ktot);
#pragma unroll
        for (int u = 0; u < U; ++u) b[u] = *reinterpret_cast<const Vec *>(qt + u * ktot);
    }
    for (; r + U <= nij; r += U) {
        const bool more = r + 2 * U <= nij;                      // another whole batch follows: its loads go out first
        Vec na[U], nb[U];
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) na[u] = *reinterpret_cast<const Vec *>(thl + (U + u) * ktot);
#pragma unroll
            for (int u = 0; u < U; ++u) nb[u] = *reinterpret_cast<const Vec *>(qt + (U + u) * ktot);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) th_row<T, V>(P, es, a[u], b[u], ex, pr, epsp, off + u * ktot, accq, acct);
        thl += U * ktot;
        qt += U * ktot;
        off += U * ktot;
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a[u] = na[u];
                b[u] = nb[u];
            }
        }
    }
    for (; r < nij; ++r) {
        const Vec a1 = *reinterpret_cast<const Vec *>(thl);
        const Vec b1 = *reinterpret_cast<const Vec *>(qt);
        th_row<T, V>(P, es, a1, b1, ex, pr, epsp, off, accq, acct);
        thl += ktot;
        qt += ktot;
        off += ktot;
    }
    const T cnt = (T)nij;
    if (P.ql_mean) *reinterpret_cast<Vec *>(lane.row(P.ql_mean, P.pitch_mean)) = chain_mean<T, V>(accq, cnt);
    if (P.t_mean) *reinterpret_cast<Vec *>(lane.row(P.t_mean, P.pitch_mean)) = chain_mean<T, V>(acct, cnt);
}

#else  // SPC_THERMO_HOST ----------------------------------------------------------------------------------------------------

constexpr int TH_TAB_LIBRARY = 0, TH_TAB_LDS = 1, TH_TAB_GLOBAL = 2;      // spc_les_thermo_args.table_mode

template <typename T> static int les_thermo_impl(const spc_les_thermo_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_thermo", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    if ((rc = chain_pitch(a->ktot, a->pitch_prof, a->pitch_mean, "%sles_thermo: pitch_prof %lld or pitch_mean %lld smaller than ktot"))) return rc;
    if (a->n_tab < 2) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_thermo: n_tab = %lld < 2", "", (long long)a->n_tab);
    if (a->n_iter < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_thermo: n_iter = %lld < 0", "", (long long)a->n_iter);
    if (a->table_mode < TH_TAB_LIBRARY || a->table_mode > TH_TAB_GLOBAL)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_thermo: table_mode %lld outside 0 ... 2", "", (long long)a->table_mode);
    if (!(a->inv_step > 0)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_thermo: inv_step must be > 0");
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->thl, "thl"); REQUIRE(a->qt, "qt"); REQUIRE(a->presf, "presf"); REQUIRE(a->ex, "ex"); REQUIRE(a->es_tab, "es_tab");
    REQUIRE(a->qsat, "qsat"); REQUIRE(a->ql, "ql");
    const void *in[5] = {a->thl, a->qt, a->presf, a->ex, a->es_tab};
    const void *out[5] = {a->qsat, a->ql, a->temp, a->ql_mean, a->t_mean};
    if ((rc = chain_alias(in, 5, out, 5, "les_thermo: an output is also an input (thl, qt, presf, ex and es_tab are read while it is written)",
                          "les_thermo: two outputs are the same array")))
        return rc;
    uintptr_t bits = (uintptr_t)(a->ktot * sizeof(T)) | (uintptr_t)(a->pitch_prof * sizeof(T)) | (uintptr_t)(a->pitch_mean * sizeof(T));
    for (int i = 0; i < 4; ++i) bits |= (uintptr_t)in[i];                  // (the table is read one element at a time)
    for (int o = 0; o < 5; ++o) bits |= (uintptr_t)out[o];
    LesThermoP<T> p = {};
    bool wide; int64_t grid;
    if ((rc = chain_geometry<T>("les_thermo", bits, (uintptr_t)a->es_tab, a->n_les, a->ktot, TH_THREADS,
                                "les_thermo: ktot == 1 (numpy reduces a one-level plane pairwise; as in les_advance)", wide, p.chains, grid)))
        return rc;
    p.thl = (const T *)a->thl; p.qt = (const T *)a->qt; p.presf = (const T *)a->presf; p.ex = (const T *)a->ex; p.es = (const T *)a->es_tab;
    p.qsat = (T *)a->qsat; p.ql = (T *)a->ql; p.temp = (T *)a->temp; p.ql_mean = (T *)a->ql_mean; p.t_mean = (T *)a->t_mean;
    p.pitch_prof = a->pitch_prof; p.pitch_mean = a->pitch_mean;
    p.t_lo = (T)a->t_lo; p.inv_step = (T)a->inv_step;
    p.t_hi = (T)(a->t_lo + (double)(a->n_tab - 1) / a->inv_step);
    p.nij = a->itot * a->jtot; p.ktot = a->ktot; p.n_tab = a->n_tab; p.n_iter = a->n_iter;
    const size_t tab_bytes = (size_t)a->n_tab * sizeof(T);
    // the library's choice: LDS where the table fits the default limit (measured: DESIGN.md 7.3)
    const bool lds = a->table_mode == TH_TAB_LDS || (a->table_mode == TH_TAB_LIBRARY && tab_bytes <= (size_t)MAX_LDS_BYTES);
    void (*const kern)(const LesThermoP<T>) = lds ? (wide ? k_les_thermo<T, CHAIN_V<T>, true> : k_les_thermo<T, 1, true>)
                                                  : (wide ? k_les_thermo<T, CHAIN_V<T>, false> : k_les_thermo<T, 1, false>);
    if (lds && (rc = ensure_lds(kern, tab_bytes, "les_thermo"))) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(TH_THREADS), lds ? tab_bytes : 0, (hipStream_t)stream, p);
    return launch_status("k_les_thermo");
}

#endif
