// spc_micro.hpp -- K14: warm-rain microphysics of the device-resident LES fields (cloud water -> rain, one upwind step of
// sedimentation, the surface rain, the cloud ice) and the slab means of what it changes in ONE pass, kernel and host side.
// spc_hip.hip includes it twice, like spc_advance.hpp: with the kernel among the device headers, and -- SPC_MICRO_HOST
// defined -- after spc_launch.hpp and the host side of spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule
// (include/spc.h) per cell, in T, one rounding per operation, never an fma (the build has FP contraction off):
//   qr_up = k + 1 < ktot ? qr[k + 1] : +0.0                       the OLD qr: qr_new is a separate buffer
//   out = so[l][k] * qr;   qs = (qr - out) + si[l][k] * qr_up
//   d = ql - qc0;   x = d > 0 ? d : (d != d ? d : +0.0)
//   s = ka * x + (kc * ql) * qs;   s = s > ql ? ql : s
//   qt -= s;   thl += lcpex[l][k] * s;   qr_new = qs + s;   rain[l][i][j] += (so[l][0] * qr[k = 0]) * w[l][0]
//   fi = temp >= tu ? 0 : (temp <= td ? 1 : (tu - temp) / den);   qi = (ql - s) * fi
//   means of the new qt, the new thl, qr_new and qi by k_slab_means' rule
// K11's shape: a lane owns V adjacent k of one LES (spc_chain.hpp) and walks the itot * jtot rows in row-major order: the
// sequential slab sums fix that chain.  ONE lane carries all four sums, since they hang on the same s.  qr_up is the lane's
// own next element for v < V - 1; for its last element it is one extra load of qr[k + V] (nothing for the lane at the top).
// The lane at k == 0 also carries rain: it loads and stores rain[l][r] with row r.  A lane stores only the elements of qt, thl
// and rain it loaded itself, and qr is never written, so the in-place update needs no ordering beyond program order.
// Loads do not depend on the arithmetic: a lane holds TWO batches of U rows -- the loads of batch b + 1 are issued before
// the arithmetic and stores of batch b.  Five 16-byte streams and two scalars per row against the two of K11's QT lanes:
// the 16-byte forms take 256 VGPRs and about 120 AGPRs with U = 4 rows per batch (320 bytes of loads per lane in flight; K11:
// 8 rows, 4 for its QT lanes, 128 bytes), one wave per SIMD, and 214 VGPRs with U = 2, two waves per SIMD; no scratch and no
// spill in either (DESIGN.md 7.3 has the counts).  A workgroup is ONE wave, so that the waves of a launch spread over all CUs,
// and the launch has n_les * ktot / V / 64 of them: 320 at 256 LES of 160 doubles, fewer than the chip has SIMDs.  The host
// side picks U by that count: MIC_U_FEW = 4 where every wave has a SIMD to itself (the registers of a wave then limit
// nothing, and the longer batch hides more of the latency of the serial walk), MIC_U_MANY = 2 above it (a second wave per
// SIMD is worth more than the longer batch: measured).  The bits do not depend on U.
#ifndef SPC_MICRO_HOST

constexpr int MIC_THREADS = 64;
constexpr int MIC_U_FEW = 4;       // rows per batch of a lane where the launch has at most one wave per SIMD
constexpr int MIC_U_MANY = 2;      // ... and above that

template <typename T> struct LesMicroP {
    T *qt, *thl, *qr_new, *rain;
    const T *ql, *qr, *temp;
    const T *sed_out, *sed_in, *lcpex, *w;
    T *qt_mean, *thl_mean, *qr_mean, *qi_mean;
    int64_t chains;                // n_les * (ktot / V)
    int64_t pitch_prof, pitch_mean;
    T qc0, ka, kc, tu, td, den;
    int32_t nij, ktot;
};

// what a lane loads of one row
template <typename T, int V> struct MicRow {
    SlabVec<T, V> qt, ql, qr, thl, temp;
    T up, rn;                      // qr[k + V] (+0.0 for the lane at the top); rain[l][r] (the lane at k == 0)
};

// the loads of the row at element offset o; top: the lane holds level ktot - 1; rain: &rain[l][r] for the lane at k == 0, else NULL
template <typename T, int V> __device__ __forceinline__ void mic_load(MicRow<T, V> &x, const LesMicroP<T> &P, int64_t o, bool top, const T *rain)
{
    using Vec = SlabVec<T, V>;
    x.qt = *reinterpret_cast<const Vec *>(P.qt + o);
    x.ql = *reinterpret_cast<const Vec *>(P.ql + o);
    x.qr = *reinterpret_cast<const Vec *>(P.qr + o);
    x.thl = x.qt;
    x.temp = x.ql;
    if (P.thl) x.thl = *reinterpret_cast<const Vec *>(P.thl + o);
    if (P.temp) x.temp = *reinterpret_cast<const Vec *>(P.temp + o);
    x.up = top ? (T)0 : P.qr[o + V];
    x.rn = rain ? *rain : (T)0;
}

template <typename T, int V> struct MicProf {
    SlabVec<T, V> so, si, lc;
    T w0;
};

// one row of one lane: V cells, their stores and the four sums
template <typename T, int V>
__device__ __forceinline__ void mic_row(const LesMicroP<T> &P, const MicRow<T, V> &x, const MicProf<T, V> &f, int64_t o, T *rain,
                                        SlabVec<T, V> &aqt, SlabVec<T, V> &athl, SlabVec<T, V> &aqr, SlabVec<T, V> &aqi)
{
    using Vec = SlabVec<T, V>;
    Vec nqt, nthl, nqr, qi;
    T out0 = (T)0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const T qr = x.qr.v[v], ql = x.ql.v[v];
        const T qu = v + 1 < V ? x.qr.v[v + 1 < V ? v + 1 : v] : x.up;
        const T out = f.so.v[v] * qr;
        const T qs = (qr - out) + f.si.v[v] * qu;
        const T d = ql - P.qc0;
        const T xx = d > (T)0 ? d : (d != d ? d : (T)0);          // NaN stays NaN; -0.0 and negatives give +0.0
        T s = P.ka * xx + (P.kc * ql) * qs;
        s = s > ql ? ql : s;                                        // NaN stays NaN
        nqt.v[v] = x.qt.v[v] - s;
        nthl.v[v] = x.thl.v[v] + f.lc.v[v] * s;
        nqr.v[v] = qs + s;
        const T t = x.temp.v[v];
        const T fi = t >= P.tu ? (T)0 : (t <= P.td ? (T)1 : (P.tu - t) / P.den);      // IEEE division (the build has no fast-math)
        qi.v[v] = (ql - s) * fi;
        if (v == 0) out0 = out;
    }
    *reinterpret_cast<Vec *>(P.qt + o) = nqt;
    if (P.thl) *reinterpret_cast<Vec *>(P.thl + o) = nthl;
    *reinterpret_cast<Vec *>(P.qr_new + o) = nqr;
    if (rain) *rain = x.rn + out0 * f.w0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        aqt.v[v] += nqt.v[v];
        athl.v[v] += nthl.v[v];
        aqr.v[v] += nqr.v[v];
        aqi.v[v] += qi.v[v];
    }
}

// grid ceil(chains / MIC_THREADS)
template <typename T, int V, int U> __global__ __launch_bounds__(MIC_THREADS) void k_les_microphysics(const LesMicroP<T> P)
{
    using Vec = SlabVec<T, V>;
    using Row = MicRow<T, V>;
    const int64_t g = (int64_t)blockIdx.x * MIC_THREADS + threadIdx.x;
    if (g >= P.chains) return;
    const ChainLane<V> lane(g, P.ktot);
    const int64_t ktot = P.ktot;
    const int nij = P.nij;
    const bool top = lane.k + V >= P.ktot;
    int64_t off = lane.cell(nij, ktot);
    T *rain = lane.k == 0 && P.rain ? P.rain + lane.l * nij : nullptr;
    MicProf<T, V> f;
    f.so = *reinterpret_cast<const Vec *>(lane.row(P.sed_out, P.pitch_prof));
    f.si = *reinterpret_cast<const Vec *>(lane.row(P.sed_in, P.pitch_prof));
    f.lc = f.so;
    if (P.thl) f.lc = *reinterpret_cast<const Vec *>(lane.row(P.lcpex, P.pitch_prof));
    f.w0 = rain ? P.w[lane.l * P.pitch_prof] : (T)0;
    Vec aqt, athl, aqr, aqi;
#pragma unroll
    for (int v = 0; v < V; ++v) aqt.v[v] = athl.v[v] = aqr.v[v] = aqi.v[v] = (T)0;      // numpy starts a sum from add's identity, +0.0
    Row x[U];
    int r = 0;
    if (U <= nij) {
#pragma unroll
        for (int u = 0; u < U; ++u) mic_load<T, V>(x[u], P, off + u * ktot, top, rain ? rain + u : nullptr);
    }
    for (; r + U <= nij; r += U) {
        const bool more = r + 2 * U <= nij;                      // another whole batch follows: its loads go out first
        Row nx[U];
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) mic_load<T, V>(nx[u], P, off + (U + u) * ktot, top, rain ? rain + U + u : nullptr);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) mic_row<T, V>(P, x[u], f, off + u * ktot, rain ? rain + u : nullptr, aqt, athl, aqr, aqi);
        off += U * ktot;
        if (rain) rain += U;
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = nx[u];
        }
    }
    for (; r < nij; ++r) {
        Row x1;
        mic_load<T, V>(x1, P, off, top, rain);
        mic_row<T, V>(P, x1, f, off, rain, aqt, athl, aqr, aqi);
        off += ktot;
        if (rain) ++rain;
    }
    const T cnt = (T)nij;
    const int64_t m = lane.row(P.pitch_mean);
    if (P.qt_mean) *reinterpret_cast<Vec *>(P.qt_mean + m) = chain_mean<T, V>(aqt, cnt);
    if (P.thl_mean) *reinterpret_cast<Vec *>(P.thl_mean + m) = chain_mean<T, V>(athl, cnt);
    if (P.qr_mean) *reinterpret_cast<Vec *>(P.qr_mean + m) = chain_mean<T, V>(aqr, cnt);
    if (P.qi_mean) *reinterpret_cast<Vec *>(P.qi_mean + m) = chain_mean<T, V>(aqi, cnt);
}

#else  // SPC_MICRO_HOST -----------------------------------------------------------------------------------------------------

template <typename T> static int les_micro_impl(const spc_les_micro_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_microphysics", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    if ((rc = chain_pitch(a->ktot, a->pitch_prof, a->pitch_mean, "%sles_microphysics: pitch_prof %lld or pitch_mean %lld smaller than ktot"))) return rc;
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->qt, "qt"); REQUIRE(a->ql, "ql"); REQUIRE(a->qr, "qr"); REQUIRE(a->qr_new, "qr_new");
    REQUIRE(a->sed_out, "sed_out"); REQUIRE(a->sed_in, "sed_in");
    REQUIRE(!a->thl || a->lcpex, "lcpex (thl is given)");
    REQUIRE(!a->rain || a->w, "w (rain is given)");
    if (a->thl_mean && !a->thl) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_microphysics: thl_mean without thl");
    if (a->qi_mean && !a->temp) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_microphysics: qi_mean without temp (the cloud ice needs the temperature)");
    // (equal base pointers are what is detected, as in K11: partially overlapping views are the caller's to avoid)
    const void *in[7] = {a->ql, a->qr, a->temp, a->sed_out, a->sed_in, a->thl ? a->lcpex : nullptr, a->rain ? a->w : nullptr};
    const void *out[8] = {a->qr_new, a->qt, a->thl, a->rain, a->qt_mean, a->thl_mean, a->qr_mean, a->qi_mean};
    if ((rc = chain_alias(in, 7, out, 8, "les_microphysics: a written array is also an input (qr_new must not be qr: the level below reads the old qr)",
                          "les_microphysics: two written arrays are the same array")))
        return rc;
    uintptr_t bits = (uintptr_t)(a->ktot * sizeof(T)) | (uintptr_t)(a->pitch_prof * sizeof(T)) | (uintptr_t)(a->pitch_mean * sizeof(T));
    for (int i = 0; i < 6; ++i) bits |= (uintptr_t)in[i];                  // (w and rain are read and written one element at a time)
    for (int o = 0; o < 8; ++o)
        if (o != 3) bits |= (uintptr_t)out[o];
    LesMicroP<T> p = {};
    bool wide; int64_t grid;
    if ((rc = chain_geometry<T>("les_microphysics", bits, (uintptr_t)a->w | (uintptr_t)a->rain, a->n_les, a->ktot, MIC_THREADS,
                                "les_microphysics: ktot == 1 (numpy reduces a one-level plane pairwise; as in les_advance)", wide, p.chains, grid)))
        return rc;
    p.qt = (T *)a->qt; p.thl = (T *)a->thl; p.qr_new = (T *)a->qr_new; p.rain = (T *)a->rain;
    p.ql = (const T *)a->ql; p.qr = (const T *)a->qr; p.temp = (const T *)a->temp;
    p.sed_out = (const T *)a->sed_out; p.sed_in = (const T *)a->sed_in; p.lcpex = (const T *)a->lcpex; p.w = (const T *)a->w;
    p.qt_mean = (T *)a->qt_mean; p.thl_mean = (T *)a->thl_mean; p.qr_mean = (T *)a->qr_mean; p.qi_mean = (T *)a->qi_mean;
    p.pitch_prof = a->pitch_prof; p.pitch_mean = a->pitch_mean;
    p.qc0 = (T)a->qc0;
    p.ka = (T)((T)a->k_auto * (T)a->dt);
    p.kc = (T)((T)a->k_acc * (T)a->dt);
    p.tu = (T)a->t_up; p.td = (T)a->t_dn;
    p.den = p.tu - p.td;
    p.nij = a->itot * a->jtot; p.ktot = a->ktot;
    const bool few = grid <= (int64_t)device_cus() * 4;   // a workgroup is one wave: at most one wave per SIMD
    void (*const kern)(const LesMicroP<T>) = few ? (wide ? k_les_microphysics<T, CHAIN_V<T>, MIC_U_FEW> : k_les_microphysics<T, 1, MIC_U_FEW>)
                                                 : (wide ? k_les_microphysics<T, CHAIN_V<T>, MIC_U_MANY> : k_les_microphysics<T, 1, MIC_U_MANY>);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(MIC_THREADS), 0, (hipStream_t)stream, p);
    return launch_status("k_les_microphysics");
}

#endif
