// spc_advance.hpp -- K11: one step of the device-resident LES fields and the slab means of the stepped fields in ONE pass,
// kernel and host side.  spc_hip.hip includes it twice, like spc_slab.hpp: with the kernel among the device headers, and --
// SPC_ADVANCE_HOST defined -- after spc_launch.hpp and the host side of spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule
// (include/spc.h), per field f of the launch, LES l, level k:
//   inc      = tend[f][l][k] * (T)dt                    one rounding in T (where tend[f] != NULL; else the field keeps its bits)
//   field    = field + inc                              one rounding, IN PLACE, no fma (the build has FP contraction off)
//   q        = d > 0 ? d : (d != d ? d : +0.0),  d = field[sat_field] - qsat      (AFTER sat_field's update; -> ql)
//   mean[f]  = numpy.mean(new field[l], axis=(0, 1))[k]  k_slab_means' rule: acc = +0; acc += x over (i, j) in row-major
//              order in T; one IEEE division by T(itot * jtot).  ql_mean likewise, of q.
// The sequential sum fixes one dependent add chain of itot * jtot per (f, l, k), as in K10; the chains of different fields are
// independent: blockIdx.y is the field, a lane owns V adjacent k of one (f, l) (spc_chain.hpp).  The lanes of sat_field carry the
// QT chain AND the q chain: two input streams (QT, qsat), two output streams (QT, ql), two sums.  A lane stores only the
// elements it loaded itself, so the in-place update needs no ordering beyond program order.
// Loads do not depend on the adds: a lane holds TWO batches of rows -- the loads of batch b + 1 are issued before the adds
// and stores of batch b -- of ADV_U rows each (ADV_US for the lanes of sat_field, which load two streams).
#ifndef SPC_ADVANCE_HOST

constexpr int ADV_MAXF = 8;        // fields per launch (SPC_ADVANCE_MAX_FIELDS)
constexpr int ADV_THREADS = 256;
constexpr int ADV_U = 8;           // rows per batch of a lane with one input stream
constexpr int ADV_US = 4;          // rows per batch of a lane of sat_field (two input streams)

template <typename T> struct LesAdvanceP {
    T *field[ADV_MAXF];
    const T *tend[ADV_MAXF];
    T *mean[ADV_MAXF];
    const T *qsat;
    T *ql, *ql_mean;
    int64_t chains;                // n_les * (ktot / V): lanes per field
    int64_t pitch_tend, pitch_mean;
    T dt;
    int32_t nij, ktot, sat_field;
};

// one row of one lane: update, store, sum; for the lanes of sat_field the same for q
template <typename T, int V, bool SAT>
__device__ __forceinline__ void adv_row(SlabVec<T, V> x, const SlabVec<T, V> &s, const SlabVec<T, V> &inc, bool upd, T *dst, T *ql,
                                        SlabVec<T, V> &acc, SlabVec<T, V> &accq)
{
    using Vec = SlabVec<T, V>;
    if (upd) {
#pragma unroll
        for (int v = 0; v < V; ++v) x.v[v] = x.v[v] + inc.v[v];
        *reinterpret_cast<Vec *>(dst) = x;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) acc.v[v] += x.v[v];
    if (SAT) {
        Vec q;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const T d = x.v[v] - s.v[v];
            q.v[v] = d > (T)0 ? d : (d != d ? d : (T)0);         // NaN stays NaN; -0.0 and negatives give +0.0
        }
        if (ql) *reinterpret_cast<Vec *>(ql) = q;
#pragma unroll
        for (int v = 0; v < V; ++v) accq.v[v] += q.v[v];
    }
}

template <typename T, int V, bool SAT> __device__ __forceinline__ void adv_chain(const LesAdvanceP<T> &p, int f, const ChainLane<V> &lane)
{
    using Vec = SlabVec<T, V>;
    constexpr int U = SAT ? ADV_US : ADV_U;
    const int64_t ktot = p.ktot;
    const int nij = p.nij;
    const bool upd = p.tend[f] != nullptr;
    const int64_t off = lane.cell(nij, ktot);
    T *dst = p.field[f] + off;
    const T *qs = SAT ? p.qsat + off : nullptr;
    T *ql = SAT && p.ql ? p.ql + off : nullptr;
    Vec inc, acc, accq;
#pragma unroll
    for (int v = 0; v < V; ++v) inc.v[v] = acc.v[v] = accq.v[v] = (T)0;      // numpy starts a sum from add's identity, +0.0
    if (upd) {
        const Vec t = *reinterpret_cast<const Vec *>(lane.row(p.tend[f], p.pitch_tend));
#pragma unroll
        for (int v = 0; v < V; ++v) inc.v[v] = t.v[v] * p.dt;
    }
    Vec x[U], s[U];
    int r = 0;
    if (U <= nij) {
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = *reinterpret_cast<const Vec *>(dst + u * ktot);
        if (SAT) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = *reinterpret_cast<const Vec *>(qs + u * ktot);
        }
    }
    for (; r + U <= nij; r += U) {
        const bool more = r + 2 * U <= nij;                      // another whole batch follows: its loads go out first
        Vec nx[U], ns[U];
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) nx[u] = *reinterpret_cast<const Vec *>(dst + (U + u) * ktot);
            if (SAT) {
#pragma unroll
                for (int u = 0; u < U; ++u) ns[u] = *reinterpret_cast<const Vec *>(qs + (U + u) * ktot);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) adv_row<T, V, SAT>(x[u], s[u], inc, upd, dst + u * ktot, ql ? ql + u * ktot : nullptr, acc, accq);
        dst += U * ktot;
        if (SAT) qs += U * ktot;
        if (ql) ql += U * ktot;
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                x[u] = nx[u];
                if (SAT) s[u] = ns[u];
            }
        }
    }
    for (; r < nij; ++r) {
        const Vec x1 = *reinterpret_cast<const Vec *>(dst);
        Vec s1 = x1;
        if (SAT) s1 = *reinterpret_cast<const Vec *>(qs);
        adv_row<T, V, SAT>(x1, s1, inc, upd, dst, ql, acc, accq);
        dst += ktot;
        if (SAT) qs += ktot;
        if (ql) ql += ktot;
    }
    const T cnt = (T)nij;
    if (p.mean[f]) *reinterpret_cast<Vec *>(lane.row(p.mean[f], p.pitch_mean)) = chain_mean<T, V>(acc, cnt);
    if (SAT && p.ql_mean) *reinterpret_cast<Vec *>(lane.row(p.ql_mean, p.pitch_mean)) = chain_mean<T, V>(accq, cnt);
}

// grid (ceil(chains / ADV_THREADS), n_fields)
template <typename T, int V> __global__ __launch_bounds__(ADV_THREADS) void k_les_advance(const LesAdvanceP<T> p)
{
    const int64_t g = (int64_t)blockIdx.x * ADV_THREADS + threadIdx.x;
    if (g >= p.chains) return;
    const int f = blockIdx.y;
    const ChainLane<V> lane(g, p.ktot);
    if (f == p.sat_field)
        adv_chain<T, V, true>(p, f, lane);
    else if (p.tend[f] || p.mean[f])                             // else: nothing of this field is asked for
        adv_chain<T, V, false>(p, f, lane);
}

#else  // SPC_ADVANCE_HOST ---------------------------------------------------------------------------------------------------

template <typename T> static int les_advance_impl(const spc_les_advance_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_advance", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    static_assert(SPC_ADVANCE_MAX_FIELDS == ADV_MAXF, "include/spc.h and spc_advance.hpp disagree on the fields per launch");
    if (a->n_fields < 1 || a->n_fields > SPC_ADVANCE_MAX_FIELDS)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advance: field count %lld outside 1 ... %lld", "", (long long)a->n_fields, SPC_ADVANCE_MAX_FIELDS);
    if ((rc = chain_pitch(a->ktot, a->pitch_tend, a->pitch_mean, "%sles_advance: pitch_tend %lld or pitch_mean %lld smaller than ktot"))) return rc;
    if (a->sat_field < -1 || a->sat_field >= a->n_fields)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advance: sat_field %lld outside -1 ... %lld", "", (long long)a->sat_field, (long long)a->n_fields - 1);
    if (a->n_les == 0) return SPC_OK;
    const bool sat = a->sat_field >= 0;
    if (sat) REQUIRE(a->qsat, "qsat");
    LesAdvanceP<T> p = {};
    uintptr_t bits = (uintptr_t)(a->ktot * sizeof(T)) | (uintptr_t)(a->pitch_tend * sizeof(T)) | (uintptr_t)(a->pitch_mean * sizeof(T));
    if (sat) {
        p.qsat = (const T *)a->qsat; p.ql = (T *)a->ql; p.ql_mean = (T *)a->ql_mean;
        bits |= (uintptr_t)a->qsat | (uintptr_t)a->ql | (uintptr_t)a->ql_mean;
    }
    for (int f = 0; f < a->n_fields; ++f) {
        REQUIRE(a->fields[f], "fields[f]");
        if (sat && a->ql && (a->ql == a->fields[f] || a->ql == a->qsat))
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advance: ql is also a field or qsat (it is written while they are read)");
        if (sat && a->qsat == a->fields[f])
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advance: qsat is also a field (it is read while they are updated)");
        for (int g = 0; g < f; ++g)
            if (a->fields[g] == a->fields[f])
                return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advance: fields[%lld] and fields[%lld] are the same field", "", g, f);
        p.field[f] = (T *)a->fields[f];
        p.tend[f] = (const T *)a->tend[f];
        p.mean[f] = (T *)a->mean[f];
        bits |= (uintptr_t)a->fields[f] | (uintptr_t)a->tend[f] | (uintptr_t)a->mean[f];
    }
    bool wide; int64_t grid;
    if ((rc = chain_geometry<T>("les_advance", bits, 0, a->n_les, a->ktot, ADV_THREADS,
                                "les_advance: ktot == 1 (numpy reduces a one-level plane pairwise: step the field and call slab_means)", wide, p.chains, grid)))
        return rc;
    p.nij = a->itot * a->jtot;
    p.ktot = a->ktot;
    p.sat_field = a->sat_field;
    p.pitch_tend = a->pitch_tend;
    p.pitch_mean = a->pitch_mean;
    p.dt = (T)a->dt;
    void (*const kern)(const LesAdvanceP<T>) = wide ? k_les_advance<T, CHAIN_V<T>> : k_les_advance<T, 1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid, (unsigned)a->n_fields), dim3(ADV_THREADS), 0, (hipStream_t)stream, p);
    return launch_status("k_les_advance");
}

#endif
