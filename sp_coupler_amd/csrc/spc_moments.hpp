// spc_moments.hpp -- K20: the second moments of the LES 3-D fields per (LES, level): means, variances, standard deviations of a
// set of fields and the covariances of pairs of them, in ONE launch, kernel and host side.  spc_hip.hip includes it twice, like
// spc_qtlocal.hpp: with the kernel among the device headers (after spc_chain.hpp: SlabVec), and -- SPC_MOMENTS_HOST defined --
// after spc_launch.hpp and the host side of spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule (include/spc.h)
// is NumPy's: per (l, k), N = itot * jtot rows r = (i, j) in row-major order, everything in T, one rounding per operation, never
// an fma (the build has FP contraction off):
//   m_f   = (sum over r, sequential from +0.0, of x_f[r]) / T(N)                      K10's rule
//   var_f = (sum over r, sequential from +0.0, of (x_f[r] - m_f) * (x_f[r] - m_f)) / T(N);  std_f = sqrt(var_f)
//   cov_p = (sum over r, sequential from +0.0, of (x_a[r] - m_a) * (x_b[r] - m_b)) / T(N)
// A field given at the upper faces (K17's W) is first brought to the centres: xc[k] = T(0.5) * (x[k - 1] + x[k]), x[-1] := +0.0.
//
// The order binds the ADDS: per (l, k) two dependent chains of N adds, the second behind the first.  Nothing else is bound, and
// the launch is cut so that as many chains as possible run at once:
//   - blockIdx.y is a JOB: one field (its mean, then its sum of squared deviations) or one pair (the means of its two fields,
//     then the sum of the products of their deviations).  A pair forms the means of its fields again instead of waiting for the
//     field jobs: the adds are the same adds, so the bits are the same, and no workgroup waits for another.  At most 8 + 8 jobs.
//   - a lane owns V adjacent levels of one LES in one job, consecutive lanes consecutive k (K10's shape): adjacent LES share a
//     wave where ktot < 64 V.  A lane therefore carries V chains (a pair: 2 V in its first walk); the other chains that hide the
//     latency of an add are those of the other waves of the CU.
//   - U rows of loads are in flight per lane ahead of the adds that consume them (K10's SLAB_U; a pair has U / 2 rows of each of
//     its two fields); every accumulator and every row in flight is a register: no scratch, no LDS.
//   wide    V = 16 B / sizeof(T), U = 8: one 16-byte access per lane and row; taken where every field, every output,
//           ktot * sizeof(T) and pitch_out * sizeof(T) are multiples of 16 bytes
//   narrow  V = 1, U = 32: single elements; every other view and ktot -- and planes of 1 024 rows and more where the wide
//           launch would have fewer than 2 048 waves (16 LES of 64 x 64 x 160: 240 waves wide): there the chain of 4 096 adds
//           and the bytes a wave has in flight bound the launch, V = 1 doubles (f64) or quadruples (f32) the waves and the
//           deeper load-ahead keeps more bytes in flight per lane than the wide form has.  Measured on an MI355X at that size
//           (7 fields, 5 pairs, all outputs): U = 16 1.05 ms (f64) / 0.86 ms (f32), U = 32 0.92 / 0.61 ms; 214 VGPRs (f64), which
//           costs nothing where the launch has two waves per SIMD at most
// The face field needs x[k - 1] beside the lane's vector: one more single-element read per row (the same cache line as the
// vector in all but one lane of 8 or 16), none in the lane at k = 0, which takes +0.0 and never reads in front of the row.
// The second walk reads the rows again, and a pair reads its two fields in both walks beside the field jobs that read them too:
// with the seven fields and five pairs of sp_coupler_amd/statistics.py that is 34 walks of a field for 7 fields, and the fetch
// counter shows 4.0 (256 LES of 8 x 8 x 160) and 4.6 (16 LES of 64 x 64 x 160) reads of the fields reaching the HBM
// (profiles/les_moments_bench.log): the caches catch little of it, the launch is bound by those bytes at the large size.  Tried and
// kept: one job per field or pair (against all fields in one lane, which leaves 20 waves on the card at the large size); half the
// load-ahead per field in a pair job (160 -> 96 VGPRs wide f64, same time).  Staging the rows of the first walk in LDS was
// considered and not built: a lane's rows are N * 16 bytes (64 KiB at 64 x 64), 256 lanes would need 16 MiB.  Not built either:
// a loader / adder split as K6c's, which would let other lanes form the products while one lane per chain adds.
#ifndef SPC_MOMENTS_HOST

constexpr int MOM_THREADS = 256;
constexpr int MOM_MAXF = 8, MOM_MAXP = 8;
constexpr int MOM_MAXJ = MOM_MAXF + MOM_MAXP;
constexpr int MOM_U_WIDE = 8, MOM_U_NARROW = 32;            // rows of loads in flight per lane
constexpr int64_t MOM_MAX_PLANE = (int64_t)1 << 24;         // T(N) is exact in float
constexpr int MOM_LONG_PLANE = 1024;                        // rows from which a launch of few waves goes narrow
constexpr int64_t MOM_FEW_LANES = 2048 * 64;

template <typename T> struct MomJob {
    const T *x[2];                 // the field, x[1] == nullptr; or the two fields of a pair
    T *mean, *var, *std;           // a field's outputs (each may be nullptr); a pair: var is its covariance, the others nullptr
    int32_t face[2];               // x[s] is given at the upper faces
};

template <typename T> struct LesMomentsP {
    MomJob<T> job[MOM_MAXJ];
    int64_t chains;                // n_les * (ktot / V): lanes per job
    int64_t pitch_out;
    int32_t nij, ktot;
};

// one row of one field at the lane's levels: the vector, and the element below it where the field is a face field and k > 0
template <typename T, int V> struct MomRow {
    SlabVec<T, V> x;
    T below;
};

template <typename T, int V> __device__ __forceinline__ MomRow<T, V> mom_load(const T *src, const bool below)
{
    MomRow<T, V> r;
    r.x = *reinterpret_cast<const SlabVec<T, V> *>(src);
    r.below = below ? src[-1] : (T)0;                              // the closed ground: x[-1] := +0.0, never read
    return r;
}

// the row at the cell centres
template <typename T, int V> __device__ __forceinline__ SlabVec<T, V> mom_centre(const MomRow<T, V> &r, const bool face)
{
    if (!face) return r.x;
    SlabVec<T, V> c;
#pragma unroll
    for (int v = 0; v < V; ++v) c.v[v] = (T)0.5 * ((v ? r.x.v[v - 1] : r.below) + r.x.v[v]);   // one add, one multiply
    return c;
}

// the N rows of NS fields in order, U rows of loads ahead of use(c): c[s] is the row of field s at the centres
template <typename T, int V, int U, int NS, typename F>
__device__ __forceinline__ void mom_walk(const T *const (&first)[NS], const bool (&face)[NS], const bool low, const int nij, const int64_t ktot, F &&use)
{
    const T *src[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) src[s] = first[s];
    int r = 0;
    for (; r + U <= nij; r += U) {
        MomRow<T, V> x[NS][U];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int u = 0; u < U; ++u) x[s][u] = mom_load<T, V>(src[s] + u * ktot, face[s] && low);
            src[s] += U * ktot;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            SlabVec<T, V> c[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) c[s] = mom_centre<T, V>(x[s][u], face[s]);
            use(c);
        }
    }
    for (; r < nij; ++r) {
        SlabVec<T, V> c[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            c[s] = mom_centre<T, V>(mom_load<T, V>(src[s], face[s] && low), face[s]);
            src[s] += ktot;
        }
        use(c);
    }
}

template <typename T, int V, int U, int NS>
__device__ __forceinline__ void mom_job(const LesMomentsP<T> &p, const MomJob<T> &j, const ChainLane<V> &lane)
{
    using Vec = SlabVec<T, V>;
    const int64_t ktot = p.ktot;
    const T *first[NS];
    bool face[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        first[s] = lane.cell(j.x[s], p.nij, ktot);
        face[s] = j.face[s] != 0;
    }
    const bool low = lane.k > 0;
    Vec sum[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) chain_zero(sum[s]);
    mom_walk<T, V, U, NS>(first, face, low, p.nij, ktot, [&](const Vec (&c)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int v = 0; v < V; ++v) sum[s].v[v] += c[s].v[v];
    });
    const T cnt = (T)p.nij;
#pragma unroll
    for (int s = 0; s < NS; ++s) chain_mean<T, V>(sum[s], cnt);
    const int64_t o = lane.row(p.pitch_out);
    if (j.mean) *reinterpret_cast<Vec *>(j.mean + o) = sum[0];
    if (!j.var && !j.std) return;
    Vec acc;
    chain_zero(acc);
    mom_walk<T, V, U, NS>(first, face, low, p.nij, ktot, [&](const Vec (&c)[NS]) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const T da = c[0].v[v] - sum[0].v[v];
            const T db = NS == 2 ? c[NS - 1].v[v] - sum[NS - 1].v[v] : da;
            const T q = da * db;                                   // rounded on its own
            acc.v[v] += q;
        }
    });
    chain_mean<T, V>(acc, cnt);
    if (j.var) *reinterpret_cast<Vec *>(j.var + o) = acc;
    if (j.std) {
#pragma unroll
        for (int v = 0; v < V; ++v) acc.v[v] = sqrt(acc.v[v]);     // correctly rounded
        *reinterpret_cast<Vec *>(j.std + o) = acc;
    }
}

// grid (ceil(chains / MOM_THREADS), jobs)
template <typename T, int V> __global__ __launch_bounds__(MOM_THREADS) void k_les_moments(const LesMomentsP<T> p)
{
    constexpr int U = V == 1 ? MOM_U_NARROW : MOM_U_WIDE;
    const int64_t g = (int64_t)blockIdx.x * MOM_THREADS + threadIdx.x;
    if (g >= p.chains) return;
    const ChainLane<V> lane(g, p.ktot);
    const MomJob<T> &j = p.job[blockIdx.y];
    if (j.x[1])
        mom_job<T, V, U / 2, 2>(p, j, lane);                 // a pair: the same bytes in flight, over two fields
    else
        mom_job<T, V, U, 1>(p, j, lane);
}

#else  // SPC_MOMENTS_HOST ---------------------------------------------------------------------------------------------------

template <typename T> static int les_moments_impl(const spc_les_moments_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    static_assert(SPC_MOMENTS_MAX_FIELDS == MOM_MAXF && SPC_MOMENTS_MAX_PAIRS == MOM_MAXP, "include/spc.h and spc_moments.hpp disagree");
    if (a->itot >= 1 && a->jtot >= 1 && (int64_t)a->itot * a->jtot > MOM_MAX_PLANE)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_moments: more than 2^24 points per plane (their number is not exact in float)");
    int rc = slab_check_extents("les_moments", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    if (a->ktot == 1)
        return fail(SPC_ERR_UNSUPPORTED, "%sles_moments: ktot == 1 (numpy reduces a plane of one level pairwise, not in this order)");
    if (a->n_fields < 1 || a->n_fields > MOM_MAXF)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_moments: field count %lld outside 1 ... %lld", "", (long long)a->n_fields, (long long)MOM_MAXF);
    if (a->n_pairs < 0 || a->n_pairs > MOM_MAXP)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_moments: pair count %lld outside 0 ... %lld", "", (long long)a->n_pairs, (long long)MOM_MAXP);
    if (a->face_field < -1 || a->face_field >= a->n_fields)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_moments: face_field %lld is neither -1 nor a field index", "", (long long)a->face_field);
    if ((rc = chain_pitch(a->ktot, a->pitch_out, a->pitch_out, "%sles_moments: pitch_out %lld smaller than ktot"))) return rc;
    for (int q = 0; q < a->n_pairs; ++q)
        if (a->pair_a[q] < 0 || a->pair_a[q] >= a->n_fields || a->pair_b[q] < 0 || a->pair_b[q] >= a->n_fields || a->pair_a[q] == a->pair_b[q])
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_moments: pair %lld is not two different field indices", "", (long long)q);
    // every output asked for: none may START at the same address as a field or as another of them
    const void *out[MOM_MAXF * 3 + MOM_MAXP];
    int n_out = 0;
    uintptr_t bits = (uintptr_t)((size_t)a->ktot * sizeof(T)) | (uintptr_t)((size_t)a->pitch_out * sizeof(T));
    for (int f = 0; f < a->n_fields; ++f)
        for (void *const o : {a->mean[f], a->var[f], a->std[f]})
            if (o) out[n_out++] = o;
    for (int q = 0; q < a->n_pairs; ++q)
        if (a->cov[q]) out[n_out++] = a->cov[q];
    if (a->n_les == 0) return SPC_OK;
    if (!n_out) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_moments: no output asked for");
    for (int f = 0; f < a->n_fields; ++f) REQUIRE(a->fields[f], "fields[f]");
    const char *const same = "les_moments: an output is the same array as a field or as another output";
    if ((rc = chain_alias(a->fields, a->n_fields, out, n_out, same, same))) return rc;
    for (int f = 0; f < a->n_fields; ++f) bits |= (uintptr_t)a->fields[f];
    for (int o = 0; o < n_out; ++o) bits |= (uintptr_t)out[o];
    LesMomentsP<T> p = {};
    int jobs = 0;
    for (int f = 0; f < a->n_fields; ++f)
        if (a->mean[f] || a->var[f] || a->std[f]) {
            MomJob<T> &j = p.job[jobs++];
            j.x[0] = (const T *)a->fields[f];
            j.face[0] = f == a->face_field;
            j.mean = (T *)a->mean[f]; j.var = (T *)a->var[f]; j.std = (T *)a->std[f];
        }
    for (int q = 0; q < a->n_pairs; ++q)
        if (a->cov[q]) {
            MomJob<T> &j = p.job[jobs++];
            j.x[0] = (const T *)a->fields[a->pair_a[q]];
            j.x[1] = (const T *)a->fields[a->pair_b[q]];
            j.face[0] = a->pair_a[q] == a->face_field;
            j.face[1] = a->pair_b[q] == a->face_field;
            j.var = (T *)a->cov[q];
        }
    p.nij = a->itot * a->jtot;
    p.ktot = a->ktot;
    p.pitch_out = a->pitch_out;
    // a long plane in a launch of few waves goes narrow (above); (ktot == 1 was refused before the fields were looked at)
    const bool narrow = p.nij >= MOM_LONG_PLANE && a->n_les * (int64_t)(a->ktot / CHAIN_V<T>) * jobs < MOM_FEW_LANES;
    bool wide; int64_t grid;
    if ((rc = chain_geometry<T>("les_moments", bits, 0, a->n_les, a->ktot, MOM_THREADS, nullptr, wide, p.chains, grid, narrow))) return rc;
    void (*const kern)(const LesMomentsP<T>) = wide ? k_les_moments<T, CHAIN_V<T>> : k_les_moments<T, 1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid, (unsigned)jobs), dim3(MOM_THREADS), 0, (hipStream_t)stream, p);
    return launch_status("k_les_moments");
}

#endif
