// spc_slab.hpp -- K10: horizontal reductions of the LES 3-D fields (slab means, cloud fraction), kernels and host side.
// spc_hip.hip includes it twice: with the kernels among the device headers, and -- SPC_SLAB_HOST defined -- after
// spc_launch.hpp (fail, REQUIRE, ensure_lds, launch_status) for the argument checks and launches.
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous.  One field of one launch may exceed 4 GiB
// (1 024 x 64 x 64 x 160 doubles = 5.4 GB): every element offset below is 64-bit.
//
// k_slab_means      out[f][l][k] = numpy.mean(field_f[l], axis=(0, 1))[k], bit for bit.  NumPy reduces this layout by the plain
//                   sequential accumulation acc[k] = 0; acc[k] += f[i,j,k] over (i, j) in row-major order, in T, then one
//                   division by T(itot * jtot) -- NOT the pairwise sum K6 reproduces for qt[:, :, k].sum() (except where
//                   ktot == 1 makes the plane itself contiguous: k_slab_means_k1).  That order fixes one
//                   dependent add chain of itot * jtot per (l, k); a lane owns V adjacent chains (V = 16 B / sizeof(T) where
//                   ktot and the pointers allow 16-byte accesses, else 1), consecutive lanes consecutive k, so a wave reads a
//                   run of one (l, i, j) row (of the same row of adjacent LES where ktot < 64 V).  The loads of a chain do not
//                   depend on its adds: SLAB_U rows of loads are issued ahead of the adds that consume them.
// k_slab_cloud_*    A[l][r] = (number of (i, j) with any ql[i, j, lo:hi] > 0) / T(itot * jtot) for the GCM layers r of K2's
//                   index map (lo = hi[r-1], hi[r] = clip(idx[r], 0, ktot), hi[-1] = 0; 0 where hi <= lo).  One pass over QL:
//                   a wave reads a row 64 levels at a time, a ballot turns "ql > 0" into a bit mask of the row, and lane r
//                   tests its layers' bit ranges against it.  Counts are integers (exact in any order): they are summed with
//                   integer atomics IN the output rows (a 4-byte word of every T slot), then divided in place.
#ifndef SPC_SLAB_HOST

constexpr int SLAB_MAXF = 16;      // fields per launch (a get_les_profiles round asks for eight)
constexpr int SLAB_THREADS = 256;
constexpr int SLAB_U = 8;          // rows of loads in flight per lane ahead of the add chain

template <typename T> struct SlabMeansP {
    const T *field[SLAB_MAXF];
    T *out[SLAB_MAXF];
    int64_t chains;                // n_les * (ktot / V): lanes per field
    int64_t pitch_out;
    int32_t nij, ktot;
};

template <typename T, int V> __global__ __launch_bounds__(SLAB_THREADS) void k_slab_means(const SlabMeansP<T> p)
{
    const int64_t g = (int64_t)blockIdx.x * SLAB_THREADS + threadIdx.x;
    if (g >= p.chains) return;
    using Vec = SlabVec<T, V>;
    const ChainLane<V> lane(g, p.ktot);
    const int f = blockIdx.y;
    const int64_t ktot = p.ktot;
    const T *src = lane.cell(p.field[f], p.nij, ktot);
    Vec acc;
    chain_zero(acc);
    int r = 0;
    for (; r + SLAB_U <= p.nij; r += SLAB_U) {
        Vec x[SLAB_U];
#pragma unroll
        for (int u = 0; u < SLAB_U; ++u) x[u] = *reinterpret_cast<const Vec *>(src + u * ktot);
        src += SLAB_U * ktot;
#pragma unroll
        for (int u = 0; u < SLAB_U; ++u)
#pragma unroll
            for (int v = 0; v < V; ++v) acc.v[v] += x[u].v[v];
    }
    for (; r < p.nij; ++r) {
        const Vec x = *reinterpret_cast<const Vec *>(src);
        src += ktot;
#pragma unroll
        for (int v = 0; v < V; ++v) acc.v[v] += x.v[v];
    }
    *reinterpret_cast<Vec *>(lane.row(p.out[f], p.pitch_out)) = chain_mean<T, V>(acc, (T)p.nij);
}

// ktot == 1: the field of one LES is ONE contiguous run and numpy reduces it as ndarray.sum() does (pairwise blocks, vn_npsum of
// spc_vnudge.hpp), not sequentially.  A degenerate shape (an LES of one level): one lane per (field, LES).
template <typename T> __global__ __launch_bounds__(SLAB_THREADS) void k_slab_means_k1(const SlabMeansP<T> p)
{
    const int64_t l = (int64_t)blockIdx.x * SLAB_THREADS + threadIdx.x;
    if (l >= p.chains) return;
    const int f = blockIdx.y;
    const T *src = p.field[f] + l * p.nij;
    const T sum = vn_npsum([&](int i) { return src[i]; }, p.nij);
    p.out[f][l * p.pitch_out] = sum / (T)p.nij;
}

// ---- cloud fraction ------------------------------------------------------------------------------------------------------
constexpr int SLAB_CF_WAVES = SLAB_THREADS / 64;
constexpr int SLAB_CF_ROWS = 256;      // (i, j) rows per workgroup: 16 workgroups share a 64 x 64 LES
constexpr int SLAB_CF_RB = 4;          // rows a wave has in flight
constexpr int SLAB_CF_MAXNG = 2048;    // layers: nG counters per wave + the layer bounds in LDS
constexpr int SLAB_CF_MAXK = 1 << 16;  // levels: the bit masks of SLAB_CF_RB rows per wave in LDS

template <typename T> struct SlabCloudP {
    const T *ql;
    const int32_t *idx;
    T *out;
    int64_t pitch_idx, pitch_out;
    int32_t nij, ktot, nG, nwords;     // nwords = ceil(ktot / 64)
};

// the 4-byte word of out[l][r] that holds the count while it is being summed
template <typename T> __device__ __forceinline__ int *slab_count_word(const SlabCloudP<T> &p, int64_t l, int r)
{
    return reinterpret_cast<int *>(p.out + l * p.pitch_out + r);
}

template <typename T> __global__ __launch_bounds__(SLAB_THREADS) void k_slab_cloud_zero(const SlabCloudP<T> p, int64_t total)
{
    const int64_t g = (int64_t)blockIdx.x * SLAB_THREADS + threadIdx.x;
    if (g >= total) return;
    const int64_t l = g / p.nG;
    *slab_count_word(p, l, (int)(g - l * p.nG)) = 0;
}

template <typename T> __global__ __launch_bounds__(SLAB_THREADS) void k_slab_cloud_finish(const SlabCloudP<T> p, int64_t total)
{
    const int64_t g = (int64_t)blockIdx.x * SLAB_THREADS + threadIdx.x;
    if (g >= total) return;
    const int64_t l = g / p.nG;
    const int r = (int)(g - l * p.nG);
    const int c = *slab_count_word(p, l, r);                     // read, then overwritten by this lane alone
    p.out[l * p.pitch_out + r] = (T)c / (T)p.nij;
}

// any bit of the row mask in levels [lo, hi), lo < hi
__device__ __forceinline__ bool slab_any_bit(const unsigned long long *mask, int lo, int hi)
{
    const int w1 = (hi - 1) >> 6;
    for (int w = lo >> 6; w <= w1; ++w) {
        unsigned long long m = mask[w];
        const int b0 = w << 6;
        if (lo > b0) m &= ~0ull << (lo - b0);
        if (hi < b0 + 64) m &= (1ull << (hi - b0)) - 1ull;
        if (m) return true;
    }
    return false;
}

// grid (ceil(nij / SLAB_CF_ROWS), n_les); dynamic LDS: u64 mask[waves][RB][nwords] | int2 bounds[nG] | int cnt[waves][nG]
template <typename T> __global__ __launch_bounds__(SLAB_THREADS) void k_slab_cloud_count(const SlabCloudP<T> p)
{
    extern __shared__ __align__(16) unsigned char slab_smem[];
    const int nG = p.nG, nwords = p.nwords, ktot = p.ktot;
    unsigned long long *masks = reinterpret_cast<unsigned long long *>(slab_smem);
    int2 *bounds = reinterpret_cast<int2 *>(masks + SLAB_CF_WAVES * SLAB_CF_RB * nwords);
    int *cnt = reinterpret_cast<int *>(bounds + nG);
    const int64_t l = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t *idx = p.idx + l * p.pitch_idx;
    for (int r = tid; r < nG; r += SLAB_THREADS) {
        const int hi = min(max(idx[r], 0), ktot);
        const int lo = r > 0 ? min(max(idx[r - 1], 0), ktot) : 0;
        bounds[r] = make_int2(lo, hi);
    }
    for (int i = tid; i < SLAB_CF_WAVES * nG; i += SLAB_THREADS) cnt[i] = 0;
    __syncthreads();
    int *mycnt = cnt + wave * nG;
    unsigned long long *mymask = masks + wave * SLAB_CF_RB * nwords;
    const int row0 = blockIdx.x * SLAB_CF_ROWS;
    const int row1 = min(row0 + SLAB_CF_ROWS, p.nij);
    const T *base = p.ql + l * p.nij * (int64_t)ktot;
    for (int row = row0 + wave * SLAB_CF_RB; row < row1; row += SLAB_CF_WAVES * SLAB_CF_RB) {
        const int nb = min(SLAB_CF_RB, row1 - row);                // wave-uniform
        for (int w = 0; w < nwords; ++w) {
            const int k = (w << 6) + lane;
            T x[SLAB_CF_RB];
#pragma unroll
            for (int b = 0; b < SLAB_CF_RB; ++b)
                x[b] = (b < nb && k < ktot) ? base[(int64_t)(row + b) * ktot + k] : (T)0;
#pragma unroll
            for (int b = 0; b < SLAB_CF_RB; ++b) {
                const unsigned long long m = __ballot(x[b] > (T)0);   // NaN and -0.0 are not cloudy
                if (lane == 0) mymask[b * nwords + w] = m;
            }
        }
        // the masks are written and read by this wave alone: order its LDS accesses, no workgroup barrier needed
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int r = lane; r < nG; r += 64) {
            const int2 b = bounds[r];
            if (b.y <= b.x) continue;
            int c = 0;
            for (int q = 0; q < nb; ++q) c += slab_any_bit(mymask + q * nwords, b.x, b.y) ? 1 : 0;
            mycnt[r] += c;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    for (int r = tid; r < nG; r += SLAB_THREADS) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < SLAB_CF_WAVES; ++w) c += cnt[w * nG + r];
        if (c) atomicAdd(slab_count_word(p, l, r), c);
    }
}

#else  // SPC_SLAB_HOST ------------------------------------------------------------------------------------------------------

static int slab_check_extents(const char *what, int64_t n_les, int32_t itot, int32_t jtot, int32_t ktot)
{
    if (n_les < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%s: n_les = %lld < 0", what, (long long)n_les);
    if (itot < 1 || jtot < 1 || ktot < 1)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%s: itot, jtot and ktot must be >= 1", what);
    if ((int64_t)itot * jtot > INT32_MAX) return fail(SPC_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 points per plane", what);
    return SPC_OK;
}

template <typename T> static int slab_means_impl(const spc_slab_means_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("slab_means", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    static_assert(SPC_SLAB_MAX_FIELDS == SLAB_MAXF, "include/spc.h and spc_slab.hpp disagree on the fields per launch");
    if (a->n_fields < 1 || a->n_fields > SPC_SLAB_MAX_FIELDS)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sslab_means: field count %lld outside 1 ... %lld", "", (long long)a->n_fields, SPC_SLAB_MAX_FIELDS);
    if ((rc = chain_pitch(a->ktot, a->pitch_out, a->ktot, "%sslab_means: pitch_out %lld smaller than ktot %lld"))) return rc;
    if (a->n_les == 0) return SPC_OK;
    SlabMeansP<T> p = {};
    uintptr_t bits = (uintptr_t)(a->ktot * sizeof(T)) | (uintptr_t)(a->pitch_out * sizeof(T));
    for (int f = 0; f < a->n_fields; ++f) {
        REQUIRE(a->fields[f], "fields[f]");
        REQUIRE(a->out[f], "out[f]");
        if ((uintptr_t)a->fields[f] % sizeof(T) || (uintptr_t)a->out[f] % sizeof(T))
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sslab_means: a pointer is not aligned to its element type");
        p.field[f] = (const T *)a->fields[f];
        p.out[f] = (T *)a->out[f];
        bits |= (uintptr_t)a->fields[f] | (uintptr_t)a->out[f];
    }
    bool wide; int64_t grid;                          // (ktot == 1 is this kernel's own: k_slab_means_k1)
    if ((rc = chain_geometry<T>("slab_means", bits, 0, a->n_les, a->ktot, SLAB_THREADS, nullptr, wide, p.chains, grid))) return rc;
    p.nij = a->itot * a->jtot;
    p.ktot = a->ktot;
    p.pitch_out = a->pitch_out;
    void (*const kern)(const SlabMeansP<T>) = a->ktot == 1 ? k_slab_means_k1<T> : (wide ? k_slab_means<T, CHAIN_V<T>> : k_slab_means<T, 1>);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid, (unsigned)a->n_fields), dim3(SLAB_THREADS), 0, (hipStream_t)stream, p);
    return launch_status("k_slab_means");
}

template <typename T> static int slab_cloud_impl(const spc_slab_cloud_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("slab_cloud_fraction", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    if (a->nG < 1) return fail(SPC_ERR_INVALID_ARGUMENT, "%sslab_cloud_fraction: nG = %lld < 1", "", (long long)a->nG);
    if (a->pitch_out < a->nG || a->pitch_idx < a->nG)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sslab_cloud_fraction: pitch_out %lld or pitch_idx %lld smaller than nG", "",
                    (long long)a->pitch_out, (long long)a->pitch_idx);
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->ql, "ql"); REQUIRE(a->idx, "idx"); REQUIRE(a->out, "out");
    if ((uintptr_t)a->ql % sizeof(T) || (uintptr_t)a->out % sizeof(T) || (uintptr_t)a->idx % 4)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sslab_cloud_fraction: a pointer is not aligned to its element type");
    if (a->nG > SLAB_CF_MAXNG || a->ktot > SLAB_CF_MAXK)
        return fail(SPC_ERR_UNSUPPORTED, "%sslab_cloud_fraction: more than %lld layers or %lld levels", "", SLAB_CF_MAXNG, SLAB_CF_MAXK);
    if (a->n_les > 65535) return fail(SPC_ERR_UNSUPPORTED, "%sslab_cloud_fraction: more than 65535 LES per launch");
    SlabCloudP<T> p;
    p.ql = (const T *)a->ql; p.idx = a->idx; p.out = (T *)a->out;
    p.pitch_idx = a->pitch_idx; p.pitch_out = a->pitch_out;
    p.nij = a->itot * a->jtot; p.ktot = a->ktot; p.nG = a->nG; p.nwords = (a->ktot + 63) / 64;
    const int64_t total = a->n_les * (int64_t)a->nG;
    const unsigned egrid = (unsigned)((total + SLAB_THREADS - 1) / SLAB_THREADS);
    const size_t smem = (size_t)SLAB_CF_WAVES * SLAB_CF_RB * p.nwords * 8 + (size_t)p.nG * 8 + (size_t)SLAB_CF_WAVES * p.nG * 4;
    if ((rc = ensure_lds(k_slab_cloud_count<T>, smem, "slab_cloud_fraction"))) return rc;
    hipLaunchKernelGGL(k_slab_cloud_zero<T>, dim3(egrid), dim3(SLAB_THREADS), 0, (hipStream_t)stream, p, total);
    if ((rc = launch_status("k_slab_cloud_zero"))) return rc;
    hipLaunchKernelGGL(k_slab_cloud_count<T>, dim3((unsigned)((p.nij + SLAB_CF_ROWS - 1) / SLAB_CF_ROWS), (unsigned)a->n_les),
                       dim3(SLAB_THREADS), smem, (hipStream_t)stream, p);
    if ((rc = launch_status("k_slab_cloud_count"))) return rc;
    hipLaunchKernelGGL(k_slab_cloud_finish<T>, dim3(egrid), dim3(SLAB_THREADS), 0, (hipStream_t)stream, p, total);
    return launch_status("k_slab_cloud_finish");
}

#endif
