// spc_radiate.hpp -- K18: the longwave cooling and warming that the liquid water of a column gives its own air (the first two
// terms of the GCSS / DYCOMS-II parametrised flux, Stevens et al. 2005), kernel and host side.  spc_hip.hip includes it twice,
// like spc_diffuse.hpp and spc_vadvect.hpp: with the kernel among the device headers, and -- SPC_RADIATE_HOST defined -- after
// spc_launch.hpp and the host side of spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule
// (include/spc.h) per column (l, i, j), in T, one rounding per operation, never an fma (the build has FP contraction off), no
// division and no transcendental function; w = kappa rho dz and c = dt / (cp rho dz exner) are profiles [n_les x ktot], etab a
// table of exp(-x) at the nodes m / inv_step, m = 0 ... n_tab - 1, that the caller hands in:
//   t[k]    = w[l][k] * ql[k]
//   B[0]    = +0;   B[k + 1] = B[k] + t[k]              the optical depth below face k + 1, sequential upward
//   A[ktot] = +0;   A[k]     = A[k + 1] + t[k]          the optical depth above face k, sequential downward
//   E(x)    = K12's table lookup (spc_thermo.hpp: th_sat) of x clamped to [0, x_hi]
//   F[k]    = f0[l] * E(A[k]) + f1[l] * E(B[k])         k = 0 ... ktot: the net upward flux at face k
//   thl'[k] = thl[k] - c[l][k] * (F[k + 1] - F[k]);   flux[k] = F[k + 1];   fsfc = F[0]
// The shape is the column tile of spc_coltile.hpp with (tiles, faces) = (2, 1) and TWO opposed chains; the pitch is one element
// longer than K15's because phase 3 keeps the ktot + 1 faces of a column in one row -- l is per column:
//   1. all RAD_THREADS lanes walk the ql run (rad_load, on col_split) and store t into both tiles;
//   2. lane c of wave 0 runs B up its column of one tile, B[k + 1] overwriting t[k]; lane c of wave 1 runs A down its column
//      of the other, A[k] overwriting t[k]: the two chains of a column run at once on two waves, the LDS reads of a chunk of
//      RAD_U levels issued before its arithmetic;
//   3. all lanes form F of the C * (ktot + 1) faces, two lookups per face, F[k] overwriting A[k] (a face reads and writes only
//      its own slots); then all lanes walk the run again: thl read, updated and written, flux written, the lane of level 0
//      writes fsfc.
// A workgroup writes only the cells it read, so the in-place update of thl needs no ordering beyond program order.  The table
// (16 KB of doubles at the 2 049 nodes of radiation.py) is read at data-dependent indices: LDS_TAB stages it once per workgroup
// in LDS behind the tiles where the budget has room and the CU keeps as many resident workgroups as without it; otherwise it is
// read from global memory (it stays in the caches).
#ifndef SPC_RADIATE_HOST

constexpr int RAD_THREADS = 256;
constexpr int RAD_U = 8;                        // levels per chunk of a chain
constexpr int RAD_UB = 4;                       // 16-byte vectors per lane and batch of the load and store phases

template <typename T> struct LesRadiateP {
    const T *ql;
    T *thl;
    const T *w, *c, *f0, *f1, *etab;
    T *flux;                       // or nullptr
    T *fsfc;                       // or nullptr
    int64_t ncols;                 // n_les * itot * jtot
    int64_t pitch_prof;
    T x_hi, inv_step;
    int32_t nij, ktot, n_tab;
    int32_t cols;                  // C: columns per workgroup
    int32_t vec;                   // ql, thl and flux lie equally on the 16-byte grid: the mover may use 16-byte accesses
};

// exp(-x) by the table: K12's lookup line for line
template <typename T> __device__ __forceinline__ T rad_E(const T *etab, const T x, const T x_hi, const T inv_step, const int n_tab)
{
    const T xc = x < (T)0 ? (T)0 : (x > x_hi ? x_hi : x);           // NaN passes through
    const T s = xc * inv_step;
    const int m = s >= (T)0 ? min((int)s, n_tab - 2) : 0;           // NaN: m = 0, and fr below stays NaN
    const T fr = s - (T)m;
    const T e0 = etab[m];
    const T d = etab[m + 1] - e0;
    const T t = fr * d;
    return e0 + t;
}

// B[k + 1] = B[k] + t[k] up one column in LDS, B[k + 1] overwriting t[k]
template <typename T> __device__ __forceinline__ void rad_up(T *x, const int ktot)
{
    T B = (T)0;
    int k = 0;
    for (; k + RAD_U <= ktot; k += RAD_U) {
        T ct[RAD_U];
#pragma unroll
        for (int u = 0; u < RAD_U; ++u) ct[u] = x[k + u];
#pragma unroll
        for (int u = 0; u < RAD_U; ++u) {
            B = B + ct[u];
            x[k + u] = B;
        }
    }
    for (; k < ktot; ++k) {
        B = B + x[k];
        x[k] = B;
    }
}

// A[k] = A[k + 1] + t[k] down one column in LDS, A[k] overwriting t[k]
template <typename T> __device__ __forceinline__ void rad_down(T *x, const int ktot)
{
    T A = (T)0;
    int k = ktot - 1;
    for (; k - RAD_U + 1 >= 0; k -= RAD_U) {
        T ct[RAD_U];
#pragma unroll
        for (int u = 0; u < RAD_U; ++u) ct[u] = x[k - u];
#pragma unroll
        for (int u = 0; u < RAD_U; ++u) {
            A = A + ct[u];
            x[k - u] = A;
        }
    }
    for (; k >= 0; --k) {
        A = A + x[k];
        x[k] = A;
    }
}

// phase 1: t = w * ql of the run -> both tiles
template <typename T>
__device__ __forceinline__ void rad_load(const LesRadiateP<T> &p, const T *g, T *ta, T *tb, const int len, const int P, const int64_t l0, const uint32_t rem0)
{
    constexpr int V = 16 / (int)sizeof(T);
    using Vec = SlabVec<T, V>;
    const int tid = threadIdx.x, ktot = p.ktot;
    const uint32_t nij = (uint32_t)p.nij;
    int head, nv;
    col_split<T>(g, len, p.vec, head, nv);
    const int tail0 = head + nv * V;
    for (int s = tid; s < head + (len - tail0); s += RAD_THREADS) {
        const int e = s < head ? s : tail0 + (s - head);
        const int c = e / ktot, k = e - c * ktot;
        const int64_t l = l0 + (rem0 + (uint32_t)c) / nij;           // per column: a tile may span several LES
        const T t = p.w[l * p.pitch_prof + k] * g[e];
        ta[c * P + k] = t;
        tb[c * P + k] = t;
    }
    const T *gv = g + head;
    for (int i0 = 0; i0 < nv; i0 += RAD_THREADS * RAD_UB) {
        Vec x[RAD_UB];
#pragma unroll
        for (int u = 0; u < RAD_UB; ++u) {
            const int i = i0 + u * RAD_THREADS + tid;
            if (i < nv) x[u] = *reinterpret_cast<const Vec *>(gv + (int64_t)i * V);
        }
#pragma unroll
        for (int u = 0; u < RAD_UB; ++u) {
            const int i = i0 + u * RAD_THREADS + tid;
            if (i < nv) {
                const int e = head + i * V;
                int c = e / ktot, k = e - c * ktot;
                const uint32_t q = rem0 + (uint32_t)c;
                uint32_t dl = q / nij, rem = q - dl * nij;
                int64_t wo = (l0 + dl) * p.pitch_prof;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const T t = p.w[wo + k] * x[u].v[v];
                    ta[c * P + k] = t;
                    tb[c * P + k] = t;
                    if (++k == ktot) {
                        k = 0;
                        ++c;
                        if (++rem == nij) { rem = 0; ++dl; }
                        wo = (l0 + dl) * p.pitch_prof;
                    }
                }
            }
        }
    }
}

// one cell of phase 3: the new thl, and F[k + 1] in up; F: the faces of the cell's column
template <typename T> __device__ __forceinline__ T rad_cell(const T *F, const int k, const T ck, const T x, T &up)
{
    const T lo = F[k];
    up = F[k + 1];
    const T dF = up - lo;
    const T t = ck * dF;
    return x - t;
}

// phase 3: thl, flux and fsfc of the run from the faces in the tile
template <typename T>
__device__ __forceinline__ void rad_store(const LesRadiateP<T> &p, T *g, T *fl, T *fs, const T *tf, const int len, const int P, const int64_t l0, const uint32_t rem0)
{
    constexpr int V = 16 / (int)sizeof(T);
    using Vec = SlabVec<T, V>;
    const int tid = threadIdx.x, ktot = p.ktot;
    const uint32_t nij = (uint32_t)p.nij;
    int head, nv;
    col_split<T>(g, len, p.vec, head, nv);
    const int tail0 = head + nv * V;
    for (int s = tid; s < head + (len - tail0); s += RAD_THREADS) {
        const int e = s < head ? s : tail0 + (s - head);
        const int c = e / ktot, k = e - c * ktot;
        const int64_t l = l0 + (rem0 + (uint32_t)c) / nij;
        T up;
        g[e] = rad_cell<T>(tf + c * P, k, p.c[l * p.pitch_prof + k], g[e], up);
        if (fl) fl[e] = up;
        if (fs && k == 0) fs[c] = tf[c * P];
    }
    T *gv = g + head;
    T *fv = fl ? fl + head : nullptr;
    for (int i0 = 0; i0 < nv; i0 += RAD_THREADS * RAD_UB) {
        Vec x[RAD_UB];
#pragma unroll
        for (int u = 0; u < RAD_UB; ++u) {
            const int i = i0 + u * RAD_THREADS + tid;
            if (i < nv) x[u] = *reinterpret_cast<const Vec *>(gv + (int64_t)i * V);
        }
#pragma unroll
        for (int u = 0; u < RAD_UB; ++u) {
            const int i = i0 + u * RAD_THREADS + tid;
            if (i < nv) {
                const int e = head + i * V;
                int c = e / ktot, k = e - c * ktot;
                const uint32_t q = rem0 + (uint32_t)c;
                uint32_t dl = q / nij, rem = q - dl * nij;
                int64_t co = (l0 + dl) * p.pitch_prof;
                Vec y;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    x[u].v[v] = rad_cell<T>(tf + c * P, k, p.c[co + k], x[u].v[v], y.v[v]);
                    if (fs && k == 0) fs[c] = tf[c * P];
                    if (++k == ktot) {
                        k = 0;
                        ++c;
                        if (++rem == nij) { rem = 0; ++dl; }
                        co = (l0 + dl) * p.pitch_prof;
                    }
                }
                *reinterpret_cast<Vec *>(gv + (int64_t)i * V) = x[u];
                if (fv) *reinterpret_cast<Vec *>(fv + (int64_t)i * V) = y;
            }
        }
    }
}

// grid ceil(ncols / C); dynamic LDS: 2 * C * col_pitch(ktot, 1) elements, and n_tab more where LDS_TAB
template <typename T, bool LDS_TAB> __global__ __launch_bounds__(RAD_THREADS) void k_les_radiate(const LesRadiateP<T> p)
{
    extern __shared__ __align__(16) unsigned char rad_lds[];
    const int ktot = p.ktot, P = col_pitch(ktot, 1), C = p.cols;
    T *ta = reinterpret_cast<T *>(rad_lds);                       // t, then A, then F
    T *tb = ta + C * P;                                            // t, then B
    const T *etab = p.etab;
    if (LDS_TAB) {
        T *tab = tb + C * P;
        for (int i = threadIdx.x; i < p.n_tab; i += RAD_THREADS) tab[i] = p.etab[i];
        etab = tab;
    }
    const ColRun tr(blockIdx.x, C, p.ncols, p.nij, ktot);
    // 1. t = w * ql of every cell of the run -> both tiles
    rad_load<T>(p, p.ql + tr.run, ta, tb, tr.len, P, tr.l0, tr.rem0);
    __syncthreads();
    // 2. the optical depths below (wave 0) and above (wave 1) the faces, one column per lane
    {
        const int wave = threadIdx.x >> 6, c = threadIdx.x & 63;
        if (wave == 0 && c < tr.nc) rad_up<T>(tb + c * P, ktot);
        if (wave == 1 && c < tr.nc) rad_down<T>(ta + c * P, ktot);
    }
    __syncthreads();
    // 3. F of every face, then thl, flux and fsfc of every cell
    const int nf = ktot + 1;
    for (int e = threadIdx.x; e < tr.nc * nf; e += RAD_THREADS) {
        const int c = e / nf, k = e - c * nf;
        const int64_t l = tr.l0 + (tr.rem0 + (uint32_t)c) / (uint32_t)p.nij;
        const T A = k < ktot ? ta[c * P + k] : (T)0;
        const T B = k ? tb[c * P + k - 1] : (T)0;
        const T Ea = rad_E<T>(etab, A, p.x_hi, p.inv_step, p.n_tab);
        const T Eb = rad_E<T>(etab, B, p.x_hi, p.inv_step, p.n_tab);
        const T Fa = p.f0[l] * Ea;
        const T Fb = p.f1[l] * Eb;
        ta[c * P + k] = Fa + Fb;
    }
    __syncthreads();
    rad_store<T>(p, p.thl + tr.run, p.flux ? p.flux + tr.run : nullptr, p.fsfc ? p.fsfc + tr.col0 : nullptr, ta, tr.len, P, tr.l0, tr.rem0);
}

#else  // SPC_RADIATE_HOST ---------------------------------------------------------------------------------------------------

template <typename T> static int les_radiate_impl(const spc_les_radiate_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_radiate", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    if (a->n_tab < 2) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_radiate: n_tab = %lld < 2", "", (long long)a->n_tab);
    if (!(a->inv_step > 0)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_radiate: inv_step must be > 0");
    if (a->pitch_prof < a->ktot)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_radiate: pitch_prof %lld smaller than ktot", "", (long long)a->pitch_prof);
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->ql, "ql"); REQUIRE(a->thl, "thl"); REQUIRE(a->w, "w"); REQUIRE(a->c, "c");
    REQUIRE(a->f0, "f0"); REQUIRE(a->f1, "f1"); REQUIRE(a->etab, "etab");
    // (equal base pointers are what is detected, as in K15: partially overlapping views are the caller's to avoid)
    const void *in[6] = {a->ql, a->w, a->c, a->f0, a->f1, a->etab};
    const void *wr[3] = {a->thl, a->flux, a->fsfc};
    static const char *const wname[3] = {"thl", "flux", "fsfc"};
    uintptr_t bits = 0;
    if ((rc = col_alias("les_radiate", in, 6, wr, 3, wname, bits))) return rc;
    if (bits % sizeof(T)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_radiate: a pointer is not aligned to its element type");
    const int C = col_cols(a->ktot, (int)sizeof(T), 2, 1);
    if (!C)
        return fail(SPC_ERR_UNSUPPORTED, "%sles_radiate: ktot %lld above the %lld levels of which 16 columns fit the LDS", "", (long long)a->ktot,
                    (long long)col_max_ktot((int)sizeof(T), 2, 1));
    LesRadiateP<T> p = {};
    p.ql = (const T *)a->ql; p.thl = (T *)a->thl; p.w = (const T *)a->w; p.c = (const T *)a->c;
    p.f0 = (const T *)a->f0; p.f1 = (const T *)a->f1; p.etab = (const T *)a->etab;
    p.flux = (T *)a->flux; p.fsfc = (T *)a->fsfc;
    p.nij = a->itot * a->jtot;
    p.ncols = a->n_les * (int64_t)p.nij;
    p.pitch_prof = a->pitch_prof;
    p.ktot = a->ktot; p.n_tab = a->n_tab; p.cols = C;
    p.inv_step = (T)a->inv_step;
    p.x_hi = (T)((double)(a->n_tab - 1) / a->inv_step);
    p.vec = (uintptr_t)a->ql % 16 == (uintptr_t)a->thl % 16 && (!a->flux || (uintptr_t)a->flux % 16 == (uintptr_t)a->thl % 16);
    int64_t grid;
    if ((rc = col_grid("les_radiate", p.ncols, C, grid))) return rc;
    const size_t tiles = (size_t)2 * C * col_pitch(a->ktot, 1) * sizeof(T), tab = (size_t)a->n_tab * sizeof(T);
    // the table goes behind the tiles where the budget has room AND it costs the CU no resident workgroup: the launch is bound
    // by the latency of a tile's phases, which only other workgroups hide (measured: DESIGN.md 7.3)
    const bool lds_tab = tiles + tab <= (size_t)(C == 16 ? HARD_LDS_BYTES : MAX_LDS_BYTES) && HARD_LDS_BYTES / (tiles + tab) == HARD_LDS_BYTES / tiles;
    const size_t smem = tiles + (lds_tab ? tab : 0);
    void (*const kernel)(const LesRadiateP<T>) = lds_tab ? k_les_radiate<T, true> : k_les_radiate<T, false>;
    if ((rc = ensure_lds(kernel, smem, "k_les_radiate"))) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(RAD_THREADS), smem, (hipStream_t)stream, p);
    return launch_status("k_les_radiate");
}

#endif
