// spc_buoyancy.hpp -- K21: the hydrostatic pressure force of the device-resident LES fields, kernels and host side.  The buoyancy
// of every column is integrated downward from the lid to a pressure perturbation phi (k_les_hydrostatic), and the horizontal
// gradient of phi accelerates U and V in place (k_les_pgrad); continuity (K17) then turns the convergence into vertical motion.
// spc_hip.hip includes it twice, like spc_radiate.hpp and spc_advect.hpp: with the kernels among the device headers, and --
// SPC_BUOYANCY_HOST defined -- after spc_launch.hpp and the host side of spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule
// (include/spc.h), in T, one rounding per operation, never an fma (the build has FP contraction off), no division and no
// transcendental function; t0, lex and s are profiles [n_les x ktot], hx and hy [n_les] are K16's.  Per cell (l, i, j, k):
//   e   = lex[l][k] * ql                 (ql == NULL: e = +0 and m = 1 + c1 * qt)
//   tl  = thl + e
//   m   = (1 + c1 * qt) - c2 * ql
//   tv  = tl * m
//   b   = (tv - t0[l][k]) * s[l][k]
//   q[ktot] = +0;   phi[k] = q[k + 1] - b[k];   q[k] = phi[k] - b[k]       sequential downward
//   psfc = q[0]
// and then, with ip, im, jp, jm the periodic neighbours as K16 forms them:
//   gx = phi[ip] - phi[im];   du = hx[l] * gx;   u' = u - du
//   gy = phi[jp] - phi[jm];   dv = hy[l] * gy;   v' = v - dv
//   a  = |du| + |dv|;         amax[l] = max over the cells of LES l of a
// k_les_hydrostatic is the column tile of spc_coltile.hpp with (tiles, faces) = (1, 0) and ONE chain -- l is per column:
//   1. all HYD_THREADS lanes walk the thl, qt and ql runs (hyd_load, on col_split: 16-byte loads where the three lie
//      equally on the 16-byte grid) and store b into the tile;
//   2. lane c runs the chain down its column, phi[k] overwriting b[k], the LDS reads of a chunk of HYD_U levels issued before
//      its arithmetic, and writes psfc (consecutive lanes, consecutive columns);
//   3. all lanes write phi of the run back (hyd_store: one vector per lane and iteration).
// k_les_pgrad has K16's shape: a workgroup owns ADVECT_THREADS consecutive cells q = j * ktot + k of the contiguous run of a row
// i and advect_rows() consecutive rows; a lane walks its rows with a three-row register window of phi, so each phi is fetched
// once for the i direction and rows i0 - 1 and i1 (wrapped) once more per workgroup.  phi at j - 1 and j + 1 is ktot cells away
// in the same run: other lanes fetch them as their own cells at the same time.  A lane reads and writes only its own cell of u
// and v, so the in-place update needs no ordering.  amax: the bit pattern of a with the sign cleared orders like the value,
// and a NaN lies above every number: every lane keeps the largest pattern, a wave reduces by shuffles and its first lane issues
// one atomicMax (K16's), so a NaN of any cell makes amax[l] a NaN; the launcher zeroes amax first.
#ifndef SPC_BUOYANCY_HOST

constexpr int HYD_THREADS = 256;
constexpr int HYD_U = 8;                        // levels per chunk of the chain
constexpr int HYD_UB = 4;                       // 16-byte vectors per lane, array and batch of the load and store phases

template <typename T> struct LesBuoyancyP {
    const T *thl, *qt, *ql;        // ql or nullptr
    T *u, *v;
    const T *hx, *hy;
    const T *t0, *lex, *s;
    T *phi;
    T *psfc;                       // or nullptr
    T *amax;                       // or nullptr
    int64_t ncols;                 // n_les * itot * jtot
    int64_t pitch_prof;
    int64_t row;                   // jtot * ktot: cells of one row i
    T c1, c2;
    int32_t nij, itot, jtot, ktot;
    int32_t cols;                  // C: columns per workgroup of k_les_hydrostatic
    int32_t vec;                   // thl, qt and ql lie equally on the 16-byte grid: the mover may load 16 bytes at once
    int32_t nchunk, nseg, rows;    // k_les_pgrad: workgroups along the flat run and along i, rows i per workgroup
};

// the half-layer buoyancy integral of one cell; po: the cell's place in the profiles
template <typename T, bool QL> __device__ __forceinline__ T hyd_b(const LesBuoyancyP<T> &p, const int64_t po, const T thl, const T qt, const T ql)
{
    const T e = QL ? p.lex[po] * ql : (T)0;
    const T tl = thl + e;
    const T a = p.c1 * qt;
    T m = (T)1 + a;
    if (QL) {
        const T w = p.c2 * ql;
        m = m - w;
    }
    const T tv = tl * m;
    const T d = tv - p.t0[po];
    return d * p.s[po];
}

// the level that step s of the chain works on: downward from the lid
__device__ __forceinline__ int hyd_level(const int ktot, const int s) { return ktot - 1 - s; }

// phi[k] = q[k + 1] - b[k]; q[k] = phi[k] - b[k] down one column in LDS, phi[k] overwriting b[k]; returns q[0]
template <typename T> __device__ __forceinline__ T hyd_chain(T *x, const int ktot)
{
    T q = (T)0;
    int s = 0;
    for (; s + HYD_U <= ktot; s += HYD_U) {
        T cb[HYD_U];
#pragma unroll
        for (int u = 0; u < HYD_U; ++u) cb[u] = x[hyd_level(ktot, s + u)];
#pragma unroll
        for (int u = 0; u < HYD_U; ++u) {
            const T f = q - cb[u];
            q = f - cb[u];
            x[hyd_level(ktot, s + u)] = f;
        }
    }
    for (; s < ktot; ++s) {
        const T b = x[hyd_level(ktot, s)];
        const T f = q - b;
        q = f - b;
        x[hyd_level(ktot, s)] = f;
    }
    return q;
}

// phase 1: b of the run -> the tile
template <typename T, bool QL>
__device__ __forceinline__ void hyd_load(const LesBuoyancyP<T> &p, const T *thl, const T *qt, const T *ql, T *tile, const int len, const int P,
                                         const int64_t l0, const uint32_t rem0)
{
    constexpr int V = 16 / (int)sizeof(T);
    using Vec = SlabVec<T, V>;
    const int tid = threadIdx.x, ktot = p.ktot;
    const uint32_t nij = (uint32_t)p.nij;
    int head, nv;
    col_split<T>(thl, len, p.vec, head, nv);
    const int tail0 = head + nv * V;
    for (int s = tid; s < head + (len - tail0); s += HYD_THREADS) {
        const int e = s < head ? s : tail0 + (s - head);
        const int c = e / ktot, k = e - c * ktot;
        const int64_t l = l0 + (rem0 + (uint32_t)c) / nij;           // per column: a tile may span several LES
        tile[c * P + k] = hyd_b<T, QL>(p, l * p.pitch_prof + k, thl[e], qt[e], QL ? ql[e] : (T)0);
    }
    for (int i0 = 0; i0 < nv; i0 += HYD_THREADS * HYD_UB) {
        Vec x[HYD_UB], y[HYD_UB], z[HYD_UB];
#pragma unroll
        for (int u = 0; u < HYD_UB; ++u) {
            const int i = i0 + u * HYD_THREADS + tid;
            if (i < nv) {
                const int64_t o = head + (int64_t)i * V;
                x[u] = *reinterpret_cast<const Vec *>(thl + o);
                y[u] = *reinterpret_cast<const Vec *>(qt + o);
                if (QL) z[u] = *reinterpret_cast<const Vec *>(ql + o);
            }
        }
#pragma unroll
        for (int u = 0; u < HYD_UB; ++u) {
            const int i = i0 + u * HYD_THREADS + tid;
            if (i < nv) {
                const int e = head + i * V;
                int c = e / ktot, k = e - c * ktot;
                const uint32_t q = rem0 + (uint32_t)c;
                uint32_t dl = q / nij, rem = q - dl * nij;
                int64_t po = (l0 + dl) * p.pitch_prof;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    tile[c * P + k] = hyd_b<T, QL>(p, po + k, x[u].v[v], y[u].v[v], QL ? z[u].v[v] : (T)0);
                    if (++k == ktot) {
                        k = 0;
                        ++c;
                        if (++rem == nij) { rem = 0; ++dl; }
                        po = (l0 + dl) * p.pitch_prof;
                    }
                }
            }
        }
    }
}

// phase 3: phi of the run from the tile
template <typename T> __device__ __forceinline__ void hyd_store(T *g, const T *tile, const int len, const int P, const int ktot)
{
    constexpr int V = 16 / (int)sizeof(T);
    using Vec = SlabVec<T, V>;
    const int tid = threadIdx.x;
    int head, nv;
    col_split<T>(g, len, 1, head, nv);
    const int tail0 = head + nv * V;
    for (int s = tid; s < head + (len - tail0); s += HYD_THREADS) {
        const int e = s < head ? s : tail0 + (s - head);
        const int c = e / ktot, k = e - c * ktot;
        g[e] = tile[c * P + k];
    }
    T *gv = g + head;
    for (int i = tid; i < nv; i += HYD_THREADS) {
        const int e = head + i * V;
        int c = e / ktot, k = e - c * ktot;
        Vec y;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            y.v[v] = tile[c * P + k];
            if (++k == ktot) { k = 0; ++c; }
        }
        *reinterpret_cast<Vec *>(gv + (int64_t)i * V) = y;
    }
}

// grid ceil(ncols / C); dynamic LDS: C * col_pitch(ktot, 0) elements
template <typename T, bool QL> __global__ __launch_bounds__(HYD_THREADS) void k_les_hydrostatic(const LesBuoyancyP<T> p)
{
    extern __shared__ __align__(16) unsigned char hyd_lds[];
    const int ktot = p.ktot, P = col_pitch(ktot, 0);
    T *tile = reinterpret_cast<T *>(hyd_lds);                     // b, then phi
    const ColRun tr(blockIdx.x, p.cols, p.ncols, p.nij, ktot);
    // 1. b of every cell of the run -> the tile
    hyd_load<T, QL>(p, p.thl + tr.run, p.qt + tr.run, QL ? p.ql + tr.run : nullptr, tile, tr.len, P, tr.l0, tr.rem0);
    __syncthreads();
    // 2. the chain down every column, one column per lane; q[0] is the perturbation at the ground
    if ((int)threadIdx.x < tr.nc) {
        const T q0 = hyd_chain<T>(tile + threadIdx.x * P, ktot);
        if (p.psfc) p.psfc[tr.col0 + threadIdx.x] = q0;
    }
    __syncthreads();
    // 3. phi of every cell of the run
    hyd_store<T>(p.phi + tr.run, tile, tr.len, P, ktot);
}

template <typename T> struct BuoyancyBits;
template <> struct BuoyancyBits<double> { using type = unsigned long long; static constexpr unsigned long long mask = 0x7fffffffffffffffull; };
template <> struct BuoyancyBits<float> { using type = unsigned int; static constexpr unsigned int mask = 0x7fffffffu; };

// grid nchunk * nseg * n_les (the chunk fastest: neighbouring workgroups share their j - 1 / j + 1 cells)
template <typename T> __global__ __launch_bounds__(ADVECT_THREADS) void k_les_pgrad(const LesBuoyancyP<T> p)
{
    using U = typename BuoyancyBits<T>::type;
    const int64_t b = blockIdx.x;
    const int chunk = (int)(b % p.nchunk);
    const int seg = (int)((b / p.nchunk) % p.nseg);
    const int64_t l = b / ((int64_t)p.nchunk * p.nseg);
    const int itot = p.itot, ktot = p.ktot;
    const int64_t row = p.row;
    const int64_t q = (int64_t)chunk * ADVECT_THREADS + threadIdx.x;
    U amax = 0;
    if (q < row) {
        int64_t qs = q - ktot;                                       // j - 1
        if (qs < 0) qs += row;
        int64_t qn = q + ktot;                                       // j + 1
        if (qn >= row) qn -= row;
        const T hx = p.hx[l], hy = p.hy[l];
        const int i0 = seg * p.rows;
        const int i1 = i0 + p.rows < itot ? i0 + p.rows : itot;
        const int64_t les = l * itot * row;
        const int64_t bw = les + (int64_t)(i0 ? i0 - 1 : itot - 1) * row;
        int64_t bi = les + (int64_t)i0 * row;
        T fm = p.phi[bw + q], fc = p.phi[bi + q];                    // phi at i - 1 and i
        for (int i = i0; i < i1; ++i) {
            const int ip = i + 1 == itot ? 0 : i + 1;
            const int64_t be = les + (int64_t)ip * row;
            const T fp = p.phi[be + q];
            const T fjm = p.phi[bi + qs], fjp = p.phi[bi + qn];
            const T u = p.u[bi + q], v = p.v[bi + q];
            const T gx = fp - fm;
            const T gy = fjp - fjm;
            const T du = hx * gx;
            const T dv = hy * gy;
            p.u[bi + q] = u - du;
            p.v[bi + q] = v - dv;
            const T au = du < (T)0 ? -du : du, av = dv < (T)0 ? -dv : dv;
            const T a = au + av;
            U bits;
            __builtin_memcpy(&bits, &a, sizeof(T));
            bits &= BuoyancyBits<T>::mask;
            amax = bits > amax ? bits : amax;
            fm = fc;
            fc = fp;
            bi = be;
        }
    }
    if (p.amax) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const U o = __shfl_xor(amax, d, 64);
            amax = o > amax ? o : amax;
        }
        if ((threadIdx.x & 63) == 0 && amax) atomicMax(reinterpret_cast<U *>(p.amax) + l, amax);
    }
}

#else  // SPC_BUOYANCY_HOST --------------------------------------------------------------------------------------------------

template <typename T> static int les_buoyancy_impl(const spc_les_buoyancy_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_buoyancy", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    if (a->pitch_prof < a->ktot)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_buoyancy: pitch_prof %lld smaller than ktot", "", (long long)a->pitch_prof);
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->thl, "thl"); REQUIRE(a->qt, "qt"); REQUIRE(a->u, "u"); REQUIRE(a->v, "v"); REQUIRE(a->phi, "phi");
    REQUIRE(a->hx, "hx"); REQUIRE(a->hy, "hy"); REQUIRE(a->t0, "t0"); REQUIRE(a->lex, "lex"); REQUIRE(a->s, "s");
    // (equal base pointers are what is detected, as in K15: partially overlapping views are the caller's to avoid)
    const void *in[8] = {a->thl, a->qt, a->ql, a->hx, a->hy, a->t0, a->lex, a->s};
    const void *wr[5] = {a->phi, a->u, a->v, a->psfc, a->amax};
    static const char *const wname[5] = {"phi", "u", "v", "psfc", "amax"};
    uintptr_t bits = 0;
    if ((rc = col_alias("les_buoyancy", in, 8, wr, 5, wname, bits))) return rc;
    if (bits % sizeof(T)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_buoyancy: a pointer is not aligned to its element type");
    const int C = col_cols(a->ktot, (int)sizeof(T), 1, 0);
    if (!C)
        return fail(SPC_ERR_UNSUPPORTED, "%sles_buoyancy: ktot %lld above the %lld levels of which 16 columns fit the LDS", "", (long long)a->ktot,
                    (long long)col_max_ktot((int)sizeof(T), 1, 0));
    LesBuoyancyP<T> p = {};
    p.thl = (const T *)a->thl; p.qt = (const T *)a->qt; p.ql = (const T *)a->ql;
    p.u = (T *)a->u; p.v = (T *)a->v; p.hx = (const T *)a->hx; p.hy = (const T *)a->hy;
    p.t0 = (const T *)a->t0; p.lex = (const T *)a->lex; p.s = (const T *)a->s;
    p.phi = (T *)a->phi; p.psfc = (T *)a->psfc; p.amax = (T *)a->amax;
    p.c1 = (T)a->c1; p.c2 = (T)a->c2;
    p.nij = a->itot * a->jtot;
    p.ncols = a->n_les * (int64_t)p.nij;
    p.pitch_prof = a->pitch_prof;
    p.itot = a->itot; p.jtot = a->jtot; p.ktot = a->ktot; p.cols = C;
    p.row = (int64_t)a->jtot * a->ktot;
    p.vec = (uintptr_t)a->qt % 16 == (uintptr_t)a->thl % 16 && (!a->ql || (uintptr_t)a->ql % 16 == (uintptr_t)a->thl % 16);
    p.rows = advect_rows(a->n_les, a->itot, a->jtot, a->ktot);
    int64_t hgrid;
    if ((rc = col_grid("les_buoyancy", p.ncols, C, hgrid))) return rc;
    const int64_t nchunk = (p.row + ADVECT_THREADS - 1) / ADVECT_THREADS, nseg = (a->itot + p.rows - 1) / p.rows;
    if (nchunk > INT32_MAX || (double)nchunk * (double)nseg * (double)a->n_les > (double)INT32_MAX)
        return fail(SPC_ERR_UNSUPPORTED, "%sles_buoyancy: too many workgroups");
    p.nchunk = (int32_t)nchunk; p.nseg = (int32_t)nseg;
    const size_t smem = (size_t)C * col_pitch(a->ktot, 0) * sizeof(T);
    void (*const kernel)(const LesBuoyancyP<T>) = a->ql ? k_les_hydrostatic<T, true> : k_les_hydrostatic<T, false>;
    if ((rc = ensure_lds(kernel, smem, "k_les_hydrostatic"))) return rc;
    if (a->amax && hipMemsetAsync(a->amax, 0, (size_t)a->n_les * sizeof(T), (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SPC_ERR_LAUNCH, "%sles_buoyancy: amax could not be zeroed");
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)hgrid), dim3(HYD_THREADS), smem, (hipStream_t)stream, p);
    if ((rc = launch_status("k_les_hydrostatic"))) return rc;
    hipLaunchKernelGGL(k_les_pgrad<T>, dim3((unsigned)(nchunk * nseg * a->n_les)), dim3(ADVECT_THREADS), 0, (hipStream_t)stream, p);
    return launch_status("k_les_pgrad");
}

#endif
