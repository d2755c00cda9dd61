// spc_vadvect.hpp -- K17: one explicit first-order upwind step of the VERTICAL advection of the device-resident LES fields by
// the mass flux that continuity gives the horizontal winds, kernel and host side.  spc_hip.hip includes it twice, like
// spc_diffuse.hpp and spc_advect.hpp: with the kernel among the device headers, and -- SPC_VADVECT_HOST defined -- after
// spc_launch.hpp and the host side of spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule
// (include/spc.h) per cell (l, i, j, k), in T, one rounding per operation, never an fma (the build has FP contraction off), no
// division, im / ip / jm / jp the periodic neighbours, g = rho dz and r = 1 / g the profiles [n_les x ktot]:
//   cw, ce, cs, cn  K16's face Courant numbers at level k (spc_advect.hpp)
//   d  = (ce - cw) + (cn - cs);   e = g[l][k] * d
//   M[0] = +0;   M[k + 1] = M[k] - e                      the mass through the upper face, sequential in k from the ground
//   cb = M[k] * r[l][k];   ct = M[k + 1] * r[l][k];   pb = cb > 0 ? cb : 0;   pt = ct < 0 ? -ct : 0
//   x' = (x + pb * (x[km] - x)) + pt * (x[kp] - x)        km = k ? k - 1 : 0, kp = k + 1 < ktot ? k + 1 : ktot - 1
//   s  = pb + pt;   cmax[l] = max over the cells of LES l of s;   mtop[l][i][j][k] = M[k + 1]
// The shape joins K16's neighbours across i and j with K15's serial chain along k.  A workgroup takes C consecutive columns of
// the flat column index (the column tile of spc_coltile.hpp with (tiles, faces) = (1, 0): geometry and ColRun), a contiguous run of
// C * ktot cells that may span rows i and LES -- l, i and j are per column:
//   1. all VAD_THREADS lanes walk the run coalesced (a lane takes every VAD_THREADS-th cell, so a wave's accesses are one
//      contiguous stretch whatever ktot is and a view off the 16-byte grid takes the same path), form e from the six wind
//      values of the cell and store it to LDS, column c at c * pitch, pitch = ktot | 1: ODD, so the lanes of phase 2 that read
//      the same k of their columns hit distinct banks;
//   2. lane c < C runs M[k + 1] = M[k] - e[k] up its column in LDS, M[k + 1] overwriting e[k]: one dependent subtraction per
//      level, the LDS reads of a chunk of VAD_U levels issued before its arithmetic;
//   3. all lanes walk the run again: M[k] and M[k + 1] from LDS, x[km], x, x[kp] from global memory (the k - 1 / k + 1 values lie
//      in the cache lines the neighbouring lanes fetch as their own cells), out[f] and mtop written coalesced.  The face
//      numbers pb, pt of a cell are formed once and used by all NF fields (a template argument).
// The tile is C * pitch elements whatever the number of fields.  cmax: a lane keeps the maximum of its s for the LES it is in
// (its cells come in ascending l; it issues an atomicMax of its own when l changes, which happens only in a tile that spans
// LES); at the end a wave whose lanes all ended in one LES reduces by shuffles and its first lane issues ONE atomicMax on the
// unsigned bit pattern (s is never NaN and never negative: the order of the patterns is the order of the values), else every
// lane issues its own.  The launcher zeroes cmax first.  The outputs are separate buffers written whole, so no workgroup
// waits for another.
#ifndef SPC_VADVECT_HOST

constexpr int VAD_THREADS = 256;
constexpr int VAD_MAXF = 6;
constexpr int VAD_U = 8;                        // levels per chunk of the column recurrence

template <typename T> struct LesVadvectP {
    const T *u, *v;
    const T *field[VAD_MAXF];
    T *out[VAD_MAXF];
    const T *hx, *hy;
    const T *g, *r;
    T *cmax;                       // or nullptr
    T *mtop;                       // or nullptr
    int64_t ncols;                 // n_les * itot * jtot
    int64_t pitch_prof;
    int32_t itot, jtot, ktot;
    int32_t nij;                   // itot * jtot
    int32_t cols;                  // C: columns per workgroup
};

// where cell e of a workgroup's run lies: column c of the tile, level k, LES l, row i and j
struct VadCell {
    int c, k, i, j;
    int64_t l;
};

__device__ __forceinline__ VadCell vad_cell(const int e, const int ktot, const int64_t l0, const uint32_t rem0, const uint32_t nij, const uint32_t jtot)
{
    VadCell w;
    w.c = e / ktot;
    w.k = e - w.c * ktot;
    const uint32_t q = rem0 + (uint32_t)w.c;                     // the column within LES l0, or beyond it: a tile may span LES
    const uint32_t dl = q / nij, rem = q - dl * nij;
    w.l = l0 + dl;
    w.i = (int)(rem / jtot);
    w.j = (int)(rem - (uint32_t)w.i * jtot);
    return w;
}

template <typename T> __device__ __forceinline__ void vad_atomic_max(T *cmax, const int64_t l, const T s)
{
    using U = typename AdvectBits<T>::type;
    U bits;
    __builtin_memcpy(&bits, &s, sizeof(T));
    if (bits) atomicMax(reinterpret_cast<U *>(cmax) + l, bits);
}

// M[k + 1] = M[k] - e[k] up one column in LDS, M[k + 1] overwriting e[k]
template <typename T> __device__ __forceinline__ void vad_column(T *x, const int ktot)
{
    T M = (T)0;
    int k = 0;
    for (; k + VAD_U <= ktot; k += VAD_U) {
        T ce[VAD_U];
#pragma unroll
        for (int u = 0; u < VAD_U; ++u) ce[u] = x[k + u];
#pragma unroll
        for (int u = 0; u < VAD_U; ++u) {
            M = M - ce[u];
            x[k + u] = M;
        }
    }
    for (; k < ktot; ++k) {
        M = M - x[k];
        x[k] = M;
    }
}

// grid ceil(ncols / C); dynamic LDS: C * col_pitch(ktot, 0) elements
template <typename T, int NF> __global__ __launch_bounds__(VAD_THREADS) void k_les_vadvect(const LesVadvectP<T> p)
{
    extern __shared__ __align__(16) unsigned char vad_lds[];
    T *tile = reinterpret_cast<T *>(vad_lds);
    const int ktot = p.ktot, P = col_pitch(ktot, 0), C = p.cols;
    const int itot = p.itot, jtot = p.jtot;
    const ColRun tr(blockIdx.x, C, p.ncols, p.nij, ktot);
    const int64_t row = (int64_t)jtot * ktot;                    // cells of one row i
    // 1. e = g * ((ce - cw) + (cn - cs)) of every cell of the run -> LDS
    for (int e = threadIdx.x; e < tr.len; e += VAD_THREADS) {
        const VadCell w = vad_cell(e, ktot, tr.l0, tr.rem0, (uint32_t)p.nij, (uint32_t)jtot);
        const int64_t o = tr.run + e;
        const int64_t ow = o + (w.i ? -row : (int64_t)(itot - 1) * row);
        const int64_t oe = o + (w.i + 1 < itot ? row : -(int64_t)(itot - 1) * row);
        const int64_t os = o + (w.j ? -(int64_t)ktot : (int64_t)(jtot - 1) * ktot);
        const int64_t on = o + (w.j + 1 < jtot ? (int64_t)ktot : -(int64_t)(jtot - 1) * ktot);
        const T uw = p.u[ow], uc = p.u[o], ue = p.u[oe];
        const T vs = p.v[os], vc = p.v[o], vn = p.v[on];
        const T hx = p.hx[w.l], hy = p.hy[w.l];
        const T gk = p.g[w.l * p.pitch_prof + w.k];
        const T aw = uw + uc, ae = uc + ue, as = vs + vc, an = vc + vn;
        const T cw = aw * hx;
        const T ce = ae * hx;
        const T cs = as * hy;
        const T cn = an * hy;
        const T dx = ce - cw;
        const T dy = cn - cs;
        const T d = dx + dy;
        tile[w.c * P + w.k] = gk * d;
    }
    __syncthreads();
    // 2. the mass flux through the upper faces, one column per lane
    if ((int)threadIdx.x < tr.nc) vad_column<T>(tile + threadIdx.x * P, ktot);
    __syncthreads();
    // 3. the upwind step of every field, mtop and the Courant sums
    T smax = (T)0;
    int64_t lcur = -1;
    for (int e = threadIdx.x; e < tr.len; e += VAD_THREADS) {
        const VadCell w = vad_cell(e, ktot, tr.l0, tr.rem0, (uint32_t)p.nij, (uint32_t)jtot);
        const int64_t o = tr.run + e;
        const int k = w.k;
        const T *M = tile + w.c * P;
        const T Mb = k ? M[k - 1] : (T)0;
        const T Mt = M[k];
        const int64_t okm = k ? o - 1 : o;
        const int64_t okp = k + 1 < ktot ? o + 1 : o;
        const T rk = p.r[w.l * p.pitch_prof + k];
        const T cb = Mb * rk;
        const T ct = Mt * rk;
        const T pb = cb > (T)0 ? cb : (T)0;
        const T pt = ct < (T)0 ? -ct : (T)0;
        const T s = pb + pt;
        if (p.cmax) {
            if (w.l != lcur) {                                   // the lane's cells come in ascending l
                if (lcur >= 0) vad_atomic_max<T>(p.cmax, lcur, smax);
                lcur = w.l;
                smax = (T)0;
            }
            smax = s > smax ? s : smax;
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const T x = p.field[f][o], xm = p.field[f][okm], xp = p.field[f][okp];
            const T db = xm - x, dt = xp - x;
            const T tb = pb * db;
            const T tt = pt * dt;
            T y = x + tb;
            y = y + tt;
            p.out[f][o] = y;
        }
        if (p.mtop) p.mtop[o] = Mt;
    }
    if (p.cmax) {
        long long lw = lcur;                                     // the last LES of the wave (-1: no lane had a cell)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const long long o = __shfl_xor(lw, d, 64);
            lw = o > lw ? o : lw;
        }
        if (__all(lcur < 0 || lcur == lw)) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const T o = __shfl_xor(smax, d, 64);
                smax = o > smax ? o : smax;
            }
            if ((threadIdx.x & 63) == 0 && lw >= 0) vad_atomic_max<T>(p.cmax, lw, smax);
        } else if (lcur >= 0) {
            vad_atomic_max<T>(p.cmax, lcur, smax);
        }
    }
}

#else  // SPC_VADVECT_HOST ---------------------------------------------------------------------------------------------------

// ---- the host path that K17, K22 and K23 share ----------------------------------------------------------------------------------
// The three kernels take one tile (spc_coltile.hpp, (tiles, faces) = (1, 0)), one grid and the same arrays; their argument blocks are ONE layout that
// grew at its end (K22 added ftop, K23 the limiter), which include/spc.h spells out three times.  The shared code reads the
// members by name, so it does not depend on that, but the Python side builds the blocks from one another (_abi.py):
#define VAD_SAME_OFFSET(m)                                                                                                 \
    static_assert(offsetof(spc_les_vadvect_args, m) == offsetof(spc_les_transport_args, m) &&                             \
                      offsetof(spc_les_transport_args, m) == offsetof(spc_les_transport2_args, m),                        \
                  "spc_les_vadvect_args, spc_les_transport_args and spc_les_transport2_args disagree on " #m)
VAD_SAME_OFFSET(n_les); VAD_SAME_OFFSET(itot); VAD_SAME_OFFSET(jtot); VAD_SAME_OFFSET(ktot); VAD_SAME_OFFSET(n_fields);
VAD_SAME_OFFSET(u); VAD_SAME_OFFSET(v); VAD_SAME_OFFSET(fields); VAD_SAME_OFFSET(out); VAD_SAME_OFFSET(hx); VAD_SAME_OFFSET(hy);
VAD_SAME_OFFSET(cmax); VAD_SAME_OFFSET(g); VAD_SAME_OFFSET(r); VAD_SAME_OFFSET(pitch_prof); VAD_SAME_OFFSET(mtop);
#undef VAD_SAME_OFFSET
static_assert(offsetof(spc_les_transport_args, ftop) == offsetof(spc_les_transport2_args, ftop), "spc_les_transport_args and spc_les_transport2_args disagree on ftop");
static_assert(sizeof(spc_les_vadvect_args) == offsetof(spc_les_transport_args, ftop) && sizeof(spc_les_transport_args) == offsetof(spc_les_transport2_args, limiter),
              "each argument block of the family is the one before it with members added at its end");

// Every check of the argument block ``a`` of kernel ``name`` (the name in the texts of spc_last_error()), in the order a caller
// can observe, then the parameter block ``p`` filled and cmax zeroed on ``stream``.  A is one of the three args structs, P the
// kernel's LesVadvectP<T> / LesTransportP<T>; ftop is taken where A has one (every A but K17's).  ``more`` is a check of the
// kernel's own that is made after the field count and before "nothing to do" (K23's limiter), or nullptr.  After SPC_OK the
// caller launches its kernel -- unless p.cols is still 0: an ensemble without LES, for which no pointer was looked at.
template <typename T, typename A, typename P> static int vad_family_args(const char *name, const A *a, P &p, void *stream, int (*more)(const A *) = nullptr)
{
    constexpr bool HAS_FTOP = !std::is_same<A, spc_les_vadvect_args>::value;
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents(name, a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    if (a->n_fields < 0 || a->n_fields > VAD_MAXF)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%s: field count %lld outside 0 ... %lld", name, (long long)a->n_fields, (long long)VAD_MAXF);
    if (more && (rc = more(a)) != SPC_OK) return rc;
    if (a->n_fields == 0 && !a->cmax && !a->mtop) return fail(SPC_ERR_INVALID_ARGUMENT, "%s: no field, no cmax and no mtop: nothing to do", name);
    if (a->pitch_prof < a->ktot) return fail(SPC_ERR_INVALID_ARGUMENT, "%s: pitch_prof %lld smaller than ktot", name, (long long)a->pitch_prof);
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->u, "u"); REQUIRE(a->v, "v"); REQUIRE(a->hx, "hx"); REQUIRE(a->hy, "hy"); REQUIRE(a->g, "g"); REQUIRE(a->r, "r");
    // (equal base pointers are what is detected, as in K11, K14, K15 and K16: partially overlapping views are the caller's to avoid)
    const void *in[6 + VAD_MAXF] = {a->u, a->v, a->hx, a->hy, a->g, a->r};
    const void *wr[3 + VAD_MAXF];
    int n_in = 6, n_wr = 0;
    uintptr_t bits = 0;
    for (int f = 0; f < a->n_fields; ++f) {
        REQUIRE(a->fields[f], "fields[f]");
        REQUIRE(a->out[f], "out[f]");
        in[n_in++] = a->fields[f];
        p.field[f] = (const T *)a->fields[f];
        p.out[f] = (T *)a->out[f];
    }
    for (int f = 0; f < a->n_fields; ++f) {
        for (int q = 0; q < n_wr; ++q)
            if (wr[q] == a->out[f])
                return fail(SPC_ERR_INVALID_ARGUMENT, "%s: out[%lld] and out[%lld] are the same array", name, (long long)q, (long long)f);
        for (int q = 0; q < n_in; ++q)
            if (in[q] == a->out[f])
                return fail(SPC_ERR_INVALID_ARGUMENT, "%s: out[%lld] is also an input (every cell reads its neighbours' old values)", name, (long long)f);
        wr[n_wr++] = a->out[f];
    }
    void *ftop = nullptr;
    if constexpr (HAS_FTOP) ftop = a->n_fields ? a->ftop : nullptr;   // (no field: nothing of ftop to write)
    const void *extra[3] = {a->mtop, a->cmax, ftop};
    static const char *const extra_name[3] = {"mtop", "cmax", "ftop"};
    for (int x = 0; x < 3; ++x) {
        if (!extra[x]) continue;
        char who[64];                                                 // "<kernel>: <array>": fail() takes one string
        snprintf(who, sizeof(who), "%s: %s", name, extra_name[x]);
        for (int q = 0; q < n_wr; ++q)
            if (wr[q] == extra[x]) return fail(SPC_ERR_INVALID_ARGUMENT, "%s is the same array as another output", who);
        for (int q = 0; q < n_in; ++q)
            if (in[q] == extra[x]) return fail(SPC_ERR_INVALID_ARGUMENT, "%s is also an input (it is written while they are read)", who);
        wr[n_wr++] = extra[x];
    }
    for (int q = 0; q < n_in; ++q) bits |= (uintptr_t)in[q];
    for (int q = 0; q < n_wr; ++q) bits |= (uintptr_t)wr[q];
    if (bits % sizeof(T)) return fail(SPC_ERR_INVALID_ARGUMENT, "%s: a pointer is not aligned to its element type", name);
    const int C = col_cols(a->ktot, (int)sizeof(T), 1, 0);
    if (!C)
        return fail(SPC_ERR_UNSUPPORTED, "%s: ktot %lld above the %lld levels of which 16 columns fit the LDS", name, (long long)a->ktot,
                    (long long)col_max_ktot((int)sizeof(T), 1, 0));
    p.u = (const T *)a->u; p.v = (const T *)a->v; p.hx = (const T *)a->hx; p.hy = (const T *)a->hy;
    p.g = (const T *)a->g; p.r = (const T *)a->r; p.cmax = (T *)a->cmax; p.mtop = (T *)a->mtop;
    if constexpr (HAS_FTOP) p.ftop = (T *)ftop;
    p.itot = a->itot; p.jtot = a->jtot; p.ktot = a->ktot;
    p.nij = a->itot * a->jtot;
    p.ncols = a->n_les * (int64_t)p.nij;
    p.pitch_prof = a->pitch_prof;
    int64_t grid;
    if ((rc = col_grid(name, p.ncols, C, grid))) return rc;
    if (a->cmax && hipMemsetAsync(a->cmax, 0, (size_t)a->n_les * sizeof(T), (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SPC_ERR_LAUNCH, "%s: cmax could not be zeroed", name);
    }
    p.cols = C;
    return SPC_OK;
}

// one workgroup of VAD_THREADS per p.cols columns, the tile of col_pitch(ktot, 0) elements per column in dynamic LDS
template <typename K, typename P> static int vad_family_launch(K kernel, const char *kernel_name, const P &p, void *stream)
{
    const size_t smem = (size_t)p.cols * col_pitch(p.ktot, 0) * sizeof(*p.u);
    const int rc = ensure_lds(kernel, smem, kernel_name);
    if (rc) return rc;
    const int64_t grid = (p.ncols + p.cols - 1) / p.cols;         // (checked against INT32_MAX by vad_family_args, before cmax is zeroed)
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(VAD_THREADS), smem, (hipStream_t)stream, p);
    return launch_status(kernel_name);
}

template <typename T> static int les_vadvect_impl(const spc_les_vadvect_args *a, void *stream)
{
    static_assert(SPC_VADVECT_MAX_FIELDS == VAD_MAXF, "include/spc.h and spc_vadvect.hpp disagree on the fields per launch");
    LesVadvectP<T> p = {};
    const int rc = vad_family_args<T>("les_vadvect", a, p, stream);
    if (rc || !p.cols) return rc;
    switch (a->n_fields) {
    case 0: return vad_family_launch(k_les_vadvect<T, 0>, "k_les_vadvect", p, stream);
    case 1: return vad_family_launch(k_les_vadvect<T, 1>, "k_les_vadvect", p, stream);
    case 2: return vad_family_launch(k_les_vadvect<T, 2>, "k_les_vadvect", p, stream);
    case 3: return vad_family_launch(k_les_vadvect<T, 3>, "k_les_vadvect", p, stream);
    case 4: return vad_family_launch(k_les_vadvect<T, 4>, "k_les_vadvect", p, stream);
    case 5: return vad_family_launch(k_les_vadvect<T, 5>, "k_les_vadvect", p, stream);
    default: return vad_family_launch(k_les_vadvect<T, 6>, "k_les_vadvect", p, stream);
    }
}

#endif
