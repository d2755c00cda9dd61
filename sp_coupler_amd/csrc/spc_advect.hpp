// spc_advect.hpp -- K16: one explicit first-order upwind step of the horizontal advection of the device-resident LES fields on
// a doubly periodic plane, kernel and host side.  spc_hip.hip includes it twice, like spc_diffuse.hpp: with the kernel among
// the device headers, and -- SPC_ADVECT_HOST defined -- after spc_launch.hpp and the host side of spc_slab.hpp
// (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule
// (include/spc.h) per cell (l, i, j, k), in T, one rounding per operation, never an fma (the build has FP contraction off), no
// division, im / ip / jm / jp the periodic neighbours:
//   cw = (u[im][j] + u[i][j]) * hx[l];   ce = (u[i][j] + u[ip][j]) * hx[l]
//   cs = (v[i][jm] + v[i][j]) * hy[l];   cn = (v[i][j] + v[i][jp]) * hy[l]
//   pw = cw > 0 ? cw : 0;   pe = ce < 0 ? -ce : 0;   ps = cs > 0 ? cs : 0;   pn = cn < 0 ? -cn : 0
//   x' = (((x + pw * (x[im][j] - x)) + pe * (x[ip][j] - x)) + ps * (x[i][jm] - x)) + pn * (x[i][jp] - x)
//   s  = ((pw + pe) + ps) + pn;   cmax[l] = max over the cells of LES l of s
// The shape is the first of this project with neighbours across the two non-contiguous axes.  One row i of one LES is a
// contiguous run of jtot * ktot cells, and j - 1 / j + 1 are ktot cells before / behind a cell IN THAT RUN (wrapped at its
// ends), so the (j, k) plane is walked FLAT: a workgroup owns ADVECT_THREADS consecutive cells q = j * ktot + k of the run --
// every access of a wave is one contiguous stretch whatever ktot is, no lane idles at a ktot that is no multiple of 64, and a
// view off the 16-byte grid takes the same path -- and `rows` consecutive rows i: ADVECT_ROWS_MANY where that still leaves
// ADVECT_MANY_WGS workgroups, else ADVECT_ROWS_FEW (advect_rows; measured: DESIGN.md 7.3).  A lane walks its rows with a register
// window per array (the values at i - 1, i, i + 1 of u and of every field): each element is fetched once for the i direction,
// and rows i0 - 1 and i1 (wrapped) once more per workgroup, 2 / rows of the reads.  The j - 1 and j + 1 values of v and of
// the fields are loaded from the same row ktot cells away: other lanes of the workgroup or of its neighbours on the same row
// fetch them as their own cells at the same time, so they come from the L1 / L2 and not from HBM a second time.  The face
// numbers pw, pe, ps, pn of a cell are formed once and used by all NF fields (a template argument: the windows stay in
// registers).  The outputs are separate buffers written whole, so no workgroup waits for another.  cmax: every lane keeps the
// maximum of its s, a wave reduces by shuffles and its first lane issues one atomicMax on the unsigned bit pattern (s is never
// NaN and never negative: the order of the patterns is the order of the values); the launcher zeroes cmax first.
#ifndef SPC_ADVECT_HOST

constexpr int ADVECT_THREADS = 256;                // consecutive cells of the flat (j, k) run of a row per workgroup
constexpr int ADVECT_ROWS_FEW = 8;                 // consecutive rows i per workgroup of a launch of few workgroups
constexpr int ADVECT_ROWS_MANY = 32;               // ... of a launch that has ADVECT_MANY_WGS workgroups even so
constexpr int ADVECT_MANY_WGS = 1024;
constexpr int ADVECT_MAXF = 6;

template <typename T> struct LesAdvectP {
    const T *u, *v;
    const T *field[ADVECT_MAXF];
    T *out[ADVECT_MAXF];
    const T *hx, *hy;
    T *cmax;                       // or nullptr
    int64_t row;                   // jtot * ktot: cells of one row i
    int32_t itot, jtot, ktot;
    int32_t nchunk, nseg;          // workgroups along the flat run and along i
    int32_t rows;                  // rows i per workgroup
};

template <typename T> struct AdvectBits;
template <> struct AdvectBits<double> { using type = unsigned long long; };
template <> struct AdvectBits<float> { using type = unsigned int; };

// grid nchunk * nseg * n_les (the chunk fastest: neighbouring workgroups share their j - 1 / j + 1 cells)
template <typename T, int NF> __global__ __launch_bounds__(ADVECT_THREADS) void k_les_advect(const LesAdvectP<T> p)
{
    const int64_t b = blockIdx.x;
    const int chunk = (int)(b % p.nchunk);
    const int seg = (int)((b / p.nchunk) % p.nseg);
    const int64_t l = b / ((int64_t)p.nchunk * p.nseg);
    const int itot = p.itot, ktot = p.ktot;
    const int64_t row = p.row;
    const int64_t q = (int64_t)chunk * ADVECT_THREADS + threadIdx.x;
    T smax = (T)0;
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
        T uw = p.u[bw + q], uc = p.u[bi + q];
        T xw[NF ? NF : 1], xc[NF ? NF : 1];
#pragma unroll
        for (int f = 0; f < NF; ++f) { xw[f] = p.field[f][bw + q]; xc[f] = p.field[f][bi + q]; }
        for (int i = i0; i < i1; ++i) {
            const int ip = i + 1 == itot ? 0 : i + 1;
            const int64_t be = les + (int64_t)ip * row;
            const T ue = p.u[be + q];
            const T vc = p.v[bi + q], vs = p.v[bi + qs], vn = p.v[bi + qn];
            T xe[NF ? NF : 1], xs[NF ? NF : 1], xn[NF ? NF : 1];
#pragma unroll
            for (int f = 0; f < NF; ++f) { xe[f] = p.field[f][be + q]; xs[f] = p.field[f][bi + qs]; xn[f] = p.field[f][bi + qn]; }
            const T aw = uw + uc, ae = uc + ue, as = vs + vc, an = vc + vn;
            const T cw = aw * hx;
            const T ce = ae * hx;
            const T cs = as * hy;
            const T cn = an * hy;
            const T pw = cw > (T)0 ? cw : (T)0;
            const T pe = ce < (T)0 ? -ce : (T)0;
            const T ps = cs > (T)0 ? cs : (T)0;
            const T pn = cn < (T)0 ? -cn : (T)0;
            T s = pw + pe;
            s = s + ps;
            s = s + pn;
            smax = s > smax ? s : smax;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const T x = xc[f];
                const T dw = xw[f] - x, de = xe[f] - x, ds = xs[f] - x, dn = xn[f] - x;
                const T tw = pw * dw, te = pe * de, ts = ps * ds, tn = pn * dn;
                T r = x + tw;
                r = r + te;
                r = r + ts;
                r = r + tn;
                p.out[f][bi + q] = r;
                xw[f] = x;
                xc[f] = xe[f];
            }
            uw = uc;
            uc = ue;
            bi = be;
        }
    }
    if (p.cmax) {
        using U = typename AdvectBits<T>::type;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const T o = __shfl_xor(smax, d, 64);
            smax = o > smax ? o : smax;
        }
        if ((threadIdx.x & 63) == 0) {
            U bits;
            __builtin_memcpy(&bits, &smax, sizeof(T));
            if (bits) atomicMax(reinterpret_cast<U *>(p.cmax) + l, bits);
        }
    }
}

// cells of the flat (j, k) run of a row that one workgroup owns, 0: bad arguments
inline int advect_strip(int jtot, int ktot, int esize) { return jtot < 1 || ktot < 1 || (esize != 4 && esize != 8) ? 0 : ADVECT_THREADS; }

// rows i that one workgroup walks, 0: bad arguments
inline int advect_rows(int64_t n_les, int itot, int jtot, int ktot)
{
    if (n_les < 0 || itot < 1 || jtot < 1 || ktot < 1) return 0;
    const double nchunk = (double)(((int64_t)jtot * ktot + ADVECT_THREADS - 1) / ADVECT_THREADS);
    const double wgs = nchunk * (double)((itot + ADVECT_ROWS_MANY - 1) / ADVECT_ROWS_MANY) * (double)n_les;
    return wgs >= (double)ADVECT_MANY_WGS ? ADVECT_ROWS_MANY : ADVECT_ROWS_FEW;
}

#else  // SPC_ADVECT_HOST ----------------------------------------------------------------------------------------------------

template <typename T, int NF> static int les_advect_launch(const LesAdvectP<T> &p, int64_t grid, void *stream)
{
    hipLaunchKernelGGL((k_les_advect<T, NF>), dim3((unsigned)grid), dim3(ADVECT_THREADS), 0, (hipStream_t)stream, p);
    return launch_status("k_les_advect");
}

template <typename T> static int les_advect_impl(const spc_les_advect_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_advect", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    static_assert(SPC_ADVECT_MAX_FIELDS == ADVECT_MAXF, "include/spc.h and spc_advect.hpp disagree on the fields per launch");
    if (a->n_fields < 0 || a->n_fields > SPC_ADVECT_MAX_FIELDS)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advect: field count %lld outside 0 ... %lld", "", (long long)a->n_fields, SPC_ADVECT_MAX_FIELDS);
    if (a->n_fields == 0 && !a->cmax)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advect: no field and no cmax: nothing to do");
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->u, "u"); REQUIRE(a->v, "v"); REQUIRE(a->hx, "hx"); REQUIRE(a->hy, "hy");
    LesAdvectP<T> p = {};
    uintptr_t bits = (uintptr_t)a->u | (uintptr_t)a->v | (uintptr_t)a->hx | (uintptr_t)a->hy | (uintptr_t)a->cmax;
    if (a->cmax && (a->cmax == a->u || a->cmax == a->v || a->cmax == a->hx || a->cmax == a->hy))
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advect: cmax is also an input (it is written while they are read)");
    // (equal base pointers are what is detected, as in K11, K14 and K15: partially overlapping views are the caller's to avoid)
    for (int f = 0; f < a->n_fields; ++f) {
        REQUIRE(a->fields[f], "fields[f]");
        REQUIRE(a->out[f], "out[f]");
        if (a->fields[f] == a->cmax)
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advect: cmax is also an input (it is written while they are read)");
        for (int g = 0; g < f; ++g)
            if (a->out[g] == a->out[f])
                return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advect: out[%lld] and out[%lld] are the same array", "", g, f);
        bool in = a->out[f] == a->u || a->out[f] == a->v || a->out[f] == a->hx || a->out[f] == a->hy || a->out[f] == a->cmax;
        for (int g = 0; g < a->n_fields; ++g) in = in || a->out[f] == a->fields[g];
        if (in)
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advect: out[%lld] is also an input or cmax (every cell reads its neighbours' old values)", "", f);
        p.field[f] = (const T *)a->fields[f];
        p.out[f] = (T *)a->out[f];
        bits |= (uintptr_t)a->fields[f] | (uintptr_t)a->out[f];
    }
    if (bits % sizeof(T)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_advect: a pointer is not aligned to its element type");
    p.u = (const T *)a->u; p.v = (const T *)a->v; p.hx = (const T *)a->hx; p.hy = (const T *)a->hy; p.cmax = (T *)a->cmax;
    p.itot = a->itot; p.jtot = a->jtot; p.ktot = a->ktot;
    p.row = (int64_t)a->jtot * a->ktot;
    p.rows = advect_rows(a->n_les, a->itot, a->jtot, a->ktot);
    const int64_t nchunk = (p.row + ADVECT_THREADS - 1) / ADVECT_THREADS, nseg = (a->itot + p.rows - 1) / p.rows;
    if (nchunk > INT32_MAX || (double)nchunk * (double)nseg * (double)a->n_les > (double)INT32_MAX)
        return fail(SPC_ERR_UNSUPPORTED, "%sles_advect: too many workgroups");
    p.nchunk = (int32_t)nchunk; p.nseg = (int32_t)nseg;
    const int64_t grid = nchunk * nseg * a->n_les;
    if (a->cmax && hipMemsetAsync(a->cmax, 0, (size_t)a->n_les * sizeof(T), (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SPC_ERR_LAUNCH, "%sles_advect: cmax could not be zeroed");
    }
    switch (a->n_fields) {
    case 0: return les_advect_launch<T, 0>(p, grid, stream);
    case 1: return les_advect_launch<T, 1>(p, grid, stream);
    case 2: return les_advect_launch<T, 2>(p, grid, stream);
    case 3: return les_advect_launch<T, 3>(p, grid, stream);
    case 4: return les_advect_launch<T, 4>(p, grid, stream);
    case 5: return les_advect_launch<T, 5>(p, grid, stream);
    default: return les_advect_launch<T, 6>(p, grid, stream);
    }
}

#endif
