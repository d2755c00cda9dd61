// spc_mix.hpp -- K24: the Smagorinsky-Lilly subgrid closure of the device-resident LES fields, kernels and host side.  An eddy
// viscosity per cell from the resolved deformation and the stratification (k_les_eddy), and one explicit step in flux form of the
// horizontal mixing of the carried fields by that viscosity (k_les_hmix): two launches behind one entry point.  spc_hip.hip
// includes it twice, like spc_advect.hpp and spc_buoyancy.hpp: with the kernels among the device headers, and -- SPC_MIX_HOST
// defined -- after spc_launch.hpp and the host side of spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule
// (include/spc.h), in T, one rounding per operation, never an fma (the build has FP contraction off), no division, no
// transcendental function, one correctly rounded sqrt per cell (K20's); im / ip / jm / jp K16's periodic neighbours,
// kp = min(k + 1, ktot - 1), kq = max(k - 1, 0) (clamped BEFORE the load); gx, gy, kcap [n_les]; gz, bz, l2 [n_les x ktot]:
//   ux = (u[ip] - u[im]) * gx;   vx = (v[ip] - v[im]) * gx;   uy = (u[jp] - u[jm]) * gy;   vy = (v[jp] - v[jm]) * gy
//   uz = (u[kp] - u[kq]) * gz;   vz = (v[kp] - v[kq]) * gz
//   a  = ux * ux + vy * vy;   sh = uy + vx;   d = (a + a) + sh * sh;   d = d + (uz * uz + vz * vz)
//   d  = d - (theta[kp] - theta[kq]) * bz                    where theta != NULL
//   e  = d > 0 ? d : +0;   kk = l2 * sqrt(e);   kmax[l] = max kk;   km = kk < kcap ? kk : kcap
// and per field x with ax, ay [n_les] of that field:
//   kw = km[im] + km;   ke = km + km[ip];   ks = km[jm] + km;   kn = km + km[jp]
//   fw = (kw * ax) * (x - x[im]);   fe = (ke * ax) * (x[ip] - x);   fs = (ks * ay) * (x - x[jm]);   fn = (kn * ay) * (x[jp] - x)
//   out = x + ((fe - fw) + (fn - fs))
// Both kernels have K16's shape (spc_advect.hpp: advect_strip, advect_rows): a workgroup owns ADVECT_THREADS consecutive cells
// q = j * ktot + k of the contiguous run of a row i and walks `rows` consecutive rows with a three-row register window per array
// (u and v in k_les_eddy; km and every field in k_les_hmix), so each element is fetched once for the i direction and rows i0 - 1
// and i1 (wrapped) once more per workgroup.  j - 1 / j + 1 are ktot cells away in the same run (wrapped), k - 1 / k + 1 the
// adjacent cells of the run, clamped by k = q % ktot: ONE integer remainder per lane for the whole walk, and the profiles gz,
// bz, l2 of a lane are loaded once, since its k never changes.  Those neighbours are other lanes' own cells of the same row,
// fetched at the same time: they come from the L1 / L2.  HBM traffic: k_les_eddy reads u, v, theta and writes km (4 passes),
// k_les_hmix reads km and NF fields and writes NF outputs (1 + 2 NF).  NF is a template argument: the windows stay in
// registers (VGPR counts: DESIGN.md 7.3; no instantiation uses scratch).  kmax: kk is never NaN and never negative (l2 > 0
// finite is the caller's duty), so the order of the bit patterns is the order of the values: every lane keeps its maximum, a
// wave reduces by shuffles and its first lane issues one atomicMax (K16's); the launcher zeroes kmax first.
#ifndef SPC_MIX_HOST

constexpr int MIX_MAXF = 6;

template <typename T> struct LesMixP {
    const T *u, *v, *theta;        // theta or nullptr
    const T *gx, *gy, *kcap;
    const T *gz, *bz, *l2;         // bz or nullptr (only without theta)
    T *km;
    T *kmax;                       // or nullptr
    const T *field[MIX_MAXF];
    T *out[MIX_MAXF];
    const T *ax[MIX_MAXF], *ay[MIX_MAXF];
    int64_t pitch_prof;
    int64_t row;                   // jtot * ktot: cells of one row i
    int32_t itot, jtot, ktot;
    int32_t nchunk, nseg;          // workgroups along the flat run and along i
    int32_t rows;                  // rows i per workgroup
};

// grid nchunk * nseg * n_les (the chunk fastest: neighbouring workgroups share their j - 1 / j + 1 cells)
template <typename T, bool TH> __global__ __launch_bounds__(ADVECT_THREADS) void k_les_eddy(const LesMixP<T> p)
{
    const int64_t b = blockIdx.x;
    const int chunk = (int)(b % p.nchunk);
    const int seg = (int)((b / p.nchunk) % p.nseg);
    const int64_t l = b / ((int64_t)p.nchunk * p.nseg);
    const int itot = p.itot, ktot = p.ktot;
    const int64_t row = p.row;
    const int64_t q = (int64_t)chunk * ADVECT_THREADS + threadIdx.x;
    T top = (T)0;
    if (q < row) {
        int64_t qs = q - ktot;                                       // j - 1
        if (qs < 0) qs += row;
        int64_t qn = q + ktot;                                       // j + 1
        if (qn >= row) qn -= row;
        const int k = (int)(q % ktot);
        const int64_t qu = k + 1 < ktot ? q + 1 : q;                 // kp: clamped before the load
        const int64_t qd = k > 0 ? q - 1 : q;                        // kq
        const T gx = p.gx[l], gy = p.gy[l], kcap = p.kcap[l];
        const int64_t po = l * p.pitch_prof + k;
        const T gz = p.gz[po], l2 = p.l2[po];
        const T bz = TH ? p.bz[po] : (T)0;
        const int i0 = seg * p.rows;
        const int i1 = i0 + p.rows < itot ? i0 + p.rows : itot;
        const int64_t les = l * itot * row;
        const int64_t bw = les + (int64_t)(i0 ? i0 - 1 : itot - 1) * row;
        int64_t bi = les + (int64_t)i0 * row;
        T uw = p.u[bw + q], uc = p.u[bi + q];
        T vw = p.v[bw + q], vc = p.v[bi + q];
        for (int i = i0; i < i1; ++i) {
            const int ip = i + 1 == itot ? 0 : i + 1;
            const int64_t be = les + (int64_t)ip * row;
            const T ue = p.u[be + q], ve = p.v[be + q];
            const T us = p.u[bi + qs], un = p.u[bi + qn], ud = p.u[bi + qd], uu = p.u[bi + qu];
            const T vs = p.v[bi + qs], vn = p.v[bi + qn], vd = p.v[bi + qd], vu = p.v[bi + qu];
            T td = (T)0, tu = (T)0;
            if (TH) { td = p.theta[bi + qd]; tu = p.theta[bi + qu]; }
            const T dux = ue - uw, dvx = ve - vw, duy = un - us, dvy = vn - vs, duz = uu - ud, dvz = vu - vd;
            const T ux = dux * gx, vx = dvx * gx;
            const T uy = duy * gy, vy = dvy * gy;
            const T uz = duz * gz, vz = dvz * gz;
            const T uxx = ux * ux, vyy = vy * vy;
            const T a = uxx + vyy;
            const T sh = uy + vx;
            const T a2 = a + a, sh2 = sh * sh;
            T d = a2 + sh2;
            const T uzz = uz * uz, vzz = vz * vz;
            const T z = uzz + vzz;
            d = d + z;
            if (TH) {
                const T dt = tu - td;
                const T n2 = dt * bz;
                d = d - n2;
            }
            const T e = d > (T)0 ? d : (T)0;                         // a NaN gives +0
            const T r = sqrt(e);                                     // correctly rounded
            const T kk = l2 * r;
            top = kk > top ? kk : top;
            p.km[bi + q] = kk < kcap ? kk : kcap;
            uw = uc; uc = ue;
            vw = vc; vc = ve;
            bi = be;
        }
    }
    if (p.kmax) {
        using U = typename AdvectBits<T>::type;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const T o = __shfl_xor(top, d, 64);
            top = o > top ? o : top;
        }
        if ((threadIdx.x & 63) == 0) {
            U bits;
            __builtin_memcpy(&bits, &top, sizeof(T));
            if (bits) atomicMax(reinterpret_cast<U *>(p.kmax) + l, bits);
        }
    }
}

// grid as k_les_eddy
template <typename T, int NF> __global__ __launch_bounds__(ADVECT_THREADS) void k_les_hmix(const LesMixP<T> p)
{
    const int64_t b = blockIdx.x;
    const int chunk = (int)(b % p.nchunk);
    const int seg = (int)((b / p.nchunk) % p.nseg);
    const int64_t l = b / ((int64_t)p.nchunk * p.nseg);
    const int itot = p.itot, ktot = p.ktot;
    const int64_t row = p.row;
    const int64_t q = (int64_t)chunk * ADVECT_THREADS + threadIdx.x;
    if (q >= row) return;
    int64_t qs = q - ktot;                                           // j - 1
    if (qs < 0) qs += row;
    int64_t qn = q + ktot;                                           // j + 1
    if (qn >= row) qn -= row;
    const int i0 = seg * p.rows;
    const int i1 = i0 + p.rows < itot ? i0 + p.rows : itot;
    const int64_t les = l * itot * row;
    const int64_t bw = les + (int64_t)(i0 ? i0 - 1 : itot - 1) * row;
    int64_t bi = les + (int64_t)i0 * row;
    T mw = p.km[bw + q], mc = p.km[bi + q];
    T xw[NF], xc[NF], ax[NF], ay[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        xw[f] = p.field[f][bw + q];
        xc[f] = p.field[f][bi + q];
        ax[f] = p.ax[f][l];
        ay[f] = p.ay[f][l];
    }
    for (int i = i0; i < i1; ++i) {
        const int ip = i + 1 == itot ? 0 : i + 1;
        const int64_t be = les + (int64_t)ip * row;
        const T me = p.km[be + q], ms = p.km[bi + qs], mn = p.km[bi + qn];
        T xe[NF], xs[NF], xn[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) { xe[f] = p.field[f][be + q]; xs[f] = p.field[f][bi + qs]; xn[f] = p.field[f][bi + qn]; }
        const T kw = mw + mc, ke = mc + me, ks = ms + mc, kn = mc + mn;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const T x = xc[f];
            const T cw = kw * ax[f], ce = ke * ax[f], cs = ks * ay[f], cn = kn * ay[f];
            const T dw = x - xw[f], de = xe[f] - x, ds = x - xs[f], dn = xn[f] - x;
            const T fw = cw * dw, fe = ce * de, fs = cs * ds, fn = cn * dn;
            const T hx = fe - fw, hy = fn - fs;
            const T h = hx + hy;
            p.out[f][bi + q] = x + h;
            xw[f] = x;
            xc[f] = xe[f];
        }
        mw = mc;
        mc = me;
        bi = be;
    }
}

#else  // SPC_MIX_HOST -------------------------------------------------------------------------------------------------------

template <typename T, int NF> static int les_hmix_launch(const LesMixP<T> &p, int64_t grid, void *stream)
{
    hipLaunchKernelGGL((k_les_hmix<T, NF>), dim3((unsigned)grid), dim3(ADVECT_THREADS), 0, (hipStream_t)stream, p);
    return launch_status("k_les_hmix");
}

template <typename T> static int les_mix_impl(const spc_les_mix_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_mix", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    static_assert(SPC_MIX_MAX_FIELDS == MIX_MAXF, "include/spc.h and spc_mix.hpp disagree on the fields per launch");
    if (a->pitch_prof < a->ktot)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_mix: pitch_prof %lld smaller than ktot", "", (long long)a->pitch_prof);
    if (a->n_fields < 0 || a->n_fields > SPC_MIX_MAX_FIELDS)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_mix: field count %lld outside 0 ... %lld", "", (long long)a->n_fields, (long long)SPC_MIX_MAX_FIELDS);
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->u, "u"); REQUIRE(a->v, "v"); REQUIRE(a->gx, "gx"); REQUIRE(a->gy, "gy"); REQUIRE(a->kcap, "kcap");
    REQUIRE(a->gz, "gz"); REQUIRE(a->l2, "l2"); REQUIRE(a->km, "km");
    if (a->theta && !a->bz) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_mix: theta without bz");
    const int nf = a->n_fields;
    for (int f = 0; f < nf; ++f) {
        REQUIRE(a->fields[f], "fields[f]"); REQUIRE(a->out[f], "out[f]"); REQUIRE(a->ax[f], "ax[f]"); REQUIRE(a->ay[f], "ay[f]");
    }
    // (equal base pointers are what is detected, as in K16 and K21: partially overlapping views are the caller's to avoid)
    const void *in[9 + 3 * MIX_MAXF] = {a->u, a->v, a->theta, a->gx, a->gy, a->kcap, a->gz, a->theta ? a->bz : nullptr, a->l2};
    const void *wr[2 + MIX_MAXF] = {a->km, a->kmax};
    int nin = 9, nwr = 2;
    for (int f = 0; f < nf; ++f) {
        in[nin++] = a->fields[f]; in[nin++] = a->ax[f]; in[nin++] = a->ay[f];
        wr[nwr++] = a->out[f];
    }
    uintptr_t bits = 0;
    for (int x = 0; x < nwr; ++x) {
        if (!wr[x]) continue;
        const char *const name = x == 0 ? "km" : x == 1 ? "kmax" : "an out[f]";
        for (int q = 0; q < nin; ++q)
            if (in[q] && in[q] == wr[x]) return fail(SPC_ERR_INVALID_ARGUMENT, "les_mix: %s is also an input (it is written while they are read)", name);
        for (int q = 0; q < x; ++q)
            if (wr[q] == wr[x]) return fail(SPC_ERR_INVALID_ARGUMENT, "les_mix: %s is the same array as another output", name);
        bits |= (uintptr_t)wr[x];
    }
    for (int q = 0; q < nin; ++q) bits |= (uintptr_t)in[q];
    if (bits % sizeof(T)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_mix: a pointer is not aligned to its element type");
    LesMixP<T> p = {};
    p.u = (const T *)a->u; p.v = (const T *)a->v; p.theta = (const T *)a->theta;
    p.gx = (const T *)a->gx; p.gy = (const T *)a->gy; p.kcap = (const T *)a->kcap;
    p.gz = (const T *)a->gz; p.bz = (const T *)a->bz; p.l2 = (const T *)a->l2;
    p.km = (T *)a->km; p.kmax = (T *)a->kmax;
    for (int f = 0; f < nf; ++f) {
        p.field[f] = (const T *)a->fields[f]; p.out[f] = (T *)a->out[f];
        p.ax[f] = (const T *)a->ax[f]; p.ay[f] = (const T *)a->ay[f];
    }
    p.pitch_prof = a->pitch_prof;
    p.itot = a->itot; p.jtot = a->jtot; p.ktot = a->ktot;
    p.row = (int64_t)a->jtot * a->ktot;
    p.rows = advect_rows(a->n_les, a->itot, a->jtot, a->ktot);
    const int64_t nchunk = (p.row + ADVECT_THREADS - 1) / ADVECT_THREADS, nseg = (a->itot + p.rows - 1) / p.rows;
    if (nchunk > INT32_MAX || (double)nchunk * (double)nseg * (double)a->n_les > (double)INT32_MAX)
        return fail(SPC_ERR_UNSUPPORTED, "%sles_mix: too many workgroups");
    p.nchunk = (int32_t)nchunk; p.nseg = (int32_t)nseg;
    const int64_t grid = nchunk * nseg * a->n_les;
    if (a->kmax && hipMemsetAsync(a->kmax, 0, (size_t)a->n_les * sizeof(T), (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SPC_ERR_LAUNCH, "%sles_mix: kmax could not be zeroed");
    }
    void (*const eddy)(const LesMixP<T>) = a->theta ? k_les_eddy<T, true> : k_les_eddy<T, false>;
    hipLaunchKernelGGL(eddy, dim3((unsigned)grid), dim3(ADVECT_THREADS), 0, (hipStream_t)stream, p);
    if ((rc = launch_status("k_les_eddy"))) return rc;
    switch (nf) {
    case 0: return SPC_OK;
    case 1: return les_hmix_launch<T, 1>(p, grid, stream);
    case 2: return les_hmix_launch<T, 2>(p, grid, stream);
    case 3: return les_hmix_launch<T, 3>(p, grid, stream);
    case 4: return les_hmix_launch<T, 4>(p, grid, stream);
    case 5: return les_hmix_launch<T, 5>(p, grid, stream);
    default: return les_hmix_launch<T, 6>(p, grid, stream);
    }
}

#endif
