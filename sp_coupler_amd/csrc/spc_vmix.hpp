// spc_vmix.hpp -- K25: one backward-Euler step of the vertical mixing of the device-resident LES fields by each column's OWN eddy
// viscosity (K24's km), with the kinematic surface fluxes of K15 and a neutral bulk drag on the lowest wind level, kernels and
// host side.  spc_hip.hip includes it twice, like spc_diffuse.hpp: with the kernels among the device headers (after
// spc_diffuse.hpp, whose DIF_U and DIF_UB it reuses), and -- SPC_VMIX_HOST defined -- after spc_launch.hpp and the host
// side of spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The matrix of the step
// depends on the column, so -- unlike K15 -- the Thomas elimination runs in the kernel: ONE correctly rounded IEEE division per
// level, and ONE correctly rounded sqrt per column (the wind speed of the drag).  The rule (include/spc.h) per column (l, i, j)
// of field f, in T, one rounding per operation, never an fma (the build has FP contraction off):
//   sp    = sqrt(u[0] * u[0] + v[0] * v[0])                                      k_les_speed, only where some dr[f] != NULL
//   t     = (km[k-1] + km[k]) + kb[l][k];   s[k] = t > 0 ? t : +0;   s[k] = s[k] < kv2[l] ? s[k] : kv2[l]      face k = 1 ... ktot-1
//   lo[k] = el[f][l][k] * s[k]  (lo[0] = +0);   up[k] = eu[f][l][k] * s[k+1]  (up[ktot-1] = +0)
//   b[k]  = (1 + lo[k]) + up[k];   b[0] = b[0] + dr[f][l] * sp
//   d[0]  = flux[f] ? x[0] + s0[l] * flux[f][l] : x[0];   d[k] = x[k]
//   m[0]  = 1 / b[0];   q[0] = up[0] * m[0];   y[0] = d[0] * m[0]
//   m[k]  = 1 / (b[k] - lo[k] * q[k-1]);   q[k] = up[k] * m[k];   y[k] = (d[k] + lo[k] * y[k-1]) * m[k]
//   x'[ktot-1] = y[ktot-1];   x'[k] = y[k] + q[k] * x'[k+1]
// The winds are updated in place by other workgroups, so the speed of the drag is not read from u and v during the solve: the
// entry point is TWO launches, as K21's and K24's.  k_les_speed (one lane per column) writes sp whole into the caller's plane
// speed [n_les][itot][jtot]; then k_les_vmix runs.
// k_les_vmix is the column tile of spc_coltile.hpp with (tiles, faces) = (2, 0), one field per blockIdx.y: the km run and the
// field run are copied into the two tiles (col_move), and lane c < C eliminates column c: in the forward sweep q[k] overwrites
// km[k] once km[k+1] is in a register, and y overwrites x; the back substitution reads both.  l is per lane: a tile may span
// several LES.  el, eu and kb do not depend on the chain: the reads of chunk j + 1 (8 levels, 4 in f64) are issued before the
// arithmetic of chunk j, as are the LDS reads of x and km; where a tile spans at most DIF_STAGE LES and the LDS budget has room,
// their rows are staged in LDS behind the tiles (K15's staging).  Every field of a launch repeats the elimination of its class (the
// division runs in lanes that would otherwise idle) so that no pivot travels through memory.  At 160 levels: 32 columns of f32,
// 16 of f64.
#ifndef SPC_VMIX_HOST

constexpr int VMIX_MAXF = 6;
constexpr int VMIX_THREADS = 256;
constexpr int VMIX_U64 = 4;                     // levels per chunk of a sweep in f64: three workgroups per CU need at most 168 VGPRs

template <typename T> struct LesVmixP {
    T *field[VMIX_MAXF];
    const T *flux[VMIX_MAXF], *dr[VMIX_MAXF], *el[VMIX_MAXF], *eu[VMIX_MAXF];
    const T *km, *kb, *kv2, *s0;
    const T *u, *v;
    T *speed;
    int64_t ncols;                 // n_les * itot * jtot
    int64_t pitch_prof;
    int32_t nij, ktot;
    int32_t stage;                 // DIF_STAGE where the rows fit the LDS budget behind the tiles, else 0
};

// grid ceil(ncols / VMIX_THREADS): the speed of the lowest level of every column
template <typename T> __global__ __launch_bounds__(VMIX_THREADS) void k_les_speed(const LesVmixP<T> p)
{
    const int64_t c = (int64_t)blockIdx.x * VMIX_THREADS + threadIdx.x;
    if (c >= p.ncols) return;
    const T u = p.u[c * p.ktot], v = p.v[c * p.ktot];
    const T uu = u * u, vv = v * v;
    const T e = uu + vv;
    p.speed[c] = sqrt(e);                                            // correctly rounded
}

// twice the diffusivity of the face between two cells of km ka (below) and kn (above)
template <typename T> __device__ __forceinline__ T vmix_face(const T ka, const T kn, const T bg, const T cap)
{
    const T h = ka + kn;
    const T t = h + bg;
    const T s = t > (T)0 ? t : (T)0;                                 // a NaN or a negative sum gives +0
    return s < cap ? s : cap;
}

// the elimination and both sweeps of one column in LDS; x: the field, kq: km on entry, q afterwards; el, eu, kb: the rows of the
// column's LES; d: d[0]; drag: dr * sp where DRAG
template <typename T, bool DRAG>
__device__ __forceinline__ void vmix_column(T *x, T *kq, const T *el, const T *eu, const T *kb, const T cap, const T d, const T drag, const int ktot)
{
    constexpr int U = sizeof(T) == 8 ? VMIX_U64 : DIF_U;             // levels per chunk of a sweep
    T kc = kq[0], slo = (T)0, up = (T)0;
    if (ktot > 1) {
        const T kn = kq[1];
        slo = vmix_face<T>(kc, kn, kb[1], cap);
        up = eu[0] * slo;
        kc = kn;
    }
    T b = (T)1 + up;                                                 // (1 + lo[0]) + up[0] with lo[0] = +0
    if (DRAG) b = b + drag;
    T m = (T)1 / b;
    T q = up * m, y = d * m;
    kq[0] = q;
    x[0] = y;
    // level k, slo = s[k], kc = km[k], q = q[k - 1], y = y[k - 1]; the levels below the lid have a face above
    int k = 1;
    const int top = ktot - 1;
    if (k + U <= top) {
        T ce[U], cu[U], cb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { ce[u] = el[k + u]; cu[u] = eu[k + u]; cb[u] = kb[k + 1 + u]; }
        for (; k + U <= top; k += U) {
            const bool more = k + 2 * U <= top;                  // another whole chunk follows: its loads go out first
            T ne[U], nu[U], nb[U], cx[U], ck[U];
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u) { ne[u] = el[k + U + u]; nu[u] = eu[k + U + u]; nb[u] = kb[k + U + 1 + u]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) { cx[u] = x[k + u]; ck[u] = kq[k + 1 + u]; }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const T sup = vmix_face<T>(kc, ck[u], cb[u], cap);
                const T lo = ce[u] * slo;
                up = cu[u] * sup;
                const T b1 = (T)1 + lo;
                const T bk = b1 + up;
                const T lq = lo * q;
                const T den = bk - lq;
                m = (T)1 / den;
                q = up * m;
                const T ly = lo * y;
                const T r = cx[u] + ly;
                y = r * m;
                kq[k + u] = q;
                x[k + u] = y;
                slo = sup;
                kc = ck[u];
            }
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u) { ce[u] = ne[u]; cu[u] = nu[u]; cb[u] = nb[u]; }
            }
        }
    }
    for (; k < top; ++k) {
        const T kn = kq[k + 1];
        const T sup = vmix_face<T>(kc, kn, kb[k + 1], cap);
        const T lo = el[k] * slo;
        up = eu[k] * sup;
        const T b1 = (T)1 + lo;
        const T bk = b1 + up;
        const T lq = lo * q;
        const T den = bk - lq;
        m = (T)1 / den;
        q = up * m;
        const T ly = lo * y;
        const T r = x[k] + ly;
        y = r * m;
        kq[k] = q;
        x[k] = y;
        slo = sup;
        kc = kn;
    }
    if (top > 0) {                                                   // the lid: up = +0, and q[top] is never read
        const T lo = el[top] * slo;
        const T bk = (T)1 + lo;                                      // (1 + lo) + (+0)
        const T lq = lo * q;
        const T den = bk - lq;
        m = (T)1 / den;
        const T ly = lo * y;
        const T r = x[top] + ly;
        y = r * m;
        x[top] = y;
    }
    // back substitution: y holds x'[ktot - 1]
    k = ktot - 2;
    for (; k - U + 1 >= 0; k -= U) {
        T cx[U], cq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { cx[u] = x[k - u]; cq[u] = kq[k - u]; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const T t = cq[u] * y;
            y = cx[u] + t;
            x[k - u] = y;
        }
    }
    for (; k >= 0; --k) {
        const T t = kq[k] * y;
        y = x[k] + t;
        x[k] = y;
    }
}

// grid (ceil(ncols / C), n_fields); dynamic LDS: 2 * C * col_pitch(ktot, 0) elements, and 3 * DIF_STAGE * ktot more where p.stage
template <typename T, int C> __global__ __launch_bounds__(VMIX_THREADS, 3) void k_les_vmix(const LesVmixP<T> p)
{
    extern __shared__ __align__(16) unsigned char vmix_lds[];
    const int f = blockIdx.y;
    const int ktot = p.ktot, P = col_pitch(ktot, 0);
    T *xt = reinterpret_cast<T *>(vmix_lds);
    T *kt = xt + C * P;
    const int64_t col0 = (int64_t)blockIdx.x * C;
    const int64_t left = p.ncols - col0;
    const int nc = left < C ? (int)left : C;                         // the last tile is partial
    T *run = p.field[f] + col0 * ktot;
    col_move<T, VMIX_THREADS, DIF_UB, false>(run, xt, nc * ktot, ktot, P);
    col_move<T, VMIX_THREADS, DIF_UB, false>(const_cast<T *>(p.km) + col0 * ktot, kt, nc * ktot, ktot, P);      // a load: km is not written
    // the rows of el, eu and kb of the tile's LES, [3][DIF_STAGE][ktot] behind the tiles, where the tile spans at most p.stage LES
    const int64_t l0 = col0 / p.nij;
    const int nl = (int)((col0 + nc - 1) / p.nij - l0) + 1;
    const bool staged = nl <= p.stage;                               // the same for every lane of the workgroup
    T *prof = kt + C * P;
    if (staged) {
        for (int e = threadIdx.x; e < 3 * nl * ktot; e += VMIX_THREADS) {
            const int r = e / ktot, k = e - r * ktot;
            const int which = r / nl, dl = r - which * nl;
            const T *src = which == 0 ? p.el[f] : (which == 1 ? p.eu[f] : p.kb);
            prof[(which * DIF_STAGE + dl) * ktot + k] = src[(l0 + dl) * p.pitch_prof + k];
        }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < nc) {
        const int64_t l = (col0 + c) / p.nij;                        // per lane: a tile may span several LES
        const int64_t o = l * p.pitch_prof;
        T *x = xt + c * P;
        T d = x[0];
        const T *flux = p.flux[f];
        if (flux) {
            const T t = p.s0[l] * flux[l];
            d = d + t;
        }
        const T cap = p.kv2[l];
        const T *el = p.el[f] + o, *eu = p.eu[f] + o, *kb = p.kb + o;
        if (staged) {
            el = prof + (int)(l - l0) * ktot;
            eu = el + DIF_STAGE * ktot;
            kb = el + 2 * DIF_STAGE * ktot;
        }
        const T *dr = p.dr[f];
        if (dr) {
            const T drag = dr[l] * p.speed[col0 + c];
            vmix_column<T, true>(x, kt + c * P, el, eu, kb, cap, d, drag, ktot);
        } else {
            vmix_column<T, false>(x, kt + c * P, el, eu, kb, cap, d, (T)0, ktot);
        }
    }
    __syncthreads();
    col_move<T, VMIX_THREADS, DIF_UB, true>(run, xt, nc * ktot, ktot, P);
}

#else  // SPC_VMIX_HOST ------------------------------------------------------------------------------------------------------

template <typename T> static int les_vmix_impl(const spc_les_vmix_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_vmix", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    static_assert(SPC_VMIX_MAX_FIELDS == VMIX_MAXF, "include/spc.h and spc_vmix.hpp disagree on the fields per launch");
    if (a->n_fields < 1 || a->n_fields > SPC_VMIX_MAX_FIELDS)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_vmix: field count %lld outside 1 ... %lld", "", (long long)a->n_fields, (long long)SPC_VMIX_MAX_FIELDS);
    if (a->pitch_prof < a->ktot)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_vmix: pitch_prof %lld smaller than ktot", "", (long long)a->pitch_prof);
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->km, "km"); REQUIRE(a->kb, "kb"); REQUIRE(a->kv2, "kv2");
    LesVmixP<T> p = {};
    uintptr_t bits = (uintptr_t)a->km | (uintptr_t)a->kb | (uintptr_t)a->kv2 | (uintptr_t)a->s0;
    bool drag = false;
    // (equal base pointers are what is detected, as in K15: partially overlapping views are the caller's to avoid)
    for (int f = 0; f < a->n_fields; ++f) {
        REQUIRE(a->fields[f], "fields[f]"); REQUIRE(a->el[f], "el[f]"); REQUIRE(a->eu[f], "eu[f]");
        const void *const x = a->fields[f];
        for (int g = 0; g < f; ++g)
            if (a->fields[g] == x)
                return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_vmix: fields[%lld] and fields[%lld] are the same field", "", (long long)g, (long long)f);
        bool read = x == a->km || x == a->speed || x == a->kb || x == a->kv2 || x == a->s0 || x == a->flux[f] || x == a->dr[f];
        for (int g = 0; g < a->n_fields; ++g) read = read || x == a->el[g] || x == a->eu[g] || x == a->flux[g] || x == a->dr[g];
        if (read)
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_vmix: fields[%lld] is also km, speed, a profile, s0, a drag or a flux (it is written while they are read)", "", (long long)f);
        if (a->flux[f] && !a->s0)
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_vmix: flux[%lld] without s0", "", (long long)f);
        if (a->dr[f] && !(a->u && a->v && a->speed))
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_vmix: dr[%lld] without u, v and speed", "", (long long)f);
        drag = drag || a->dr[f];
        p.field[f] = (T *)x;
        p.flux[f] = (const T *)a->flux[f]; p.dr[f] = (const T *)a->dr[f];
        p.el[f] = (const T *)a->el[f]; p.eu[f] = (const T *)a->eu[f];
        bits |= (uintptr_t)x | (uintptr_t)a->flux[f] | (uintptr_t)a->dr[f] | (uintptr_t)a->el[f] | (uintptr_t)a->eu[f];
    }
    if (drag) {
        // speed is written by the first launch while u and v are read, and read by the second while km and the profiles are
        bool read = a->speed == a->u || a->speed == a->v || a->speed == a->km || a->speed == a->kb || a->speed == a->kv2 || a->speed == a->s0;
        for (int g = 0; g < a->n_fields; ++g)
            read = read || a->speed == a->el[g] || a->speed == a->eu[g] || a->speed == a->flux[g] || a->speed == a->dr[g];
        if (read) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_vmix: speed is also an input (it is written while they are read)");
        bits |= (uintptr_t)a->u | (uintptr_t)a->v | (uintptr_t)a->speed;
    }
    if (bits % sizeof(T)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_vmix: a pointer is not aligned to its element type");
    const int C = col_cols(a->ktot, (int)sizeof(T), 2, 0);
    if (!C)
        return fail(SPC_ERR_UNSUPPORTED, "%sles_vmix: ktot %lld above the %lld levels of which 16 columns fit the LDS twice", "", (long long)a->ktot,
                    (long long)col_max_ktot((int)sizeof(T), 2, 0));
    p.km = (const T *)a->km; p.kb = (const T *)a->kb; p.kv2 = (const T *)a->kv2; p.s0 = (const T *)a->s0;
    p.u = (const T *)a->u; p.v = (const T *)a->v; p.speed = (T *)a->speed;
    p.nij = a->itot * a->jtot;
    p.ncols = a->n_les * (int64_t)p.nij;
    p.pitch_prof = a->pitch_prof;
    p.ktot = a->ktot;
    if (drag) {
        const int64_t grid = (p.ncols + VMIX_THREADS - 1) / VMIX_THREADS;
        if (grid > INT32_MAX) return fail(SPC_ERR_UNSUPPORTED, "%sles_vmix: too many workgroups");
        hipLaunchKernelGGL((k_les_speed<T>), dim3((unsigned)grid), dim3(VMIX_THREADS), 0, (hipStream_t)stream, p);
        if ((rc = launch_status("k_les_speed"))) return rc;
    }
    return col_dispatch(C, [&](auto c) {
        return col_stage_launch<T>(k_les_vmix<T, decltype(c)::value>, "k_les_vmix", "les_vmix", p, C, 2, a->n_fields, VMIX_THREADS, stream);
    });
}

#endif
