// spc_hmix.hpp -- K26: one backward-Euler step of the HORIZONTAL mixing of the device-resident LES fields by each line's OWN eddy
// viscosity (K24's km, uncapped), in place, kernel and host side.  spc_hip.hip includes it twice, like spc_vmix.hpp: with the
// kernel among the device headers, and -- SPC_HMIX_HOST defined -- after spc_launch.hpp and the host side of spc_slab.hpp
// (slab_check_extents).
//
// Fields and km are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets.  The entry point is TWO launches
// of ONE kernel (Lie splitting): every line along i, then every line along j, which reads what the first wrote.  A line is
// periodic, so its system is a cyclic tridiagonal one; the last cell is condensed out (x = y + z x[n-1]) and the rest is a Thomas
// elimination with two right-hand sides.  The rule (include/spc.h) per line of n cells of field f, a = ax[f][l] (ay[f][l] in the
// second sweep), ip = (i + 1) mod n, in T, one rounding per operation, never an fma (the build has FP contraction off):
//   t[i] = km[i] + km[ip];   s[i] = t[i] > 0 ? t[i] : +0;   s[i] = s[i] < kh2[l] ? s[i] : kh2[l];   w[i] = a * s[i]
//   up[i] = w[i];   lo[i] = w[im];   b[i] = (1 + lo[i]) + up[i]
//   c[i] = (i == 0 ? lo[0] : +0) + (i == n-2 ? up[n-2] : +0)
//   p = 1 / b[0];                     q[0] = up[0] * p;   y[0] = x[0] * p;   z[0] = c[0] * p
//   p = 1 / (b[i] - lo[i] * q[i-1]);  q[i] = up[i] * p;   y[i] = (x[i] + lo[i] * y[i-1]) * p;   z[i] = (c[i] + lo[i] * z[i-1]) * p
//   y[i] = y[i] + q[i] * y[i+1];      z[i] = z[i] + q[i] * z[i+1]                                  i = n-3 ... 0
//   num = (x[n-1] + up[n-1] * y[0]) + lo[n-1] * y[n-2];   den = (b[n-1] - up[n-1] * z[0]) - lo[n-1] * z[n-2]
//   x'[n-1] = num / den;              x'[i] = y[i] + z[i] * x'[n-1]
// Shape: the lines of a sweep are numbered g = 0 ... n_les * itot * jtot * ktot / n - 1 so that `inner` consecutive lines are
// contiguous in memory (inner = jtot * ktot along i, ktot along j): line g starts at (g / inner) * (n * inner) + g % inner and
// its cells are `inner` apart, which serves both sweeps.  ONE lane owns ONE line (l per lane: a workgroup may span several LES),
// consecutive lanes own consecutive lines, so every access of a wave is coalesced, and there is no barrier.  A lane walks its line
// three times: forward (km and x read, y written INTO THE FIELD, q and z into LDS), backward (y rewritten, z in LDS), and once
// more for x'.  Only q and z need storage of their own: 2 (n - 1) elements per line in LDS, [cell][lane] so that a wave's accesses
// fall into distinct banks; a workgroup takes hline_lines(n, sizeof(T)) lines.  The division chain is serial; the loads of a
// chunk of HLINE_U cells go out together before its arithmetic, since an in-place store keeps the compiler from hoisting them.
// The field is the blockIdx.y job: every field of a launch repeats the elimination of its class so that no pivot travels
// through memory.  Per field and sweep: km read once, the field read and written three times each (7 passes; the second and the
// third walk find their lines in L2).
#ifndef SPC_HMIX_HOST

constexpr int HLINE_MAXF = 6;
constexpr int HLINE_U = 8;                      // cells per chunk of a walk

template <typename T> struct LesHlineP {
    T *field[HLINE_MAXF];
    const T *a[HLINE_MAXF];        // ax[f] in the sweep along i, ay[f] in the sweep along j
    const T *km, *kh2;
    int64_t nlines;                // the lines of the sweep
    int64_t per_les;               // ... of one LES
    int64_t inner;                 // contiguous lines, and the distance of two cells of a line
    int32_t n;                     // cells of a line, >= 2
};

// the weight of the face between two cells of km ka and kn
template <typename T> __device__ __forceinline__ T hline_face(const T ka, const T kn, const T a, const T cap)
{
    const T t = ka + kn;
    const T s = t > (T)0 ? t : (T)0;                                 // a NaN or a negative sum gives +0
    const T sc = s < cap ? s : cap;
    return a * sc;
}

// lines per workgroup for lines of n cells of esize bytes: as many as the 64 KiB default holds of q and z, 256 at the most; long
// lines take 32 or 16 lines of the whole LDS; 0: unsupported
inline int hline_lines(int n, int esize)
{
    if (n < 1 || (esize != 4 && esize != 8)) return 0;
    const int64_t line = 2 * (int64_t)(n > 1 ? n - 1 : 1) * esize;
    for (int L = 256; L >= 64; L >>= 1)
        if (L * line <= MAX_LDS_BYTES) return L;
    if (32 * line <= HARD_LDS_BYTES) return 32;
    if (16 * line <= HARD_LDS_BYTES) return 16;
    return 0;
}

// grid (ceil(nlines / L), n_fields), max(L, 64) threads; dynamic LDS: 2 * (n - 1) * L elements
template <typename T, int L> __global__ __launch_bounds__(L < 64 ? 64 : L) void k_les_hline(const LesHlineP<T> p)
{
    extern __shared__ __align__(16) unsigned char hline_lds[];
    const int lane = threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x * L + lane;
    if (lane >= L || g >= p.nlines) return;                          // the last workgroup is partial; the kernel has no barrier
    const int f = blockIdx.y;
    const int n = p.n, m = n - 1;                                    // m unknowns are condensed on cell m
    const int64_t st = p.inner;
    const int64_t outer = g / st;
    const int64_t base = outer * (st * n) + (g - outer * st);
    const int64_t l = g / p.per_les;                                 // per lane: a workgroup may span several LES
    T *x = p.field[f] + base;
    const T *km = p.km + base;
    const T a = p.a[f][l], cap = p.kh2[l];
    T *q = reinterpret_cast<T *>(hline_lds) + lane;                  // q[i] at q[i * L], z[i] at z[i * L]
    T *z = q + m * L;
    // cell 0
    const T k0 = km[0], kl = km[m * st];
    const T wl = hline_face<T>(kl, k0, a, cap);                      // the face between n-1 and 0: lo[0] and up[n-1]
    T kc = km[st];
    T up = hline_face<T>(k0, kc, a, cap);
    T qv, yv, zv;
    {
        const T b1 = (T)1 + wl;
        const T b = b1 + up;
        const T c = wl + (m == 1 ? up : (T)0);
        const T pv = (T)1 / b;
        qv = up * pv;
        yv = x[0] * pv;
        zv = c * pv;
        q[0] = qv;
        z[0] = zv;
        x[0] = yv;
    }
    T lo = up;
    // cells 1 ... n-2; lo = w[i-1], kc = km[i], qv, yv, zv those of cell i-1
    for (int i = 1; i < m; i += HLINE_U) {
        T cx[HLINE_U], ck[HLINE_U];
#pragma unroll
        for (int u = 0; u < HLINE_U; ++u)
            if (i + u < m) { cx[u] = x[(i + u) * st]; ck[u] = km[(i + u + 1) * st]; }
#pragma unroll
        for (int u = 0; u < HLINE_U; ++u)
            if (i + u < m) {
                up = hline_face<T>(kc, ck[u], a, cap);
                const T b1 = (T)1 + lo;
                const T b = b1 + up;
                const T c = (T)0 + (i + u == m - 1 ? up : (T)0);
                const T lq = lo * qv;
                const T piv = b - lq;
                const T pv = (T)1 / piv;
                qv = up * pv;
                const T ly = lo * yv;
                const T ry = cx[u] + ly;
                yv = ry * pv;
                const T lz = lo * zv;
                const T rz = c + lz;
                zv = rz * pv;
                q[(i + u) * L] = qv;
                z[(i + u) * L] = zv;
                x[(i + u) * st] = yv;
                lo = up;
                kc = ck[u];
            }
    }
    // lo = w[n-2] = lo[n-1]; the back substitution of both right-hand sides leaves cell n-2 as it is
    const T yl = yv, zl = zv;
    for (int i = m - 2; i >= 0; i -= HLINE_U) {
        T cy[HLINE_U], cq[HLINE_U], cz[HLINE_U];
#pragma unroll
        for (int u = 0; u < HLINE_U; ++u)
            if (i - u >= 0) { cy[u] = x[(i - u) * st]; cq[u] = q[(i - u) * L]; cz[u] = z[(i - u) * L]; }
#pragma unroll
        for (int u = 0; u < HLINE_U; ++u)
            if (i - u >= 0) {
                const T ty = cq[u] * yv;
                yv = cy[u] + ty;
                const T tz = cq[u] * zv;
                zv = cz[u] + tz;
                x[(i - u) * st] = yv;
                z[(i - u) * L] = zv;
            }
    }
    // yv = y[0], zv = z[0]: the condensed cell
    const T xl = x[m * st];
    const T b1 = (T)1 + lo;
    const T bl = b1 + wl;
    const T n1 = wl * yv;
    const T n2 = xl + n1;
    const T n3 = lo * yl;
    const T num = n2 + n3;
    const T d1 = wl * zv;
    const T d2 = bl - d1;
    const T d3 = lo * zl;
    const T den = d2 - d3;
    const T xn = num / den;                                          // correctly rounded
    x[m * st] = xn;
    for (int i = 0; i < m; i += HLINE_U) {
        T cy[HLINE_U], cz[HLINE_U];
#pragma unroll
        for (int u = 0; u < HLINE_U; ++u)
            if (i + u < m) { cy[u] = x[(i + u) * st]; cz[u] = z[(i + u) * L]; }
#pragma unroll
        for (int u = 0; u < HLINE_U; ++u)
            if (i + u < m) {
                const T t = cz[u] * xn;
                x[(i + u) * st] = cy[u] + t;
            }
    }
}

#else  // SPC_HMIX_HOST ------------------------------------------------------------------------------------------------------

template <typename F> static int hline_dispatch(int L, F f)
{
    switch (L) {
    case 256: return f(std::integral_constant<int, 256>());
    case 128: return f(std::integral_constant<int, 128>());
    case 64: return f(std::integral_constant<int, 64>());
    case 32: return f(std::integral_constant<int, 32>());
    }
    return f(std::integral_constant<int, 16>());
}

template <typename T> static int les_hmix_impl(const spc_les_hmix_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_hmix", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    static_assert(SPC_HMIX_MAX_FIELDS == HLINE_MAXF, "include/spc.h and spc_hmix.hpp disagree on the fields per launch");
    if (a->n_fields < 1 || a->n_fields > SPC_HMIX_MAX_FIELDS)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_hmix: field count %lld outside 1 ... %lld", "", (long long)a->n_fields, (long long)SPC_HMIX_MAX_FIELDS);
    if (a->axes < 1 || a->axes > 3)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_hmix: axes %lld outside 1 ... 3 (bit 0: along i, bit 1: along j)", "", (long long)a->axes);
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->km, "km"); REQUIRE(a->kh2, "kh2");
    LesHlineP<T> p = {};
    uintptr_t bits = (uintptr_t)a->km | (uintptr_t)a->kh2;
    // (equal base pointers are what is detected, as in K25: partially overlapping views are the caller's to avoid)
    for (int f = 0; f < a->n_fields; ++f) {
        REQUIRE(a->fields[f], "fields[f]"); REQUIRE(a->ax[f], "ax[f]"); REQUIRE(a->ay[f], "ay[f]");
        const void *const x = a->fields[f];
        for (int g = 0; g < f; ++g)
            if (a->fields[g] == x)
                return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_hmix: fields[%lld] and fields[%lld] are the same field", "", (long long)g, (long long)f);
        bool read = x == a->km || x == a->kh2;
        for (int g = 0; g < a->n_fields; ++g) read = read || x == a->ax[g] || x == a->ay[g];
        if (read)
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_hmix: fields[%lld] is also km, kh2 or a coefficient (it is written while they are read)", "", (long long)f);
        p.field[f] = (T *)x;
        bits |= (uintptr_t)x | (uintptr_t)a->ax[f] | (uintptr_t)a->ay[f];
    }
    if (bits % sizeof(T)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_hmix: a pointer is not aligned to its element type");
    const int32_t ext[2] = {a->itot, a->jtot};
    int64_t grids[2] = {0, 0};
    const int64_t cells = (int64_t)a->itot * a->jtot * a->ktot;
    for (int axis = 0; axis < 2; ++axis) {                           // both sweeps are checked before the first is launched
        if (!(a->axes >> axis & 1) || ext[axis] == 1) continue;      // a line of one cell keeps every bit
        const int L = hline_lines(ext[axis], (int)sizeof(T));
        if (!L) {
            int top = ext[axis];
            while (!hline_lines(top, (int)sizeof(T))) --top;
            return fail(SPC_ERR_UNSUPPORTED, "les_hmix: %s %lld above the %lld cells of a line of which 16 fit the LDS", axis ? "jtot" : "itot",
                        (long long)ext[axis], (long long)top);
        }
        grids[axis] = (a->n_les * (cells / ext[axis]) + L - 1) / L;
        if (grids[axis] > INT32_MAX) return fail(SPC_ERR_UNSUPPORTED, "%sles_hmix: too many workgroups");
    }
    p.km = (const T *)a->km; p.kh2 = (const T *)a->kh2;
    for (int axis = 0; axis < 2; ++axis) {
        if (!grids[axis]) continue;
        p.n = ext[axis];
        p.per_les = cells / p.n;
        p.nlines = a->n_les * p.per_les;
        p.inner = axis ? a->ktot : (int64_t)a->jtot * a->ktot;
        for (int f = 0; f < a->n_fields; ++f) p.a[f] = (const T *)(axis ? a->ay[f] : a->ax[f]);
        const int L = hline_lines(p.n, (int)sizeof(T));
        const size_t smem = (size_t)2 * (p.n - 1) * L * sizeof(T);
        rc = hline_dispatch(L, [&](auto c) {
            constexpr int LL = decltype(c)::value;
            int e = ensure_lds(k_les_hline<T, LL>, smem, "k_les_hline");
            if (e) return e;
            hipLaunchKernelGGL((k_les_hline<T, LL>), dim3((unsigned)grids[axis], (unsigned)a->n_fields), dim3(LL < 64 ? 64 : LL), smem, (hipStream_t)stream, p);
            return launch_status("k_les_hline");
        });
        if (rc) return rc;
    }
    return SPC_OK;
}

#endif
