// spc_qtlocal.hpp -- K19: the local cloud-water forcing of the LES moisture (qt_forcing == 'local' | 'strong'), kernels and host
// side.  spc_hip.hip includes it twice, like spc_radiate.hpp: with the kernels among the device headers, and --
// SPC_QTLOCAL_HOST defined -- after spc_launch.hpp and the host side of spc_slab.hpp (slab_check_extents).
//
// The reference hands every LES the cloud-water forcing and the GCM's cloud-water profile (splib/spcpl.py:346-347) and lets
// DALES act on them (Dales.QT_FORCING_LOCAL / QT_FORCING_STRONG, splib/modfac.py:70-73).  DALES's source is not part of the
// reference, so the rule below is THIS library's definition (include/spc.h), shaped on what the coupler passes in
// and on the option's help text ("stimulate ql alignment with ... local forcing").
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  Per (l, k), in T, one
// rounding per operation, never an fma (the build has FP contraction off); a = A[l][k], m = QTM[l][k], N = itot * jtot:
//   a is +0, -0 or NaN:  the level keeps every bit of qt, count = 0
//   wet(cell) = a > 0 ? qt > m : ql > 0                     (a NaN compares false: dry)
//   c = the number of wet cells of the plane;  count[l][k] = c
//   c == 0 or c == N:    the level keeps every bit of qt
//   else  s = a * T(N);  dw = s / T(c);  dd = s / T(N - c);  qt' = wet ? qt + dw : qt - dd      IN PLACE
// A plane (l, k) is N cells that lie ktot elements apart, and its count must be whole before its first cell is written: the
// first kernel here with a per-plane reduction in front of its stores.  The count is an integer, so neither the order of the
// cells nor the cut of the launch can change a bit of the result.
//
// A workgroup of 256 lanes owns a TILE of TW adjacent levels of one LES: TK lanes run along k (V adjacent levels each) and
// RL = 256 / TK row-lanes share the N rows (i, j) of the tile, row-lane q taking the rows q, q + RL, ...
//   wide    V = 16 B / sizeof(T), TK = 16: one 16-byte access per lane, 256 contiguous bytes per row and 4 rows per wave
//           instruction; taken where qt, ql and ktot * sizeof(T) are multiples of 16 bytes (every row then starts on the grid)
//   narrow  V = 1, TK = 64: single elements, a wave reads 64 adjacent levels of one row; every other view and ktot
// (K18's head and tail do not carry over: the rows of a tile lie ktot elements apart, so where ktot * sizeof(T) is not a
// multiple of 16 every row has a head of its own.)
//   1. every lane reads a and m of its levels; a level with a zero or NaN a is skipped from here on: no load, no store
//   2. the row-lanes walk their rows, QTL_U rows of loads in flight ahead of the compares (qt where a > 0, ql where a < 0),
//      and count their wet cells in registers; the partial counts meet in TW words of LDS by integer atomics
//   3. count[l][k] is written; levels with c == 0 or c == N are skipped from here on
//   4. two divisions per lane and level, then the same walk again: qt (and ql where a < 0) re-read -- from L2 where the tile
//      fits --, the predicate re-evaluated on the value read, qt' stored (a whole vector where all V levels are touched)
// FUSED runs 1-4 in one launch.  Where n_les * ceil(ktot / 64) workgroups would leave most CUs idle (few LES with large planes)
// a plane is SPLIT over S workgroups that take ceil(N / S) consecutive rows each: count is zeroed on the stream, k_..<COUNT>
// runs 1-2 and adds its part into count[l][k] with an integer atomicAdd, k_..<APPLY> reads the whole count and runs 4.  The
// kernel boundary is the only ordering between workgroups.  No float atomics anywhere.
#ifndef SPC_QTLOCAL_HOST

constexpr int QTL_THREADS = 256;
constexpr int QTL_U = 4;                        // rows of loads in flight per lane
constexpr int QTL_FUSED = 0, QTL_COUNT = 1, QTL_APPLY = 2;
constexpr int64_t QTL_MAX_PLANE = (int64_t)1 << 24;     // T(N), T(c) and T(N - c) are exact in float

// the split factor the library chooses: 1 where the fused launch has at least 512 workgroups of nominal 64-level tiles, else as
// many parts as bring the launch to ~1 024 workgroups, each of at least 64 rows; 0: bad arguments
inline int qtl_split(int64_t n_les, int64_t itot, int64_t jtot, int64_t ktot, int esize)
{
    if (n_les < 1 || itot < 1 || jtot < 1 || ktot < 1 || (esize != 4 && esize != 8) || itot * jtot > QTL_MAX_PLANE) return 0;
    const int64_t N = itot * jtot, wgs = n_les * ((ktot + 63) / 64);
    if (wgs >= 512) return 1;
    const int64_t want = (1024 + wgs - 1) / wgs, most = N / 64;
    return (int)(want < most ? want : (most < 1 ? 1 : most));
}

template <typename T> struct LesQtLocalP {
    T *qt;
    const T *ql, *A, *QTM;
    int32_t *count;
    int64_t pitch_prof, pitch_count;
    int32_t nij, ktot;
    int32_t tiles;                 // ceil(ktot / TW)
    int32_t split, chunk;          // parts of a plane, rows per part
};

// grid n_les * tiles * split; block b: part = b % split, tile = (b / split) % tiles, l = b / (split * tiles)
template <typename T, int V, int TK, int MODE> __global__ __launch_bounds__(QTL_THREADS) void k_les_qt_local(const LesQtLocalP<T> p)
{
    constexpr int RL = QTL_THREADS / TK, TW = TK * V;
    using Vec = SlabVec<T, V>;
    __shared__ int red[TW];
    const int tid = threadIdx.x, kl = tid % TK, rl = tid / TK;
    const int64_t b = blockIdx.x, bt = b / p.split;
    const int part = (int)(b - bt * p.split);
    const int64_t l = bt / p.tiles;
    const int tile = (int)(bt - l * p.tiles);
    const int k0 = tile * TW + kl * V;                             // wide: ktot % V == 0, so a vector never leaves its row
    const int ktot = p.ktot, N = p.nij;
    const int r0 = part * p.chunk, r1 = min(N, r0 + p.chunk);
    const int64_t cell0 = l * (int64_t)N * ktot + k0;              // row 0 of the LES at the lane's first level
    // 1. a, m and the sign of a per level
    T a[V], m[V];
    int mode[V];                                                    // 0: untouched, 1: a > 0 (qt > m), 2: a < 0 (ql > 0)
    bool pos = false, neg = false;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        a[v] = m[v] = (T)0;
        if (k0 + v < ktot) {
            a[v] = p.A[l * p.pitch_prof + k0 + v];
            m[v] = p.QTM[l * p.pitch_prof + k0 + v];
        }
        mode[v] = a[v] > (T)0 ? 1 : (a[v] < (T)0 ? 2 : 0);          // +0, -0 and NaN: 0
        pos |= mode[v] == 1;
        neg |= mode[v] == 2;
    }
    int c[V];
    if (MODE != QTL_APPLY) {
        // 2. the wet cells of the lane's rows, then of the tile
        if (tid < TW) red[tid] = 0;
        __syncthreads();
        if (pos || neg) {
            int cnt[V];
#pragma unroll
            for (int v = 0; v < V; ++v) cnt[v] = 0;
            for (int r = r0 + rl; r < r1; r += RL * QTL_U) {
                Vec x[QTL_U] = {}, y[QTL_U] = {};
#pragma unroll
                for (int u = 0; u < QTL_U; ++u) {
                    const int rr = r + u * RL;
                    if (rr < r1) {
                        const int64_t e = cell0 + (int64_t)rr * ktot;
                        if (pos) x[u] = *reinterpret_cast<const Vec *>(p.qt + e);
                        if (neg) y[u] = *reinterpret_cast<const Vec *>(p.ql + e);
                    }
                }
#pragma unroll
                for (int u = 0; u < QTL_U; ++u)
                    if (r + u * RL < r1) {
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            const bool wet = mode[v] == 1 ? x[u].v[v] > m[v] : (mode[v] == 2 ? y[u].v[v] > (T)0 : false);
                            cnt[v] += wet ? 1 : 0;
                        }
                    }
            }
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (cnt[v]) atomicAdd(&red[kl * V + v], cnt[v]);
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < V; ++v) c[v] = red[kl * V + v];
        // 3. the count of the plane (FUSED), or this part's share of it (COUNT: the launch zeroed count first)
        if (rl == 0) {
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (k0 + v < ktot) {
                    int32_t *const q = p.count + l * p.pitch_count + k0 + v;
                    if (MODE == QTL_FUSED)
                        *q = c[v];
                    else if (c[v])
                        atomicAdd(q, c[v]);
                }
        }
        if (MODE == QTL_COUNT) return;
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) c[v] = (mode[v] && k0 + v < ktot) ? p.count[l * p.pitch_count + k0 + v] : 0;
    }
    // 4. the shares of the wet and of the dry cells, then the walk that applies them
    T dw[V], dd[V];
    bool act[V], any = false, all = true, need_ql = false;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        act[v] = mode[v] != 0 && c[v] > 0 && c[v] < N;
        dw[v] = dd[v] = (T)0;
        if (act[v]) {
            const T s = a[v] * (T)N;
            dw[v] = s / (T)c[v];                                    // two true IEEE quotients (spc_device.hpp: every quotient is)
            dd[v] = s / (T)(N - c[v]);
        }
        any |= act[v];
        all &= act[v];
        need_ql |= act[v] && mode[v] == 2;
    }
    if (!any) return;
    for (int r = r0 + rl; r < r1; r += RL * QTL_U) {
        Vec x[QTL_U] = {}, y[QTL_U] = {};
#pragma unroll
        for (int u = 0; u < QTL_U; ++u) {
            const int rr = r + u * RL;
            if (rr < r1) {
                const int64_t e = cell0 + (int64_t)rr * ktot;
                x[u] = *reinterpret_cast<const Vec *>(p.qt + e);
                if (need_ql) y[u] = *reinterpret_cast<const Vec *>(p.ql + e);
            }
        }
#pragma unroll
        for (int u = 0; u < QTL_U; ++u) {
            const int rr = r + u * RL;
            if (rr < r1) {
                T *const q = p.qt + cell0 + (int64_t)rr * ktot;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const T t = x[u].v[v];
                    const bool wet = mode[v] == 1 ? t > m[v] : y[u].v[v] > (T)0;
                    const T up = t + dw[v], dn = t - dd[v];
                    x[u].v[v] = act[v] ? (wet ? up : dn) : t;
                }
                if (all) {
                    *reinterpret_cast<Vec *>(q) = x[u];
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v)
                        if (act[v]) q[v] = x[u].v[v];               // an untouched level is never stored to
                }
            }
        }
    }
}

// count[l][0 ... ktot - 1] = 0 in front of a split launch (the words between pitched rows are not touched)
__global__ __launch_bounds__(QTL_THREADS) void k_les_qt_local_zero(int32_t *count, const int64_t pitch, const int32_t ktot, const int64_t total)
{
    const int64_t g = (int64_t)blockIdx.x * QTL_THREADS + threadIdx.x;
    if (g >= total) return;
    const int64_t l = g / ktot;
    count[l * pitch + (g - l * ktot)] = 0;
}

#else  // SPC_QTLOCAL_HOST ---------------------------------------------------------------------------------------------------

template <typename T, int V, int TK> static int les_qt_local_launch(LesQtLocalP<T> p, int64_t n_les, void *stream)
{
    constexpr int TW = TK * V;
    p.tiles = (p.ktot + TW - 1) / TW;
    const int64_t grid = n_les * p.tiles * p.split;
    if (grid > INT32_MAX) return fail(SPC_ERR_UNSUPPORTED, "%sles_qt_local: too many workgroups");
    if (p.split == 1) {
        hipLaunchKernelGGL((k_les_qt_local<T, V, TK, QTL_FUSED>), dim3((unsigned)grid), dim3(QTL_THREADS), 0, (hipStream_t)stream, p);
        return launch_status("k_les_qt_local");
    }
    const int64_t total = n_les * p.ktot;
    const int64_t zgrid = (total + QTL_THREADS - 1) / QTL_THREADS;
    if (zgrid > INT32_MAX) return fail(SPC_ERR_UNSUPPORTED, "%sles_qt_local: too many workgroups");
    hipLaunchKernelGGL(k_les_qt_local_zero, dim3((unsigned)zgrid), dim3(QTL_THREADS), 0, (hipStream_t)stream, p.count, p.pitch_count, p.ktot, total);
    int rc = launch_status("k_les_qt_local_zero");
    if (rc) return rc;
    hipLaunchKernelGGL((k_les_qt_local<T, V, TK, QTL_COUNT>), dim3((unsigned)grid), dim3(QTL_THREADS), 0, (hipStream_t)stream, p);
    if ((rc = launch_status("k_les_qt_local (count)"))) return rc;
    hipLaunchKernelGGL((k_les_qt_local<T, V, TK, QTL_APPLY>), dim3((unsigned)grid), dim3(QTL_THREADS), 0, (hipStream_t)stream, p);
    return launch_status("k_les_qt_local (apply)");
}

template <typename T> static int les_qt_local_impl(const spc_les_qt_local_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    if (a->itot >= 1 && a->jtot >= 1 && (int64_t)a->itot * a->jtot > QTL_MAX_PLANE)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_qt_local: more than 2^24 points per plane (their number is not exact in float)");
    int rc = slab_check_extents("les_qt_local", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    if (a->pitch_prof < a->ktot)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_qt_local: pitch_prof %lld smaller than ktot", "", (long long)a->pitch_prof);
    if (a->pitch_count < a->ktot)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_qt_local: pitch_count %lld smaller than ktot", "", (long long)a->pitch_count);
    if (a->split < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_qt_local: split = %lld < 0", "", (long long)a->split);
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->qt, "qt"); REQUIRE(a->ql, "ql"); REQUIRE(a->a, "a"); REQUIRE(a->qtm, "qtm"); REQUIRE(a->count, "count");
    if (a->qt == a->ql) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_qt_local: qt and ql are the same array (ql is read while qt is written)");
    if (((uintptr_t)a->qt | (uintptr_t)a->ql | (uintptr_t)a->a | (uintptr_t)a->qtm) % sizeof(T) || (uintptr_t)a->count % 4)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_qt_local: a pointer is not aligned to its element type");
    LesQtLocalP<T> p = {};
    p.qt = (T *)a->qt; p.ql = (const T *)a->ql; p.A = (const T *)a->a; p.QTM = (const T *)a->qtm; p.count = a->count;
    p.pitch_prof = a->pitch_prof; p.pitch_count = a->pitch_count;
    p.nij = a->itot * a->jtot; p.ktot = a->ktot;
    const int chosen = a->split ? a->split : qtl_split(a->n_les, a->itot, a->jtot, a->ktot, (int)sizeof(T));
    p.split = chosen < p.nij ? chosen : p.nij;                    // at most one part per row
    p.chunk = (p.nij + p.split - 1) / p.split;
    constexpr int VMAX = 16 / (int)sizeof(T);
    const bool wide = ((uintptr_t)a->qt | (uintptr_t)a->ql | (uintptr_t)((size_t)a->ktot * sizeof(T))) % 16 == 0;
    return wide ? les_qt_local_launch<T, VMAX, 16>(p, a->n_les, stream) : les_qt_local_launch<T, 1, 64>(p, a->n_les, stream);
}

#endif
