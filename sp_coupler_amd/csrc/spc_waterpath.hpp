// spc_waterpath.hpp -- K13: vertical reductions of the LES 3-D fields (column water paths, cloud top, cloud cover), kernels and
// host side.  spc_hip.hip includes it twice: with the kernels among the device headers, and -- SPC_WATERPATH_HOST defined --
// after spc_launch.hpp (fail, REQUIRE, cons_depth, launch_status) for the argument checks and launches.
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous (K10's layout); one field of one launch may exceed 4 GiB:
// every element offset below is 64-bit.
//
// k_les_water_paths   wp[f][l][i][j] = numpy.add.reduce(field_f[l, i, j, :] * w[l, :]), bit for bit: the product rounded on its
//                     own (never an fma), then the row of ktot products summed as ndarray.sum() sums a contiguous run -- 0 +
//                     pairwise blocks of <= 128 elements with eight accumulators, halves split at multiples of 8, the remainder
//                     of a block added in order, rows of fewer than 8 elements sequentially.  EIGHT LANES PER (l, i, j) ROW, as
//                     k_rms (spc_sputils.hpp): lane j of a row's group carries accumulator j of the current block, the eight
//                     are combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) by shuffles, the block's remainder and the tree of block
//                     sums run on every lane alike.  A wave reads eight adjacent rows, 64 contiguous bytes of each per load (f64).
//                     The fields of a launch are blockIdx.y: every field walks with the registers of one (an inner loop over the
//                     fields would carry WP_MAX_FIELDS accumulators and block sums through the tree); w[l] is a few hundred
//                     bytes that the groups of a workgroup share, so its second and later reads are cache hits.
//                     The recursion depth PD comes from ktot on the host (0: ktot <= 128; 1, 2, 3: up to 248 / 488 / 968).  PD =
//                     -1 (ktot up to 8192, one chunk of numpy's) walks the tree with an explicit stack as vn_npsum does; the stack
//                     is in LDS, one slot per lane and level, not in registers indexed at run time: no scratch memory.
// cloud outputs       the pass over field `cloud_field` also gives top[l][i][j] = the largest k with field > 0, else -1 (NaN and
//                     -0.0 are not cloudy: K10's rule), and the number of rows with top >= 0 per LES.  The count is summed with
//                     integer atomics IN cover[l] (a 4-byte word of the T slot; a wave whose eight rows lie in one LES adds once),
//                     zeroed by k_wp_cover_zero before and divided in place by k_wp_cover_finish after: exact in any order, no
//                     workspace, also when `top` itself is not asked for.
#ifndef SPC_WATERPATH_HOST

constexpr int WP_MAX_FIELDS = 4;
constexpr int WP_THREADS = 256;
constexpr int WP_ROWS = WP_THREADS / 8;     // rows per workgroup
constexpr int WP_MAXK = 8192;               // numpy's chunk: longer rows are refused
constexpr int WP_STACK = 8;                 // depth of the tree over <= 8192 elements: 7 (vn_npsum)

template <typename T> struct WaterPathP {
    const T *field[WP_MAX_FIELDS];
    T *out[WP_MAX_FIELDS];
    const T *w;
    int64_t pitch_w;
    int64_t rows;                  // n_les * itot * jtot
    int32_t nij, ktot;
    int32_t cloud_field;           // -1: none
    int32_t *top;                  // or NULL
    T *cover;                      // or NULL
    int64_t n_les;
};

// the 4-byte word of cover[l] that holds the count while it is being summed
template <typename T> __device__ __forceinline__ int *wp_count_word(T *cover, int64_t l) { return reinterpret_cast<int *>(cover + l); }

template <typename T> __global__ __launch_bounds__(WP_THREADS) void k_wp_cover_zero(const WaterPathP<T> p)
{
    const int64_t l = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (l < p.n_les) *wp_count_word(p.cover, l) = 0;
}

template <typename T> __global__ __launch_bounds__(WP_THREADS) void k_wp_cover_finish(const WaterPathP<T> p)
{
    const int64_t l = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (l >= p.n_les) return;
    const int c = *wp_count_word(p.cover, l);                    // read, then overwritten by this lane alone
    p.cover[l] = (T)c / (T)p.nij;
}

// one pairwise block [lo, lo + n), n <= 128, of the products a[k] * w[k] on the 8 lanes of a row's group (su_leaf8 with a
// product term); top: the largest k of the block with a[k] > 0 that THIS lane has seen, else unchanged (k only grows)
template <typename T> __device__ __forceinline__ T wp_leaf8(const T *a, const T *w, int lo, int n, int j, int &top)
{
    if (n < 8) {                                             // numpy: plain loop
        T res = T(0);
        for (int i = 0; i < n; ++i) {
            const T x = ldg(a + lo + i);
            res += x * ldg(w + lo + i);
            top = x > T(0) ? lo + i : top;
        }
        return res;
    }
    const int n8 = n - (n % 8);
    const T v0 = ldg(a + lo + j);
    T rj = v0 * ldg(w + lo + j);
    top = v0 > T(0) ? lo + j : top;
    int i = 8;
    for (; i + 24 < n8; i += 32) {                           // four loads of the field in flight per lane
        const int k = lo + i + j;
        const T x0 = ldg(a + k), x1 = ldg(a + k + 8), x2 = ldg(a + k + 16), x3 = ldg(a + k + 24);
        const T w0 = ldg(w + k), w1 = ldg(w + k + 8), w2 = ldg(w + k + 16), w3 = ldg(w + k + 24);
        rj += x0 * w0; rj += x1 * w1; rj += x2 * w2; rj += x3 * w3;
        top = x0 > T(0) ? k : top; top = x1 > T(0) ? k + 8 : top; top = x2 > T(0) ? k + 16 : top; top = x3 > T(0) ? k + 24 : top;
    }
    for (; i < n8; i += 8) {
        const int k = lo + i + j;
        const T x = ldg(a + k);
        rj += x * ldg(w + k);
        top = x > T(0) ? k : top;
    }
    // ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)): lane j ^ 1, then ^ 2, then ^ 4 (IEEE addition commutes)
    T s = rj + __shfl_xor(rj, 1);
    s = s + __shfl_xor(s, 2);
    s = s + __shfl_xor(s, 4);
    for (i = n8; i < n; ++i) {
        const T x = ldg(a + lo + i);
        s += x * ldg(w + lo + i);
        top = x > T(0) ? lo + i : top;
    }
    return s;
}

// numpy's pairwise recursion with its depth fixed at compile time (as su_pw8)
template <int D, typename T> __device__ __forceinline__ T wp_pw8(const T *a, const T *w, int lo, int n, int j, int &top)
{
    if constexpr (D == 0) {
        return wp_leaf8(a, w, lo, n, j, top);
    } else {
        if (n <= 128) return wp_leaf8(a, w, lo, n, j, top);
        int n2 = n / 2;
        n2 -= n2 % 8;
        const T left = wp_pw8<D - 1>(a, w, lo, n2, j, top);
        return left + wp_pw8<D - 1>(a, w, lo + n2, n - n2, j, top);
    }
}

// grid (ceil(rows / WP_ROWS), n_fields)
template <typename T, int PD> __global__ __launch_bounds__(WP_THREADS) void k_les_water_paths(const WaterPathP<T> p)
{
    const int64_t row = (int64_t)blockIdx.x * WP_ROWS + (threadIdx.x >> 3);
    const int j = threadIdx.x & 7, f = blockIdx.y, n = p.ktot;
    const bool live = row < p.rows;                          // dead groups walk along on row 0 (shuffles need every lane)
    const int64_t r = live ? row : 0;
    const int64_t l = r / p.nij;
    const T *const ar = p.field[f] + r * (int64_t)n;
    const T *const wr = p.w + l * p.pitch_w;
    int top = -1;
    T total = T(0);
    if constexpr (PD >= 0) {
        total += wp_pw8<PD>(ar, wr, 0, n, j, top);           // ndarray.sum(): 0.0 + the one chunk
    } else {
        // vn_npsum's walk, n <= 8192: the pending right halves (lo | n << 16) and left sums of this lane in LDS
        __shared__ T s_left[WP_STACK][WP_THREADS];
        __shared__ int s_right[WP_STACK][WP_THREADS];
        const int t = threadIdx.x;
        unsigned has_left = 0;
        int cur_lo = 0, cur_n = n, depth = 0;
        T v;
        for (;;) {
            while (cur_n > 128) {                            // descend into the left halves
                int n2 = cur_n / 2;
                n2 -= n2 % 8;
                s_right[depth][t] = (cur_lo + n2) | ((cur_n - n2) << 16);
                has_left &= ~(1u << depth);
                ++depth;
                cur_n = n2;
            }
            v = wp_leaf8(ar, wr, cur_lo, cur_n, j, top);
            while (depth > 0 && (has_left >> (depth - 1) & 1u)) { v = s_left[depth - 1][t] + v; --depth; }
            if (depth == 0) break;
            s_left[depth - 1][t] = v; has_left |= 1u << (depth - 1);
            const int rr = s_right[depth - 1][t];
            cur_lo = rr & 0xffff; cur_n = rr >> 16;
        }
        total += v;
    }
    if (live && j == 0) p.out[f][row] = total;
    if (f != p.cloud_field) return;                          // (uniform over the workgroup)
    top = max(top, __shfl_xor(top, 1));
    top = max(top, __shfl_xor(top, 2));
    top = max(top, __shfl_xor(top, 4));
    if (live && j == 0 && p.top) p.top[row] = top;
    if (p.cover) {
        const unsigned long long m = __ballot(live && j == 0 && top >= 0);
        const int lane = threadIdx.x & 63;
        // the first and the last row of the wave (lanes 0 and 56) live and in one LES -- then so is every row between them --
        // or the whole wave dead: one atomic for the wave, else one per cloudy row.  A dead group counts as LES -1 here (it
        // walks along on row 0, LES 0, which says nothing about the live rows in front of it)
        const int64_t lc = live ? l : -1;
        const int64_t l_first = __shfl(lc, 0), l_last = __shfl(lc, 56);
        if (l_first == l_last) {
            if (lane == 0 && m) atomicAdd(wp_count_word(p.cover, l), __popcll(m));
        } else if (live && j == 0 && top >= 0) {
            atomicAdd(wp_count_word(p.cover, l), 1);
        }
    }
}

#else  // SPC_WATERPATH_HOST -------------------------------------------------------------------------------------------------

template <typename T> static int water_paths_impl(const spc_water_path_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_water_paths", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    static_assert(SPC_WP_MAX_FIELDS == WP_MAX_FIELDS, "include/spc.h and spc_waterpath.hpp disagree on the fields per launch");
    if (a->n_fields < 1 || a->n_fields > SPC_WP_MAX_FIELDS)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_water_paths: field count %lld outside 1 ... %lld", "", (long long)a->n_fields, SPC_WP_MAX_FIELDS);
    if (a->cloud_field < -1 || a->cloud_field >= a->n_fields)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_water_paths: cloud_field %lld is neither -1 nor one of the %lld fields", "",
                    (long long)a->cloud_field, (long long)a->n_fields);
    if (a->pitch_w < a->ktot)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_water_paths: pitch_w %lld smaller than ktot %lld", "", (long long)a->pitch_w, a->ktot);
    if (a->ktot > WP_MAXK)
        return fail(SPC_ERR_UNSUPPORTED, "%sles_water_paths: ktot %lld > %lld (numpy sums longer rows in chunks)", "", (long long)a->ktot, WP_MAXK);
    if (a->n_les == 0) return SPC_OK;
    WaterPathP<T> p = {};
    const bool cloud = a->cloud_field >= 0;
    REQUIRE(a->w, "w");
    for (int f = 0; f < a->n_fields; ++f) {
        REQUIRE(a->fields[f], "fields[f]");
        REQUIRE(a->out[f], "out[f]");
        if ((uintptr_t)a->fields[f] % sizeof(T) || (uintptr_t)a->out[f] % sizeof(T))
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_water_paths: a pointer is not aligned to its element type");
        for (int g = 0; g < a->n_fields; ++g)
            if (a->out[f] == a->fields[g] || (g != f && a->out[f] == a->out[g]))
                return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_water_paths: an output is a field or another output");
        if (a->out[f] == a->w || (cloud && (a->out[f] == (void *)a->top || a->out[f] == a->cover)))
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_water_paths: an output is w, top or cover");
        p.field[f] = (const T *)a->fields[f];
        p.out[f] = (T *)a->out[f];
    }
    if ((uintptr_t)a->w % sizeof(T) || (cloud && ((uintptr_t)a->top % 4 || (uintptr_t)a->cover % sizeof(T))))
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_water_paths: a pointer is not aligned to its element type");
    p.w = (const T *)a->w; p.pitch_w = a->pitch_w;
    p.nij = a->itot * a->jtot; p.ktot = a->ktot; p.n_les = a->n_les;
    p.rows = a->n_les * (int64_t)p.nij;
    p.cloud_field = cloud && (a->top || a->cover) ? a->cloud_field : -1;
    if (p.cloud_field >= 0) {
        p.top = a->top; p.cover = (T *)a->cover;
        for (int f = 0; f < a->n_fields; ++f)
            if ((const void *)p.top == a->fields[f] || (const void *)p.cover == a->fields[f])
                return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_water_paths: top or cover is a field");
        if ((p.top && (const void *)p.top == a->w) || (p.cover && (const void *)p.cover == a->w) || (p.top && (void *)p.top == (void *)p.cover))
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_water_paths: top or cover is w, or both are one array");
    }
    const int64_t grid = (p.rows + WP_ROWS - 1) / WP_ROWS;
    if (grid > INT32_MAX) return fail(SPC_ERR_UNSUPPORTED, "%sles_water_paths: too many rows for one launch");
    const unsigned lgrid = (unsigned)((a->n_les + WP_THREADS - 1) / WP_THREADS);
    if (p.cover) {
        hipLaunchKernelGGL(k_wp_cover_zero<T>, dim3(lgrid), dim3(WP_THREADS), 0, (hipStream_t)stream, p);
        if ((rc = launch_status("k_wp_cover_zero"))) return rc;
    }
    // depth of numpy's recursion over one row (a single chunk up to 8192 elements); -1: explicit stack
    const int pd = a->ktot <= 128 ? 0 : (a->ktot <= 1024 ? cons_depth(a->ktot) : -1);
    void (*const kern)(const WaterPathP<T>) = pd == 0 ? k_les_water_paths<T, 0> : pd == 1 ? k_les_water_paths<T, 1>
                                            : pd == 2 ? k_les_water_paths<T, 2> : pd == 3 ? k_les_water_paths<T, 3> : k_les_water_paths<T, -1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid, (unsigned)a->n_fields), dim3(WP_THREADS), 0, (hipStream_t)stream, p);
    if ((rc = launch_status("k_les_water_paths"))) return rc;
    if (p.cover) {
        hipLaunchKernelGGL(k_wp_cover_finish<T>, dim3(lgrid), dim3(WP_THREADS), 0, (hipStream_t)stream, p);
        return launch_status("k_wp_cover_finish");
    }
    return SPC_OK;
}

#endif
