// spc_sputils_host.hpp -- argument checks and launches of the K7 operators (kernels: spc_sputils.hpp); included by
// spc_hip.hip after spc_launch.hpp (fail, REQUIRE, launch_status, floor_pow2, small_batch).
#pragma once

// ---- host side ----------------------------------------------------------------------------------
// Write-through stores for launches that leave <= 64 MiB behind.  (K1 / K3's small_batch() draws that line at the 32 MiB of
// the aggregate L2; measured on these operators -- profiles/r04_write_through_sweep.log -- write-through still wins at the
// 45.7 MB interp GCM->LES writes at 35 718 rows: 20.8 against 23.7 us, the dirty lines otherwise wait for the end-of-kernel
// release.)
inline int su_write_through(int64_t bytes_written) { return small_batch(bytes_written, 64); }

// ---- launch choice ---------------------------------------------------------------------------------------------
// As choose_fwd / choose_bwd of spc_launch.hpp: WHICH instantiation of a K7 kernel runs, with how many rows per workgroup, is
// decided in ONE function per operator (choose_exner ... choose_rms); the launcher and spc_sputils_describe_launch
// (include/spc.h) both call it, so a test can ask what a launch gets (tests/sputils_slabs.py).  A choose_* dereferences no
// data pointer and needs no device.  sl, pd: the template arguments as the tables below index them, i.e. of the
// instantiation that runs (the float twins have no unrolled depths).
struct SuChoice {
    int elem = 0, rb = 0, stage = 0, sl = -1, pd = -1, weighted = 0, wt = 1, p2 = 0;
    unsigned grid = 0;
    size_t smem = 0;
};

// (every check of a K7 launch runs in its choose_*, the pointer checks only for the launcher (`ptrs`); SU_EMPTY: nothing to launch)
constexpr int SU_EMPTY = 1;
#define SU_REQUIRE(ptrs, ptr, name) if (ptrs) REQUIRE(ptr, name)

// The kernels address with 32-bit BYTE offsets (su_at).  A slab of several rows stays below 2^32 bytes by su_pitch_ok and the
// cut in su_rows; a ONE-row launch is exempt from both (its pitch is never multiplied), so its row itself is bounded here:
// n elements of `bytes` each must stay below 2^32 bytes (2^29 doubles or int64 indices, 2^30 floats).
inline bool su_one_row_fits(int64_t n, size_t bytes) { return n * (int64_t)bytes < ((int64_t)1 << 32); }

template <typename T> int choose_exner(int64_t n, const void *p, const void *out, SuChoice *c, bool ptrs)
{
    if (n < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sexner: n < 0");
    if (n == 0) return SU_EMPTY;
    SU_REQUIRE(ptrs, p, "p"); SU_REQUIRE(ptrs, out, "out");
    const int64_t per = (int64_t)SU_THREADS * SU_EXNER_PER;
    if ((n + per - 1) / per > 0x7fffffff) return fail(SPC_ERR_UNSUPPORTED, "%sexner: more than 2^41 elements");
    c->elem = (int)sizeof(T); c->rb = 0; c->grid = (unsigned)((n + per - 1) / per); c->smem = 0;
    c->wt = su_write_through(n * (int64_t)sizeof(T));
    return SPC_OK;
}

template <typename T> int exner_impl(int64_t n, const void *p, void *out, int inverse, void *stream)
{
    SuChoice c;
    const int rc = choose_exner<T>(n, p, out, &c, true);
    if (rc) return rc == SU_EMPTY ? SPC_OK : rc;
    auto kern = c.wt ? k_exner<T, 1> : k_exner<T, 0>;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(SU_THREADS), 0, (hipStream_t)stream, n, (const T *)p, (T *)out, inverse);
    return launch_status("k_exner");
}

// Rows per workgroup (the slab): enough rows for ~`target` outputs per workgroup -- 4-5 per thread, the shape of K1's
// 8-column slabs -- within the LDS budget, but never so many that the grid drops under four workgroups per CU (small
// batches are latency-bound: more, smaller workgroups).
// `max_pitch`: the largest row pitch (elements) of the launch -- the kernels address a slab with 32-bit BYTE offsets r * pitch + i
// off uniform bases, so rb * max_pitch * 8 must stay below 2^32 whatever chose rb: rows
// padded to millions of elements get fewer rows per workgroup (round-4 advisor: the bound was a comment, not a check).
inline int su_rows(int64_t n_rows, int n_out, size_t lds_per_row, size_t lds_fixed, size_t esize, int *stage, int64_t max_pitch, int lds_kib = 16,
                   bool fit_rounds = true)
{
    const int target = 1100;
    const size_t cap = (size_t)lds_kib * 1024;
    int rb = n_out > 0 ? (target + n_out - 1) / n_out : 1;
    if (rb < 1) rb = 1;
    if (rb > 64) rb = 64;
    const int64_t most = n_rows / (4 * (int64_t)device_cus());   // >= 4 workgroups per CU (MI355X: 1024)
    if (rb > most) rb = most < 1 ? 1 : (int)most;
    while (rb > 1 && (lds_per_row * rb + lds_fixed) * esize > cap) --rb;      // 16 KiB: >= 8 workgroups per CU
    // every wave of a workgroup runs ceil(rb n_out / 256) rounds of the output loop, the last one partly idle: among the
    // slab heights within two rows of that choice take the one that wastes the fewest lane-rounds (91 -> 160 levels: 8 rows =
    // exactly 5 rounds instead of 7 rows = 4.4 rounds paid as 5; the operators are bound by VALU issue)
    if (fit_rounds && n_out > 0) {
        auto waste = [&](int c) { const int64_t o = (int64_t)c * n_out, rounds = (o + SU_THREADS - 1) / SU_THREADS; return (double)(rounds * SU_THREADS - o) / (double)(rounds * SU_THREADS); };
        int best = rb;
        for (int c = rb > 2 ? rb - 2 : 1; c <= rb + 2 && c <= 64; ++c) {
            if (c > most && c > 1) break;
            if ((lds_per_row * c + lds_fixed) * esize > cap && c > rb) break;
            if (waste(c) < waste(best) - 0.02) best = c;
        }
        rb = best;
    }
    while (rb > 1 && (int64_t)rb * max_pitch * 8 >= ((int64_t)1 << 32)) --rb;      // (8: the widest element; output rows of searchsorted are int64)
    *stage = (lds_per_row * rb + lds_fixed) * esize <= SU_MAX_LDS;
    return rb;
}

// the kernels address a slab with 32-bit element offsets r * pitch + i (r < 64 rows, 24-bit multiply): pitches stay below 2^24
// elements -- except for a ONE-row launch, whose row index is always 0: the pitch is never multiplied (sputils.interp /
// searchsorted on one long vector of 2^24 or more points; round-4 advisor)
inline bool su_pitch_ok(int64_t n_rows, std::initializer_list<int64_t> pitches)
{
    if (n_rows <= 1) return true;
    for (int64_t p : pitches) if (p >= ((int64_t)1 << 24)) return false;
    return true;
}
inline int64_t su_max(std::initializer_list<int64_t> v) { int64_t m = 0; for (int64_t x : v) if (x > m) m = x; return m; }

// template argument SL of the staged kernels for a row whose power-of-two floor is p2: log2 p2 + 1 where that depth is
// instantiated (rows of 64-127, 128-255, 256-511, 512-1023 entries: every level count of BASELINE.json's configs), else 0
// (the same descent with the trip count at run time)
inline int su_sl(int p2) { return p2 == 64 ? 7 : p2 == 128 ? 8 : p2 == 256 ? 9 : p2 == 512 ? 10 : 0; }

// (the unrolled depths exist for double; the float twin runs the run-time descent)
template <typename T, int WT> auto interp_kernel(int sl) -> void (*)(const SuInterpP)
{
    if constexpr (sizeof(T) == 8) {
        if (sl == 7) return k_interp<T, 7, WT>;
        if (sl == 8) return k_interp<T, 8, WT>;
        if (sl == 9) return k_interp<T, 9, WT>;
        if (sl == 10) return k_interp<T, 10, WT>;
    }
    return sl >= 0 ? k_interp<T, 0, WT> : k_interp<T, -1, WT>;
}

template <typename T, int WT> auto searchsorted_kernel(int sl) -> void (*)(const SuSearchP)
{
    if constexpr (sizeof(T) == 8) {
        if (sl == 7) return k_searchsorted<T, 7, WT>;
        if (sl == 8) return k_searchsorted<T, 8, WT>;
        if (sl == 9) return k_searchsorted<T, 9, WT>;
        if (sl == 10) return k_searchsorted<T, 10, WT>;
    }
    return sl >= 0 ? k_searchsorted<T, 0, WT> : k_searchsorted<T, -1, WT>;
}

// `ptrs`: the launcher's call (pointers required, in the order the checks always had); the description passes false
template <typename T> int choose_interp(const spc_interp_args *a, SuChoice *c, bool ptrs)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    if (a->n_rows < 0 || a->n_x < 0 || a->n_xp < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sinterp: negative extent");
    if (a->n_rows == 0 || a->n_x == 0) return SU_EMPTY;
    if (a->n_xp == 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sinterp: array of sample points is empty");   // numpy: ValueError
    // (in front of the pointer checks: a launch the offsets cannot address is refused whatever its pointers)
    if (a->n_rows == 1 && !su_one_row_fits(a->n_x, sizeof(T)))
        return fail(SPC_ERR_UNSUPPORTED, sizeof(T) == 8 ? "%sinterp: one row of 2^29 points or more (the kernels address with 32-bit byte offsets)"
                                                         : "%sinterp: one row of 2^30 points or more (the kernels address with 32-bit byte offsets)");
    SU_REQUIRE(ptrs, a->x, "x"); SU_REQUIRE(ptrs, a->xp, "xp"); SU_REQUIRE(ptrs, a->fp, "fp"); SU_REQUIRE(ptrs, a->out, "out");
    if ((a->pitch_x && a->pitch_x < a->n_x) || (a->pitch_xp && a->pitch_xp < a->n_xp) || a->pitch_fp < a->n_xp || a->pitch_out < a->n_x)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sinterp: a pitch is smaller than its row (only x and xp may be shared, pitch 0)");
    if (!su_pitch_ok(a->n_rows, {a->pitch_x, a->pitch_xp, a->pitch_fp, a->pitch_out})) return fail(SPC_ERR_UNSUPPORTED, "%sinterp: a row pitch of 2^24 elements or more");
    c->elem = (int)sizeof(T); c->p2 = floor_pow2(a->n_xp);
    const size_t xrow = 2 * (size_t)c->p2 + 2;            // su_pad(p2), a padded xp row in LDS (in size_t: tables of 2^30 entries)
    const size_t per_row = (size_t)a->n_xp + (a->pitch_xp ? xrow : 0), fixed = a->pitch_xp ? 0 : xrow;
    c->rb = su_rows(a->n_rows, a->n_x, per_row, fixed, sizeof(T), &c->stage, a->n_rows > 1 ? su_max({a->pitch_x, a->pitch_xp, a->pitch_fp, a->pitch_out}) : 0);
    if ((a->n_rows + c->rb - 1) / c->rb > 0x7fffffff) return fail(SPC_ERR_UNSUPPORTED, "%sinterp: too many rows for one launch");
    c->grid = (unsigned)((a->n_rows + c->rb - 1) / c->rb);
    c->smem = c->stage ? (per_row * c->rb + fixed) * sizeof(T) : 0;
    c->wt = su_write_through(a->n_rows * (int64_t)a->n_x * (int64_t)sizeof(T));
    c->sl = c->stage ? (sizeof(T) == 8 ? su_sl(c->p2) : 0) : -1;
    return SPC_OK;
}

template <typename T> int interp_impl(const spc_interp_args *a, void *stream)
{
    SuChoice c;
    const int rc = choose_interp<T>(a, &c, true);
    if (rc) return rc == SU_EMPTY ? SPC_OK : rc;
    SuInterpP q;
    q.n_rows = a->n_rows; q.pitch_x = a->pitch_x; q.pitch_xp = a->pitch_xp; q.pitch_fp = a->pitch_fp; q.pitch_out = a->pitch_out;
    q.n_x = a->n_x; q.n_xp = a->n_xp; q.p2 = c.p2; q.rb = c.rb;
    q.x = a->x; q.xp = a->xp; q.fp = a->fp; q.out = a->out;
    void (*kern)(const SuInterpP) = c.wt ? interp_kernel<T, 1>(c.sl) : interp_kernel<T, 0>(c.sl);
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(SU_THREADS), c.smem, (hipStream_t)stream, q);
    return launch_status("k_interp");
}

template <typename T> int choose_searchsorted(const spc_searchsorted_args *a, SuChoice *c, bool ptrs)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    if (a->n_rows < 0 || a->n_a < 0 || a->n_v < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%ssearchsorted: negative extent");
    if (a->n_rows == 0 || a->n_v == 0) return SU_EMPTY;
    if (a->n_rows == 1 && !su_one_row_fits(a->n_v, 8))            // (8: the int64 indices, whatever the keys' type)
        return fail(SPC_ERR_UNSUPPORTED, "%ssearchsorted: one row of 2^29 keys or more (the kernels address with 32-bit byte offsets)");
    SU_REQUIRE(ptrs, a->v, "v"); SU_REQUIRE(ptrs, a->out, "out");
    if (a->n_a) SU_REQUIRE(ptrs, a->a, "a");
    if ((a->pitch_a && a->pitch_a < a->n_a) || (a->pitch_v && a->pitch_v < a->n_v) || a->pitch_out < a->n_v)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%ssearchsorted: a pitch is smaller than its row (only a and v may be shared, pitch 0)");
    if (!su_pitch_ok(a->n_rows, {a->pitch_a, a->pitch_v, a->pitch_out})) return fail(SPC_ERR_UNSUPPORTED, "%ssearchsorted: a row pitch of 2^24 elements or more");
    c->elem = (int)sizeof(T); c->p2 = floor_pow2(a->n_a);
    const size_t arow = 2 * (size_t)c->p2 + 2;            // su_pad(p2)
    const size_t per_row = a->pitch_a ? arow : 0, fixed = a->pitch_a ? 0 : arow;
    c->rb = su_rows(a->n_rows, a->n_v, per_row, fixed, sizeof(T), &c->stage, a->n_rows > 1 ? su_max({a->pitch_a, a->pitch_v, a->pitch_out}) : 0);
    if ((a->n_rows + c->rb - 1) / c->rb > 0x7fffffff) return fail(SPC_ERR_UNSUPPORTED, "%ssearchsorted: too many rows for one launch");
    c->grid = (unsigned)((a->n_rows + c->rb - 1) / c->rb);
    c->smem = c->stage ? (per_row * c->rb + fixed) * sizeof(T) : 0;
    c->wt = su_write_through(a->n_rows * (int64_t)a->n_v * 8);
    c->sl = c->stage ? (sizeof(T) == 8 ? su_sl(c->p2) : 0) : -1;
    return SPC_OK;
}

template <typename T> int searchsorted_impl(const spc_searchsorted_args *a, void *stream)
{
    SuChoice c;
    const int rc = choose_searchsorted<T>(a, &c, true);
    if (rc) return rc == SU_EMPTY ? SPC_OK : rc;
    SuSearchP q;
    q.n_rows = a->n_rows; q.pitch_a = a->pitch_a; q.pitch_v = a->pitch_v; q.pitch_out = a->pitch_out;
    q.n_a = a->n_a; q.n_v = a->n_v; q.right = a->side_right != 0; q.p2 = c.p2; q.rb = c.rb;
    q.a = a->a; q.v = a->v; q.out = a->out;
    void (*kern)(const SuSearchP) = c.wt ? searchsorted_kernel<T, 1>(c.sl) : searchsorted_kernel<T, 0>(c.sl);
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(SU_THREADS), c.smem, (hipStream_t)stream, q);
    return launch_status("k_searchsorted");
}

// the instantiation of k_interp_c for (PD, SL, WEIGHTED, WT); the unrolled sum depths exist for the staged double kernel
template <typename T, int SL, bool W, int WT> auto interp_c_kernel(int pd) -> void (*)(const SuCoarseP)
{
    if constexpr (sizeof(T) == 8 && SL >= 0) {
        if (pd == 1) return k_interp_c<T, 1, SL, W, WT>;
        if (pd == 2) return k_interp_c<T, 2, SL, W, WT>;
        if (pd == 3) return k_interp_c<T, 3, SL, W, WT>;
    }
    (void)pd;
    return k_interp_c<T, -1, SL, W, WT>;
}

template <typename T, bool W, int WT> auto interp_c_kernel_sl(int sl, int pd) -> void (*)(const SuCoarseP)
{
    if constexpr (sizeof(T) == 8) {              // nL = 160 -> rows z[1:] of 159 entries: SL 8; nL = 512: SL 9
        if (sl == 8) return interp_c_kernel<T, 8, W, WT>(pd);
        if (sl == 9) return interp_c_kernel<T, 9, W, WT>(pd);
    }
    return sl >= 0 ? interp_c_kernel<T, 0, W, WT>(pd) : interp_c_kernel<T, -1, W, WT>(pd);
}

template <typename T> int choose_interp_c(const spc_interp_c_args *a, SuChoice *c, bool ptrs)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    if (a->n_rows < 0 || a->nG < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sinterp_c: negative extent");
    if (a->mode < SU_INTERP_C || a->mode > SU_INTEGRAL) return fail(SPC_ERR_INVALID_ARGUMENT, "%sinterp_c: mode must be 0, 1 or 2");
    if (a->n_rows == 0 || a->nG == 0) return SU_EMPTY;
    if (a->nL < 2) return fail(SPC_ERR_INVALID_ARGUMENT, "%sinterp_c: the fine grid needs at least 2 points");
    // (one row: the coarse bounds Zh[0 .. nG] and the results are addressed with 32-bit byte offsets as interp's points are)
    if (a->n_rows == 1 && !su_one_row_fits((int64_t)a->nG + 1, sizeof(T)))
        return fail(SPC_ERR_UNSUPPORTED, sizeof(T) == 8 ? "%sinterp_c: one row of 2^29 coarse bounds or more (the kernels address with 32-bit byte offsets)"
                                                         : "%sinterp_c: one row of 2^30 coarse bounds or more (the kernels address with 32-bit byte offsets)");
    SU_REQUIRE(ptrs, a->Zh, "Zh"); SU_REQUIRE(ptrs, a->zh, "zh"); SU_REQUIRE(ptrs, a->q, "q"); SU_REQUIRE(ptrs, a->out, "out");
    if (ptrs && a->mode == SU_INTERP_C && !a->rho) return fail(SPC_ERR_INVALID_ARGUMENT, "%sinterp_c: rho is NULL");
    if (a->n_rows > 0x7fffffff) return fail(SPC_ERR_UNSUPPORTED, "%sinterp_c: more than 2^31-1 rows");
    if (a->pitch_Zh < a->nG + 1 || (a->pitch_zh && a->pitch_zh < a->nL) || a->pitch_q < a->nL - 1 || a->pitch_out < a->nG)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sinterp_c: a pitch is smaller than its row (only zh may be shared, pitch 0)");
    if (!su_pitch_ok(a->n_rows, {a->pitch_Zh, a->pitch_zh, a->pitch_q, a->pitch_out})) return fail(SPC_ERR_UNSUPPORTED, "%sinterp_c: a row pitch of 2^24 elements or more");
    // mode 1 ignores rho; mode 2 is weighted where rho is given (the description: mode 0 and, with a non-NULL rho, mode 2)
    c->weighted = a->mode == SU_INTERP_RHO ? 0 : (a->rho != nullptr || a->mode == SU_INTERP_C);
    c->elem = (int)sizeof(T); c->p2 = floor_pow2(a->nL - 1);
    // LDS per row: the cell terms tn (and td with weights) [nL - 1], the coarse levels [nG + 1], the results [nG] + the row's
    // padded grid unless the grid is shared
    const size_t zrow = 2 * (size_t)c->p2 + 2;            // su_pad(p2)
    const size_t per_row = (size_t)(a->nL - 1) * (c->weighted ? 2 : 1) + (size_t)(2 * a->nG + 1) + (a->pitch_zh ? zrow : 0), fixed = a->pitch_zh ? 0 : zrow;
    // 32 KiB (five workgroups per CU, what the registers allow): the layer-major walk skips whole waves above the fine grid's top, the better the more rows a wave spans (measured
    // at 35 718 rows: 5 rows 40.1 us, 7-9 rows 35.4-36.3, 12 rows 37.6: profiles/r04_k7_slab_sweep.log)
    c->rb = su_rows(a->n_rows, a->nG, per_row, fixed, sizeof(T), &c->stage, a->n_rows > 1 ? su_max({a->pitch_Zh, a->pitch_zh, a->pitch_q, a->pitch_out}) : 0, 32, false);
    c->grid = (unsigned)((a->n_rows + c->rb - 1) / c->rb);
    c->smem = c->stage ? (per_row * c->rb + fixed) * sizeof(T) : 0;
    // numpy's pairwise recursion unrolled to the depth a layer of <= nL - 1 cells needs (cons_depth, as K4); the float twin,
    // the unstaged kernel and grids of more than 1024 points keep the explicit stack
    const int pd = sizeof(T) == 8 ? cons_depth(a->nL) : -1;
    c->pd = (sizeof(T) == 8 && c->stage && pd >= 1 && pd <= 3) ? pd : -1;
    c->wt = su_write_through(a->n_rows * (int64_t)a->nG * (int64_t)sizeof(T));
    const int sl = c->stage ? su_sl(c->p2) : -1;
    c->sl = c->stage ? ((sizeof(T) == 8 && (sl == 8 || sl == 9)) ? sl : 0) : -1;
    return SPC_OK;
}

template <typename T> int interp_c_impl(const spc_interp_c_args *a, void *stream)
{
    SuChoice c;
    const int rc = choose_interp_c<T>(a, &c, true);
    if (rc) return rc == SU_EMPTY ? SPC_OK : rc;
    SuCoarseP q;
    q.n_rows = a->n_rows; q.pitch_Zh = a->pitch_Zh; q.pitch_zh = a->pitch_zh; q.pitch_q = a->pitch_q; q.pitch_out = a->pitch_out;
    q.nG = a->nG; q.nL = a->nL; q.mode = a->mode; q.rb = c.rb; q.p2 = c.p2;
    q.Zh = a->Zh; q.zh = a->zh; q.q = a->q; q.rho = a->mode == SU_INTERP_RHO ? nullptr : a->rho; q.out = a->out;
    void (*kern)(const SuCoarseP) = c.weighted ? (c.wt ? interp_c_kernel_sl<T, true, 1>(c.sl, c.pd) : interp_c_kernel_sl<T, true, 0>(c.sl, c.pd))
                                               : (c.wt ? interp_c_kernel_sl<T, false, 1>(c.sl, c.pd) : interp_c_kernel_sl<T, false, 0>(c.sl, c.pd));
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(SU_THREADS), c.smem, (hipStream_t)stream, q);
    return launch_status("k_interp_c");
}

template <typename T> int choose_rms(int64_t n_rows, int64_t n, int64_t pitch, const void *a, const void *out, SuChoice *c, bool ptrs)
{
    if (n_rows < 0 || n < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%srms: negative extent");
    if (n_rows == 0) return SU_EMPTY;
    if (n > 0x7fffffff) return fail(SPC_ERR_UNSUPPORTED, "%srms: more than 2^31-1 elements per row");
    SU_REQUIRE(ptrs, out, "out");
    if (n) SU_REQUIRE(ptrs, a, "a");
    if (pitch < n) return fail(SPC_ERR_INVALID_ARGUMENT, "%srms: pitch smaller than the row");
    const int64_t grid = (n_rows + SU_THREADS / 8 - 1) / (SU_THREADS / 8);
    if (grid > 0x7fffffff) return fail(SPC_ERR_UNSUPPORTED, "%srms: too many rows for one launch");
    // depth of numpy's recursion over one row (a single chunk up to 8192 elements); -1: explicit stack, any length
    c->elem = (int)sizeof(T); c->rb = SU_THREADS / 8; c->grid = (unsigned)grid; c->smem = 0; c->wt = 1;
    c->pd = n <= 128 ? 0 : (n <= 1024 ? cons_depth((int)n) : -1);
    return SPC_OK;
}

template <typename T> int rms_impl(int64_t n_rows, int64_t n, int64_t pitch, const void *a, void *out, void *stream)
{
    SuChoice c;
    const int rc = choose_rms<T>(n_rows, n, pitch, a, out, &c, true);
    if (rc) return rc == SU_EMPTY ? SPC_OK : rc;
    const int pd = c.pd;
    void (*kern)(int64_t, int, int64_t, const T *, T *) =
        pd == 0 ? k_rms<T, 0, 1> : pd == 1 ? k_rms<T, 1, 1> : pd == 2 ? k_rms<T, 2, 1> : pd == 3 ? k_rms<T, 3, 1> : k_rms<T, -1, 1>;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(SU_THREADS), 0, (hipStream_t)stream, n_rows, (int)n, pitch, (const T *)a, (T *)out);
    return launch_status("k_rms");
}
#undef SU_REQUIRE

// ---- the text of spc_sputils_describe_launch (include/spc.h) ----------------------------------------------------------
template <typename T> int su_describe(int op, const void *args, int64_t n_rows, int64_t n, int64_t pitch, SuChoice *c)
{
    switch (op) {
    case SPC_SU_EXNER: return choose_exner<T>(n, nullptr, nullptr, c, false);
    case SPC_SU_INTERP: return choose_interp<T>((const spc_interp_args *)args, c, false);
    case SPC_SU_SEARCHSORTED: return choose_searchsorted<T>((const spc_searchsorted_args *)args, c, false);
    case SPC_SU_INTERP_C: return choose_interp_c<T>((const spc_interp_c_args *)args, c, false);
    case SPC_SU_RMS: return choose_rms<T>(n_rows, n, pitch, nullptr, nullptr, c, false);
    default: return fail(SPC_ERR_INVALID_ARGUMENT, "%ssputils_describe_launch: op must be 0..4");
    }
}

int sputils_describe_launch_impl(int op, int elem_size, const void *args, int64_t n_rows, int64_t n, int64_t pitch, char *buf, int buflen)
{
    if (!buf || buflen < 1) return fail(SPC_ERR_INVALID_ARGUMENT, "%ssputils_describe_launch: no buffer");
    if (elem_size != 8 && elem_size != 4) return fail(SPC_ERR_INVALID_ARGUMENT, "%ssputils_describe_launch: elem_size must be 8 or 4");
    SuChoice c;
    const int rc = elem_size == 8 ? su_describe<double>(op, args, n_rows, n, pitch, &c) : su_describe<float>(op, args, n_rows, n, pitch, &c);
    if (rc < 0) return rc;
    const char *ty = elem_size == 8 ? "f64" : "f32";
    char name[96];
    if (rc == SU_EMPTY) snprintf(name, sizeof(name), "none");
    else if (op == SPC_SU_EXNER) snprintf(name, sizeof(name), "k_exner<%s,wt=%d>", ty, c.wt);
    else if (op == SPC_SU_INTERP) snprintf(name, sizeof(name), "k_interp<%s,sl=%d,wt=%d>", ty, c.sl, c.wt);
    else if (op == SPC_SU_SEARCHSORTED) snprintf(name, sizeof(name), "k_searchsorted<%s,sl=%d,wt=%d>", ty, c.sl, c.wt);
    else if (op == SPC_SU_INTERP_C) snprintf(name, sizeof(name), "k_interp_c<%s,pd=%d,sl=%d,w=%d,wt=%d>", ty, c.pd, c.sl, c.weighted, c.wt);
    else snprintf(name, sizeof(name), "k_rms<%s,pd=%d,wt=%d>", ty, c.pd, c.wt);
    return snprintf(buf, (size_t)buflen, "%s rb=%d grid=%u lds=%lld cus=%d", name, c.rb, c.grid, (long long)c.smem, device_cus());
}
