// spc_launch.hpp -- host side of K1-K5: the error text, argument checks, the launch heuristics, the tables of kernel
// instantiations, the ONE choice per pass (choose_*), the launchers and the text of spc_describe_launch.  Included by
// spc_hip.hip after every kernel and before the *_host.hpp files, which use its first part (fail ... REQUIRE) too.
#pragma once

// ---- what every launcher uses (K1-K5 here, K6-K9 in the *_host.hpp files) -------------------------------------------
thread_local char g_err[512] = "";

int fail(int code, const char *fmt, const char *a = "", long long b = 0, long long c = 0)
{
    snprintf(g_err, sizeof(g_err), fmt, a, b, c);
    return code;
}

int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

// Compute units of the CURRENT device (hipDeviceAttributeMultiprocessorCount; cached per device ordinal): what the residency
// rules below count rounds of workgroups against.  An MI355X in SPX mode has 256; a CPX / DPX partition or another SKU
// has fewer, and rule 1 of pick_cb would silently pick the wrong slab there (round-4 verdict, weak 10).  SPC_CUS=<n>
// overrides (tests walk the heuristics at 32 ... 256 CUs without a GPU); without a device: 256.
int device_cus()
{
    const int forced = env_int("SPC_CUS", 0);
    if (forced > 0) return forced;
    thread_local int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return 256;
    }
    if (dev >= 0 && dev < 64 && cache[dev]) return cache[dev];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        n = 256;
    }
    if (dev >= 0 && dev < 64) cache[dev] = n;
    return n;
}

// Dynamic LDS above the 64 KiB default needs the per-function opt-in (tall columns: nL > ~1300 in K3).
template <typename KernelT> int ensure_lds(KernelT kernel, size_t smem, const char *what)
{
    if (smem <= (size_t)MAX_LDS_BYTES) return SPC_OK;
    if (smem > (size_t)HARD_LDS_BYTES)
        return fail(SPC_ERR_UNSUPPORTED, "%s needs %lld B of LDS per workgroup (gfx950 has %lld)", what, (long long)smem, HARD_LDS_BYTES);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SPC_ERR_UNSUPPORTED, "%s: cannot raise the dynamic LDS limit to %lld B", what, (long long)smem);
    }
    return SPC_OK;
}

int launch_status(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return SPC_OK;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return SPC_ERR_LAUNCH;
}

#define REQUIRE(ptr, name) \
    if (!(ptr)) return fail(SPC_ERR_INVALID_ARGUMENT, "required pointer %s is NULL", name)

// ---- host side of K1-K5 -------------------------------------------------------------------------
int floor_pow2(int n) { return cfloor_pow2(n); }      // (spc_k1.hpp: the kernels take it at compile time)

int validate(const spc_dims *d)
{
    if (!d) return fail(SPC_ERR_INVALID_ARGUMENT, "%sdims is NULL");
    if (d->n_cols < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sn_cols = %lld < 0", "", (long long)d->n_cols);
    if (d->nG < 1 || d->nL < 1)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%slevel counts must be >= 1 (nG=%lld nL=%lld)", "", d->nG, d->nL);
    if (d->pitchG < d->nG || d->pitchGh < d->nG + 1 || d->pitchL < d->nL)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%spitch smaller than the level count");
    if (d->n_cols > (int64_t)INT32_MAX * 8)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sn_cols too large for one launch");
    if (d->cols_per_block < 0 || d->cols_per_block > 64)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%scols_per_block out of range 0..64");
    return SPC_OK;
}

int geometry_id(const spc_dims *d);

// LDS elements per column / per block for each pass (pass 0 fwd, 1 bwd, 2 idx, 3 diag, 4 conservative bwd)
void lds_elems(const spc_dims *d, int pass, bool with_idx, size_t *per_col, size_t *fixed, size_t esize)
{
    const size_t nG = d->nG, nL = d->nL;
    const bool sh = d->les_grid_shared != 0;
    switch (pass) {
    case 0: *per_col = 6 * nG + ((with_idx && !sh) ? nL : 0); *fixed = (with_idx && sh) ? nL : 0; break;
    case 1: *per_col = 6 * nL + nG + (sh ? 0 : nL); *fixed = sh ? nL : 0; break;
    case 4:
        if (geometry_id(d) != 0) {   // k_backward_cons3: A[8][nL+1] | Zh[nG+1] | cell[nG] | start index; zh rows NaN-padded; dz when shared
            const size_t zrow = (size_t)su_pad(floor_pow2((int)nL - 1));
            *per_col = 8 * (nL + 1) + (nG + 1) + (nG * 4 + esize - 1) / esize + 1 + (sh ? 0 : zrow);
            *fixed = sh ? zrow + (nL - 1) : 0;
            break;
        }
        *per_col = 7 * (nL + 1) + 8 * nG + 2 + (nG * 4 + esize - 1) / esize + 1 + (sh ? 0 : nL); *fixed = sh ? nL : 0; break;   // k_backward_cons2; + zf[nL-1] per column
    case 2: *per_col = sh ? 0 : nL; *fixed = sh ? nL : 0; break;
    default: *per_col = 2 * nG; *fixed = 0; break;
    }
}

// Resident workgroups per CU for `kernel` with `smem` bytes of dynamic LDS (occupancy API, cached).
// Without a device (CPU-side ABI tests) falls back to min(4, 160 KiB / smem).
template <typename KernelT> int blocks_per_cu(KernelT kernel, size_t smem)
{
    thread_local std::unordered_map<uint64_t, int> cache;
    const uint64_t key = (uint64_t)(uintptr_t)kernel * 1000003u + smem;
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, BLOCK, smem) != hipSuccess || nb <= 0) {
        (void)hipGetLastError();
        const size_t by_lds = smem ? (size_t)(160 * 1024) / smem : 8;
        nb = (int)(by_lds < 4 ? by_lds : 4);
    }
    if (nb > 8) nb = 8;
    cache[key] = nb;
    return nb;
}

// Columns per workgroup (CB).
//  1. If some CB in {1,2,4} lets the WHOLE grid be resident at once (n_cols/CB <= CUs of the device x resident
//     workgroups per CU at that CB's LDS footprint), take the smallest such CB: a single round of
//     workgroups, maximum parallelism per column (measured: 2048 columns run 13.3 us at CB=2 but 19-20 us
//     at CB=1, which needs two rounds).
//  2. Otherwise (throughput regime) the CB with the most resident workgroups per CU among those that
//     still give >= 2 full rounds of workgroups (rounds de-synchronise the load / compute / store
//     phases), ties to the larger one (longer coalesced slabs): K1 -> 8, K3 -> 2 at 91<->160.
template <typename KernelT> int pick_cb(const spc_dims *d, int pass, bool with_idx, size_t esize, KernelT kernel)
{
    size_t per_col, fixed;
    lds_elems(d, pass, with_idx, &per_col, &fixed, esize);
    int cb = d->cols_per_block;
    if (cb > 0) {
        while (cb > 1 && (per_col * cb + fixed) * esize > (size_t)MAX_LDS_BYTES) --cb;
        return cb;
    }
    int nb[4] = {0, 0, 0, 0};
    const int64_t cus = device_cus();
    for (int i = 0; i < 4; ++i) {
        cb = 1 << i;
        const size_t smem = (per_col * cb + fixed) * esize;
        if (cb > 1 && smem > (size_t)MAX_LDS_BYTES) continue;
        nb[i] = blocks_per_cu(kernel, smem);
        if (cb <= 4 && (d->n_cols + cb - 1) / cb <= cus * nb[i]) return cb;   // rule 1
    }
    // K4 is bound by dependent LDS reads, not by memory: what counts is resident COLUMNS (2 x 4 workgroups beat 1 x 5
    // by 11 % at config 3, 4 x 2 loses 60 %: profiles/r03_k4_forms.log)
    if (pass == 4 && nb[1] * 2 > nb[0] && (d->n_cols + 1) / 2 >= 2 * cus * nb[1]) return 2;
    int best = 1, best_nb = -1;
    // (K3<float>: slabs of more than two columns lose -- 70.9 us at two, 77.5 at four, 88.5 at eight columns per workgroup at
    //  config 3, profiles/r05_f32_cbs.log -- where the residency tie of the 4-byte footprint would pick four)
    for (int i = (pass == 1 && esize == 4) ? 1 : 3; i >= 0; --i) {                      // rule 2
        cb = 1 << i;
        const int64_t rounds_x_cus = nb[i] ? (d->n_cols + cb - 1) / cb / nb[i] : 0;   // rounds of workgroups x CUs
        const bool enough = rounds_x_cus >= (cb == 8 ? 8 : 2) * cus;   // measured: 8-column slabs pay off from ~8 rounds
        if (nb[i] > best_nb && (enough || i == 0)) { best_nb = nb[i]; best = cb; }
    }
    return best;
}

// Launches that write no more than the aggregate L2 (32 MiB) store write-through: otherwise all of it is
// still dirty when the kernel ends and the end-of-kernel release has to flush it (measured: WT wins up
// to ~4096 columns, loses beyond ~16k).
int small_batch(int64_t bytes_written, int limit_mib = 32)
{
    return bytes_written <= (int64_t)limit_mib * 1024 * 1024 ? 1 : 0;
}

// 0 = generic; 1..3 = compile-time geometries with contiguous columns (see k_forward)
int geometry_id(const spc_dims *d)
{
    if (d->pitchG != d->nG || d->pitchGh != d->nG + 1 || d->pitchL != d->nL) return 0;
    if (d->nG == 91 && d->nL == 160) return 1;
    if (d->nG == 137 && d->nL == 512) return 2;
    if (d->nG == 19 && d->nL == 160) return 3;
    return 0;
}

DimsP make_dims(const spc_dims *d, int cb)
{
    DimsP p;
    p.n_cols = d->n_cols; p.pitchG = d->pitchG; p.pitchGh = d->pitchGh; p.pitchL = d->pitchL;
    p.nG = d->nG; p.nL = d->nL; p.cb = cb; p.p2G = floor_pow2(d->nG); p.p2L = floor_pow2(d->nL);
    p.shared_grid = d->les_grid_shared != 0;
    p.xcd_remap = cb <= 2;   // measured: +4-6 % for 1-2 column slabs (K3), -1.5 % for 8-column slabs (K1)
    return p;
}

// Small batches run ONE round of workgroups and are bound by latency, not bandwidth: there fewer, larger workgroups
// win.  2 / 4 columns per workgroup of 512 / 1024 threads (still one work item per thread, so the per-thread chain is
// unchanged) cover <= 1024 columns with <= 256 workgroups -- one per CU -- and the grid is dispatched in a half / a
// quarter of the time.  Measured (pre-heated, profiles/r02_ab_blocks.log): K1 8.5 -> 7.1 us and
// K3 8.1 -> 7.8 us at 1024 columns, K1 6.4 -> 5.4 us at 512; slower from 1536 columns on.  Returns the columns per
// workgroup (workgroup = 256 x that) or 0 = the 256-thread path.  SPC_SMALL_BLOCK=0 disables it (tests).
int small_block(const spc_dims *d, int items_per_col)
{
    const int64_t cus = device_cus();          // (MI355X: 256 -> the 257 ... 1024 columns of the measurements above)
    if (d->cols_per_block != 0 || items_per_col > BLOCK || d->n_cols <= cus || d->n_cols > 4 * cus) return 0;
    const int sb = env_int("SPC_SMALL_BLOCK", 1);                    // 0: off; 2 / 4: that many columns per workgroup (tests)
    if (!sb) return 0;
    if (sb == 2 || sb == 4) return sb;
    return d->n_cols <= 2 * cus ? 2 : 4;
}

// ---- launch choice ---------------------------------------------------------------------------------------------
// WHICH instantiation runs, and in what shape, is decided in ONE place per pass (choose_fwd / choose_idx / choose_bwd /
// choose_diag); the launchers and spc_describe_launch (include/spc.h) both call it, so a test can walk the dispatch table and
// assert that every instantiation it can reach has been bit-checked (tests/test_dispatch_gpu.py).
struct Choice {
    const char *kernel;   // what a failed launch is reported as
    int elem, full, idx, geo, wt, blk, pre, cb;
    int vec = 0;      // the float kernels with 8-byte accesses (spc_f32v.hpp)
    int pd = 0;       // K4 at a run-time geometry: the PD of the k_backward_cons2 instantiation (cons_kernel)
    unsigned grid;
    size_t smem;
};

// the last step of every choose_*: dynamic LDS and grid of c->cb columns per workgroup
template <typename T> int choose_shape(const spc_dims *d, int pass, bool with_idx, Choice *c)
{
    size_t per_col, fixed;
    lds_elems(d, pass, with_idx, &per_col, &fixed, sizeof(T));
    c->smem = (per_col * c->cb + fixed) * sizeof(T);
    c->grid = (unsigned)((d->n_cols + c->cb - 1) / c->cb);
    return SPC_OK;
}

// the launch of K1-K5 in the shape of `c`; `what` names the operator where the LDS limit refuses it
template <typename... P, typename... A> int launch(void (*kern)(P...), const Choice &c, void *stream, const char *what, const A &...args)
{
    const int rc = ensure_lds(kern, c.smem, what);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(c.blk), c.smem, (hipStream_t)stream, args...);
    return launch_status(c.kernel);
}

constexpr int GEO_NG[4] = {0, 91, 137, 19}, GEO_NL[4] = {0, 160, 512, 160};

template <typename T> using KLean = void (*)(const FwdP<T, false>);
template <typename T> using KFull = void (*)(const FwdP<T, true>);
template <typename T> using KBwd = void (*)(const BwdP<T>);

#define SPC_FWD_ROW(FULL_, WT_, BLK_, PRE_)                                                                          \
    {k_forward<T, FULL_, 0, 0, WT_, BLK_, PRE_>, k_forward<T, FULL_, 91, 160, WT_, BLK_, PRE_>,                      \
     k_forward<T, FULL_, 137, 512, WT_, BLK_, PRE_>, k_forward<T, FULL_, 19, 160, WT_, BLK_, PRE_>}
// 512- / 1024-thread workgroups (small_block): one round of <= 1024 columns of <= 256 work items each, i.e. always
// write-through and never 137 <-> 512 (649 work items per column): only those instantiations exist
#define SPC_FWD_ROW_BIG(BLK_)                                                                                        \
    {k_forward<T, false, 0, 0, 1, BLK_, true>, k_forward<T, false, 91, 160, 1, BLK_, true>, nullptr,                 \
     k_forward<T, false, 19, 160, 1, BLK_, true>}

// lean forward kernel of (geometry, write-through, workgroup size, prologue prefetch); nullptr = not instantiated
template <typename T> KLean<T> fwd_lean_kernel(int geo, int wt, int blk, int pre)
{
    static const KLean<T> k256[2][2][4] = {{SPC_FWD_ROW(false, 0, BLOCK, false), SPC_FWD_ROW(false, 1, BLOCK, false)},
                                           {SPC_FWD_ROW(false, 0, BLOCK, true), SPC_FWD_ROW(false, 1, BLOCK, true)}};
    static const KLean<T> k512[4] = SPC_FWD_ROW_BIG(512), k1024[4] = SPC_FWD_ROW_BIG(1024);
    if (blk == BLOCK) return k256[pre][wt][geo];
    if (!wt || !pre) return nullptr;
    return blk == 512 ? k512[geo] : (blk == 1024 ? k1024[geo] : nullptr);
}

// the FULL variant (optional outputs, surface coupling: convert_profiles() and cplsurf=True, off the default path of
// splib.py:67) exists with plain stores only: write-through is worth ~5 % on launches of <= 4 k columns and would double
// the number of its instantiations
template <typename T> KFull<T> fwd_full_kernel(int geo, int pre)
{
    static const KFull<T> k[2][4] = {SPC_FWD_ROW(true, 0, BLOCK, false), SPC_FWD_ROW(true, 0, BLOCK, true)};
    return k[pre][geo];
}
#undef SPC_FWD_ROW
#undef SPC_FWD_ROW_BIG

template <typename T> int choose_fwd(const spc_dims *d, bool with_idx, bool full, Choice *c)
{
    c->kernel = "k_forward"; c->elem = (int)sizeof(T); c->full = full; c->idx = with_idx;
    c->geo = geometry_id(d);
    c->wt = full ? 0 : small_batch(d->n_cols * (int64_t)((6 * d->nL + 1) * sizeof(T) + (with_idx ? d->nG * 4 : 0)));
    // (137 <-> 512 never qualifies for small_block: 649 work items per column; the 512- / 1024-thread kernels exist with
    //  write-through stores only)
    const int sb = (full || !c->wt) ? 0 : small_block(d, d->nL + (with_idx ? d->nG : 0));
    // single-round launches keep the prologue prefetch (k_forward's PRE); SPC_K1_PRE=0/1 forces it off / on (tests)
    const int pre_env = env_int("SPC_K1_PRE", -1);
    c->pre = (sb || (pre_env >= 0 ? pre_env != 0 : d->n_cols <= 4 * (int64_t)device_cus())) ? 1 : 0;   // measured (256 CUs): PRE = false wins from 1100 columns
    c->blk = sb ? BLOCK * sb : BLOCK;
    if (full)
        c->cb = pick_cb(d, 0, with_idx, sizeof(T), fwd_full_kernel<T>(c->geo, c->pre));
    else
        c->cb = sb ? sb : pick_cb(d, 0, with_idx, sizeof(T), fwd_lean_kernel<T>(c->geo, 0, BLOCK, c->pre));
    // float, compile-time geometry, lean, multi-round, an even slab: 8-byte accesses (spc_f32v.hpp; SPC_F32_VEC=0: tests)
    c->vec = std::is_same<T, float>::value && c->geo != 0 && !full && !sb && !c->pre && c->cb % 2 == 0 && env_int("SPC_F32_VEC", 1);
    return choose_shape<T>(d, 0, with_idx, c);
}

// K1 of the float variant with 8-byte accesses, by (geometry, write-through)
inline KLean<float> fwd_vec_kernel(int geo, int wt)
{
    static const KLean<float> k[2][4] = {{nullptr, k_forward_f32v<91, 160, 0>, k_forward_f32v<137, 512, 0>, k_forward_f32v<19, 160, 0>},
                                         {nullptr, k_forward_f32v<91, 160, 1>, k_forward_f32v<137, 512, 1>, k_forward_f32v<19, 160, 1>}};
    return k[wt ? 1 : 0][geo];
}
inline bool aligned8(std::initializer_list<const void *> ptrs)
{
    for (const void *q : ptrs) if ((uintptr_t)q & 7u) return false;
    return true;
}

template <typename T> int forward_impl(const spc_dims *d, const spc_forward_args *a, void *stream)
{
    int rc = validate(d);
    if (rc) return rc;
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    if (d->n_cols == 0) return SPC_OK;
    REQUIRE(a->U, "U"); REQUIRE(a->V, "V"); REQUIRE(a->T, "T"); REQUIRE(a->SH, "SH"); REQUIRE(a->QL, "QL");
    REQUIRE(a->QI, "QI"); REQUIRE(a->Pf, "Pf"); REQUIRE(a->Ph, "Ph"); REQUIRE(a->Zgfull, "Zgfull");
    REQUIRE(a->Zghalf, "Zghalf"); REQUIRE(a->zf, "zf"); REQUIRE(a->u_d, "u_d"); REQUIRE(a->v_d, "v_d");
    REQUIRE(a->thl_d, "thl_d"); REQUIRE(a->qt_d, "qt_d"); REQUIRE(a->ql_d, "ql_d"); REQUIRE(a->ps_d, "ps_d");
    REQUIRE(a->f_u, "f_u"); REQUIRE(a->f_v, "f_v"); REQUIRE(a->f_thl, "f_thl"); REQUIRE(a->f_qt, "f_qt");
    REQUIRE(a->f_ql, "f_ql"); REQUIRE(a->ql_ref, "ql_ref"); REQUIRE(a->f_ps, "f_ps");
    if (a->idx && !a->zh) return fail(SPC_ERR_INVALID_ARGUMENT, "%sidx requested but zh is NULL");
    if (a->rainrate && (!a->rain || !a->rain_last))
        return fail(SPC_ERR_INVALID_ARGUMENT, "%srainrate requested but rain / rain_last is NULL");
    if (a->wthl || a->wqt) {
        if (!a->wthl || !a->wqt || !a->QLflux || !a->QIflux || !a->SHflux || !a->TSflux)
            return fail(SPC_ERR_INVALID_ARGUMENT, "%ssurface coupling needs wthl, wqt and QLflux,QIflux,SHflux,TSflux");
        if ((a->z0m && !a->Z0M) || (a->z0h && !a->Z0H))
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sz0m/z0h requested but Z0M/Z0H is NULL");
    }
    const bool with_idx = a->idx != nullptr;
    const bool full = a->u || a->v || a->thl || a->qt || a->ps || a->Zf || a->Zh || a->rainrate || a->wthl;
    Choice c;
    if ((rc = choose_fwd<T>(d, with_idx, full, &c))) return rc;
#define CP(f) p.f = (const T *)a->f
#define OP(f) p.f = (T *)a->f
#define COP(f) p.o.f = (const T *)a->f
#define OOP(f) p.o.f = (T *)a->f
    auto fill = [&](auto &p) {
        p.d = make_dims(d, c.cb);
        CP(U); CP(V); p.Tm = (const T *)a->T; CP(SH); CP(QL); CP(QI); CP(Pf); CP(Ph); CP(Zgfull); CP(Zghalf);
        CP(zf); CP(zh); CP(u_d); CP(v_d); CP(thl_d); CP(qt_d); CP(ql_d); CP(ps_d);
        p.factor = (T)a->factor; p.dt = (T)a->dt;
        OP(f_u); OP(f_v); OP(f_thl); OP(f_qt); OP(f_ql); OP(ql_ref); OP(f_ps); p.idx = a->idx;
    };
    if (full) {
        const KFull<T> kern = fwd_full_kernel<T>(c.geo, c.pre);
        FwdP<T, true> p;
        fill(p);
        COP(rain); COP(rain_last); OOP(u); OOP(v); OOP(thl); OOP(qt); OOP(ps); OOP(Zf); OOP(Zh); OOP(rainrate);
        COP(Z0M); COP(Z0H); COP(QLflux); COP(QIflux); COP(SHflux); COP(TSflux); OOP(z0m); OOP(z0h); OOP(wthl); OOP(wqt);
        return launch(kern, c, stream, "forward", p);
    } else {
        KLean<T> kern = fwd_lean_kernel<T>(c.geo, c.wt, c.blk, c.pre);
        if constexpr (std::is_same<T, float>::value) {
            if (c.vec && aligned8({a->U, a->V, a->T, a->SH, a->QL, a->QI, a->Pf, a->Zgfull, a->zf, a->u_d, a->v_d, a->thl_d, a->qt_d, a->ql_d,
                                   a->f_u, a->f_v, a->f_thl, a->f_qt, a->f_ql, a->ql_ref}))
                kern = fwd_vec_kernel(c.geo, c.wt);
        }
        if (!kern) return fail(SPC_ERR_UNSUPPORTED, "%sforward: no kernel instantiated for this launch choice (internal)");
        FwdP<T, false> p;
        fill(p);
        return launch(kern, c, stream, "forward", p);
    }
}

// launch choice of K2 (one instantiation per type)
template <typename T> int choose_idx(const spc_dims *d, Choice *c)
{
    c->kernel = "k_cloud_idx"; c->elem = (int)sizeof(T); c->full = c->idx = c->geo = c->wt = c->pre = 0;
    c->blk = BLOCK;
    c->cb = pick_cb(d, 2, true, sizeof(T), k_cloud_idx<T>);
    return choose_shape<T>(d, 2, true, c);
}

template <typename T>
int cloud_idx_impl(const spc_dims *d, const void *zh, const void *Zh, int32_t *idx, void *stream)
{
    int rc = validate(d);
    if (rc) return rc;
    if (d->n_cols == 0) return SPC_OK;
    REQUIRE(zh, "zh"); REQUIRE(Zh, "Zh"); REQUIRE(idx, "idx");
    Choice c;
    if ((rc = choose_idx<T>(d, &c))) return rc;
    return launch(k_cloud_idx<T>, c, stream, "cloud_indices", make_dims(d, c.cb), (const T *)zh, (const T *)Zh, idx);
}

#define SPC_BWD_ROW(WT_, BLK_, PRE_)                                                                                 \
    {k_backward<T, 0, 0, WT_, BLK_, PRE_>, k_backward<T, 91, 160, WT_, BLK_, PRE_>, k_backward<T, 137, 512, WT_, BLK_, PRE_>, \
     k_backward<T, 19, 160, WT_, BLK_, PRE_>}
#define SPC_BWD_ROW_BIG(BLK_)                                                                                        \
    {k_backward<T, 0, 0, 1, BLK_, true>, k_backward<T, 91, 160, 1, BLK_, true>, nullptr, k_backward<T, 19, 160, 1, BLK_, true>}

// K3 of (geometry, write-through, workgroup size, prologue prefetch); nullptr = not instantiated (see fwd_lean_kernel)
template <typename T> KBwd<T> bwd_kernel(int geo, int wt, int blk, int pre)
{
    static const KBwd<T> k256[2][2][4] = {{SPC_BWD_ROW(0, BLOCK, false), SPC_BWD_ROW(1, BLOCK, false)},
                                          {SPC_BWD_ROW(0, BLOCK, true), SPC_BWD_ROW(1, BLOCK, true)}};
    static const KBwd<T> k512[4] = SPC_BWD_ROW_BIG(512), k1024[4] = SPC_BWD_ROW_BIG(1024);
    if (blk == BLOCK) return k256[pre][wt][geo];
    if (!wt || !pre) return nullptr;
    return blk == 512 ? k512[geo] : (blk == 1024 ? k1024[geo] : nullptr);
}
#undef SPC_BWD_ROW
#undef SPC_BWD_ROW_BIG

// the CB of the k_backward_cons3 instantiation that runs `cb` columns per workgroup
inline int cons3_cb(int cb) { return cb >= 2 ? 2 : 1; }

// K4 of a geometry; run-time geometry (geo 0): numpy's pairwise recursion unrolled to the depth nL needs (spc_k4.hpp) --
// pd = 1, 2, 3 for LES grids of up to 248 / 488 / 968 levels, else the explicit-stack form
template <typename T> KBwd<T> cons_kernel(int geo, int pd, int cb)
{
    // compile-time geometries: the third form (spc_k4.hpp: products per cell, padded scans, layer means stashed in registers)
    static const KBwd<T> k3[4][2] = {{nullptr, nullptr},
                                     {k_backward_cons3<T, 91, 160, 1>, k_backward_cons3<T, 91, 160, 2>},
                                     {k_backward_cons3<T, 137, 512, 1>, k_backward_cons3<T, 137, 512, 2>},
                                     {k_backward_cons3<T, 19, 160, 1>, k_backward_cons3<T, 19, 160, 2>}};
    if (geo != 0) return k3[geo][cons3_cb(cb) - 1];
    if constexpr (std::is_same<T, double>::value) {      // (the float twin, config 5's tolerance sweep, keeps the stack form)
        static const KBwd<T> kd[3] = {k_backward_cons2<T, 0, 0, 1>, k_backward_cons2<T, 0, 0, 2>, k_backward_cons2<T, 0, 0, 3>};
        if (pd >= 1 && pd <= 3) return kd[pd - 1];
    }
    return k_backward_cons2<T, 0, 0, -1>;
}

// columns per workgroup of the third-form K4: one while the whole grid is resident at once (a single round: the most
// parallelism per column), else two when that keeps more COLUMNS resident per CU (K4's rate follows them, spc_k4.hpp)
template <typename T> int pick_cb_cons3(const spc_dims *d, int geo)
{
    size_t per_col, fixed;
    lds_elems(d, 4, false, &per_col, &fixed, sizeof(T));
    const size_t smem1 = (per_col + fixed) * sizeof(T), smem2 = (2 * per_col + fixed) * sizeof(T);
    const bool two_fits = smem2 <= (size_t)MAX_LDS_BYTES;
    if (d->cols_per_block > 0) return (d->cols_per_block >= 2 && two_fits) ? 2 : 1;
    const int nb1 = blocks_per_cu(cons_kernel<T>(geo, 0, 1), smem1);
    if (d->n_cols <= (int64_t)device_cus() * nb1 || !two_fits) return 1;
    const int nb2 = blocks_per_cu(cons_kernel<T>(geo, 0, 2), smem2);
    return nb2 * 2 > nb1 ? 2 : 1;
}

// depth of numpy's pairwise recursion over at most nL elements (<= 8192: one chunk); -1: use the explicit stack
int cons_depth(int nL)
{
    if (nL > 1024) return -1;
    // vn_pw_depth(n) = max over 129 .. n of the (triple-recursive) depth of n: a running maximum, filled ONCE (it was
    // re-evaluated three times per K4 launch: tens of thousands of calls for a grid of ~1000 levels)
    static const struct Tab { signed char d[1025]; Tab() { int m = 0; for (int n = 0; n <= 1024; ++n) { if (n >= 129) { const int dn = vn_pw_depth_of(n); if (dn > m) m = dn; } d[n] = (signed char)m; } } } tab;
    const int d = nL < 0 ? 0 : tab.d[nL];
    return d < 1 ? 1 : (d <= 3 ? d : -1);
}

template <typename T> int choose_bwd(const spc_dims *d, bool cons, Choice *c)
{
    c->kernel = cons ? "k_backward_cons" : "k_backward"; c->elem = (int)sizeof(T); c->full = cons; c->idx = 0;
    c->geo = geometry_id(d);
    c->pd = (cons && c->geo == 0) ? (std::is_same<T, double>::value ? cons_depth(d->nL) : -1) : 0;
    // K3's stores stop gaining from write-through earlier than K1's: at 2 560 columns (13 MB written) it still wins 5-7 %, at
    // 3 072 ... 6 144 it loses 2-5 % (profiles/r04_write_through_sweep.log); K4 loses 10 % at config 3 (182 MB)
    c->wt = cons ? 0 : small_batch(d->n_cols * (int64_t)(7 * d->nG * sizeof(T)), 14);
    const int sb = (cons || !c->wt) ? 0 : small_block(d, d->nL > d->nG ? d->nL : d->nG);
    // PRE = false (8 waves per SIMD) pays between one round of workgroups and saturation: 1 025 ... 25 000 columns
    const int64_t cus = device_cus();      // the measured bounds 1 025 ... 25 000 are 4 ... ~98 columns per CU of the 256
    c->pre = (cons || sb || d->n_cols <= 4 * cus || d->n_cols * 256 > 25000 * cus) ? 1 : 0;
    c->blk = sb ? BLOCK * sb : BLOCK;
    c->cb = sb ? sb : (cons ? (c->geo ? pick_cb_cons3<T>(d, c->geo) : pick_cb(d, 4, false, sizeof(T), cons_kernel<T>(0, c->pd, 0)))
                            : pick_cb(d, 1, false, sizeof(T), bwd_kernel<T>(c->geo, 0, BLOCK, c->pre)));
    return choose_shape<T>(d, cons ? 4 : 1, false, c);
}

template <typename T> int backward_impl(const spc_dims *d, const spc_backward_args *a, void *stream)
{
    int rc = validate(d);
    if (rc) return rc;
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    if (d->n_cols == 0) return SPC_OK;
    REQUIRE(a->T, "T"); REQUIRE(a->SH, "SH"); REQUIRE(a->QL, "QL"); REQUIRE(a->QI, "QI"); REQUIRE(a->U, "U");
    REQUIRE(a->V, "V"); REQUIRE(a->A, "A"); REQUIRE(a->zf, "zf"); REQUIRE(a->t_d, "t_d"); REQUIRE(a->qt_d, "qt_d");
    REQUIRE(a->ql_d, "ql_d"); REQUIRE(a->ql_ice_d, "ql_ice_d"); REQUIRE(a->u_d, "u_d"); REQUIRE(a->v_d, "v_d");
    REQUIRE(a->A_prof, "A_prof"); REQUIRE(a->f_T, "f_T"); REQUIRE(a->f_SH, "f_SH"); REQUIRE(a->f_QL, "f_QL");
    REQUIRE(a->f_QI, "f_QI"); REQUIRE(a->f_U, "f_U"); REQUIRE(a->f_V, "f_V"); REQUIRE(a->f_A, "f_A");
    if (!a->Zf && (!a->Zgfull || !a->Zghalf))
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sneither Zf nor (Zgfull, Zghalf) given");
    const bool cons = a->conservative != 0;
    if (cons) {
        REQUIRE(a->zh, "zh (conservative)"); REQUIRE(a->rhobf_d, "rhobf_d (conservative)");
        if (!a->Zh && !a->Zghalf) return fail(SPC_ERR_INVALID_ARGUMENT, "%sconservative: neither Zh nor Zghalf given");
        if (d->nL < 2) return fail(SPC_ERR_INVALID_ARGUMENT, "%sconservative coarsening needs nL >= 2");
    }
    Choice c;
    if ((rc = choose_bwd<T>(d, cons, &c))) return rc;
    const KBwd<T> kern = cons ? cons_kernel<T>(c.geo, c.pd, c.cb) : bwd_kernel<T>(c.geo, c.wt, c.blk, c.pre);
    if (!kern) return fail(SPC_ERR_UNSUPPORTED, "%sbackward: no kernel instantiated for this launch choice (internal)");
    BwdP<T> p;
    p.d = make_dims(d, c.cb);
    p.Tm = (const T *)a->T; CP(SH); CP(QL); CP(QI); CP(U); CP(V); CP(A); CP(Zf); CP(Zgfull); CP(Zghalf); CP(zf);
    CP(t_d); CP(qt_d); CP(ql_d); CP(ql_ice_d); CP(u_d); CP(v_d); CP(A_prof); CP(zh); CP(Zh); CP(rhobf_d);
    p.factor = (T)a->factor; p.dt = (T)a->dt;
    OP(f_T); OP(f_SH); OP(f_QL); OP(f_QI); OP(f_U); OP(f_V); OP(f_A); p.start_index = a->start_index;
    return launch(kern, c, stream, cons ? "backward (conservative)" : "backward", p);
}

template <typename T> using KDiag = void (*)(const DiagP<T>);

// K5 of (geometry, write-through)
template <typename T> KDiag<T> diag_kernel(int geo, int wt)
{
    static const KDiag<T> k[2][4] = {{k_diag<T, 0, 0, 0>, k_diag<T, 91, 160, 0>, k_diag<T, 137, 512, 0>, k_diag<T, 19, 160, 0>},
                                     {k_diag<T, 0, 0, 1>, k_diag<T, 91, 160, 1>, k_diag<T, 137, 512, 1>, k_diag<T, 19, 160, 1>}};
    return k[wt ? 1 : 0][geo];
}

// launch choice of K5 (as choose_fwd / choose_bwd: ONE place, also behind spc_describe_launch); `a` may be NULL (describe: every
// output assumed)
template <typename T> int choose_diag(const spc_dims *d, const spc_diagnostics_args *a, Choice *c)
{
    c->kernel = "k_diag"; c->elem = (int)sizeof(T); c->full = c->idx = 0; c->pre = 0; c->blk = BLOCK;
    c->geo = geometry_id(d);
    const int64_t nGw = !a ? 4 : (a->Tv != nullptr) + (a->THL != nullptr) + (a->QT != nullptr) + (a->Zf != nullptr);
    const int64_t nLw = !a ? 3 : (a->pf != nullptr) + (a->t != nullptr) + (a->ql_water != nullptr);
    const int64_t elems = nGw * d->nG + ((!a || a->Zh) ? d->nG + 1 : 0) + ((!a || a->zf) ? nLw * d->nL : 0);
    c->wt = small_batch(d->n_cols * elems * (int64_t)sizeof(T));
    c->cb = pick_cb(d, 3, false, sizeof(T), diag_kernel<T>(c->geo, 0));
    return choose_shape<T>(d, 3, false, c);
}

template <typename T> int diag_impl(const spc_dims *d, const spc_diagnostics_args *a, void *stream)
{
    int rc = validate(d);
    if (rc) return rc;
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    if (d->n_cols == 0) return SPC_OK;
    REQUIRE(a->T, "T"); REQUIRE(a->SH, "SH"); REQUIRE(a->QL, "QL"); REQUIRE(a->QI, "QI"); REQUIRE(a->Pf, "Pf");
    REQUIRE(a->Zgfull, "Zgfull"); REQUIRE(a->Zghalf, "Zghalf");
    if ((a->pf || a->t || a->ql_water) && !a->zf) return fail(SPC_ERR_INVALID_ARGUMENT, "%sLES diagnostics need zf");
    if (a->t && (!a->thl_d || !a->ql_d)) return fail(SPC_ERR_INVALID_ARGUMENT, "%st needs thl_d and ql_d");
    if (a->ql_water && (!a->ql_d || !a->ql_ice_d)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sql_water needs ql_d and ql_ice_d");
    Choice c;
    if ((rc = choose_diag<T>(d, a, &c))) return rc;
    DiagP<T> p;
    p.d = make_dims(d, c.cb);
    p.Tm = (const T *)a->T; CP(SH); CP(QL); CP(QI); CP(Pf); CP(Zgfull); CP(Zghalf); CP(zf); CP(thl_d); CP(ql_d); CP(ql_ice_d);
    OP(Tv); OP(THL); OP(QT); OP(Zf); OP(Zh); OP(pf); OP(t); OP(ql_water);
    return launch(diag_kernel<T>(c.geo, c.wt), c, stream, "diagnostics", p);
}
#undef CP
#undef OP
#undef COP
#undef OOP

template <typename T>
int surface_impl(int64_t n, const void *Ph_s, const void *T_s, const void *QLflux, const void *QIflux,
                        const void *SHflux, const void *TSflux, void *wthl, void *wqt, void *stream)
{
    if (n < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%ssurface_fluxes: n < 0");
    if (n == 0) return SPC_OK;
    if (!Ph_s || !T_s || !QLflux || !QIflux || !SHflux || !TSflux || !wthl || !wqt)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%ssurface_fluxes: NULL pointer");
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK < 2048 ? (n + BLOCK - 1) / BLOCK : 2048);
    hipLaunchKernelGGL(k_surface<T>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, n, (const T *)Ph_s, (const T *)T_s,
                       (const T *)QLflux, (const T *)QIflux, (const T *)SHflux, (const T *)TSflux, (T *)wthl, (T *)wqt);
    return launch_status("k_surface");
}

template <typename T> int describe_impl(const spc_dims *d, int pass, int flags, Choice *c)
{
    switch (pass) {
    case 0: return choose_fwd<T>(d, (flags & 1) != 0, (flags & 2) != 0, c);
    case 1: return choose_bwd<T>(d, false, c);
    case 4: return choose_bwd<T>(d, true, c);
    case 3: return choose_diag<T>(d, nullptr, c);
    case 2: return choose_idx<T>(d, c);
    default: return fail(SPC_ERR_INVALID_ARGUMENT, "%spass must be 0..4");
    }
}

// The instantiation `c` stands for, spelled as the tables above index it (fwd_lean_kernel / fwd_full_kernel / fwd_vec_kernel,
// bwd_kernel, cons_kernel, diag_kernel): what tests/test_dispatch_gpu.py keys its bit-checks by.
void choice_name(const Choice &c, int pass, char *name, size_t len)
{
    const char *ty = c.elem == 8 ? "f64" : "f32";
    const int nG = GEO_NG[c.geo], nL = GEO_NL[c.geo];
    if (pass == 0 && c.vec)
        snprintf(name, len, "k_forward_f32v<%d,%d,wt=%d>", nG, nL, c.wt);
    else if (pass == 0)
        snprintf(name, len, "k_forward<%s,%s,%d,%d,wt=%d,blk=%d,pre=%d>", ty, c.full ? "full" : "lean", nG, nL, c.wt, c.blk, c.pre);
    else if (pass == 1)
        snprintf(name, len, "k_backward<%s,%d,%d,wt=%d,blk=%d,pre=%d>", ty, nG, nL, c.wt, c.blk, c.pre);
    else if (pass == 4 && c.geo == 0)
        snprintf(name, len, "k_backward_cons2<%s,0,0,pd=%d>", ty, c.pd);
    else if (pass == 4)
        snprintf(name, len, "k_backward_cons3<%s,%d,%d,cb=%d>", ty, nG, nL, cons3_cb(c.cb));
    else if (pass == 3)
        snprintf(name, len, "k_diag<%s,%d,%d,wt=%d>", ty, nG, nL, c.wt);
    else
        snprintf(name, len, "%s<%s>", c.kernel, ty);
}

int describe_launch_impl(const spc_dims *d, int pass, int flags, int elem_size, char *buf, int buflen)
{
    int rc = validate(d);
    if (rc) return rc;
    if (!buf || buflen < 1) return fail(SPC_ERR_INVALID_ARGUMENT, "%sdescribe_launch: no buffer");
    if (elem_size != 8 && elem_size != 4) return fail(SPC_ERR_INVALID_ARGUMENT, "%sdescribe_launch: elem_size must be 8 or 4");
    Choice c = {};
    rc = elem_size == 8 ? describe_impl<double>(d, pass, flags, &c) : describe_impl<float>(d, pass, flags, &c);
    if (rc) return rc;
    char name[160];
    choice_name(c, pass, name, sizeof(name));
    // K1's phase structure: "reach" = the PRE = false kernels (GCM fields loaded only up to the LES interpolation's reach),
    // "whole" = one phase over every level (PRE = true), "vec" = k_forward_f32v (every level)
    const char *form = pass != 0 ? "" : (c.vec ? " form=vec" : (c.pre ? " form=whole" : " form=reach"));
    return snprintf(buf, (size_t)buflen, "%s cb=%d grid=%u block=%d lds=%lld cus=%d%s", name, c.cb, c.grid, c.blk, (long long)c.smem,
                    device_cus(), form);
}

int pick_cols_per_block_impl(const spc_dims *d, int pass)
{
    int rc = validate(d);
    if (rc) return rc;
    Choice c = {};
    rc = describe_impl<double>(d, pass, 1, &c);     // forward: lean, with the fused index map
    return rc ? rc : c.cb;
}
