// spc_vnudge_host.hpp -- argument checks and launches of K6, the variability nudge (kernels: spc_vnudge2.hpp, numpy-ordered
// sums and the pairwise tree: spc_vnudge.hpp); included by spc_hip.hip after spc_launch.hpp (fail, REQUIRE, ensure_lds,
// launch_status, env_int).
#pragma once

// leaves of numpy's pairwise recursion over n elements (n <= 8192): the host-side twin of vn_build_tree's count
static int vn_count_leaves(int n)
{
    if (n <= 128) return 1;
    int n2 = n / 2;
    n2 -= n2 % 8;
    return vn_count_leaves(n2) + vn_count_leaves(n - n2);
}

// LDS bytes of the plane-resident solver (spc_vnudge2.hpp) with `t` levels per workgroup and planes of T
template <typename T> static size_t vn_lds_need(int nij, int nleaf_max, int t)
{
    return (size_t)t * vn2_plane(nij) * 2 * sizeof(T) + (size_t)t * nleaf_max * 8 + VN2_THREADS * (sizeof(T) + 4);
}

// Planes that fit the LDS (KT levels x nij x 2 sizeof(T) <= 150 KiB, KT a power of two <= 16; 64 x 64 planes: KT = 2 in
// double, 4 would fit in float) are solved there; larger planes (double: > ~9 000 points, float: > ~18 000) are streamed from the
// transposed workspace.  Returns whether the LDS path applies, the levels per workgroup and the leaf count of numpy's pairwise tree.
template <typename T> static bool vn_lds_fit(int nij, int *kt_, int *log2_kt_, int *nleaf_max_)
{
    int kt = 16, log2_kt = 4;
    const int cn = nij < 8192 ? nij : 8192, nleaf_max = nij > 8192 ? VN_MAXLEAF : vn_count_leaves(cn);
    while (kt > 1 && vn_lds_need<T>(nij, nleaf_max, kt) > (size_t)VN2_MAX_LDS) { kt >>= 1; --log2_kt; }
    *kt_ = kt; *log2_kt_ = log2_kt; *nleaf_max_ = nleaf_max;
    return vn_lds_need<T>(nij, nleaf_max, kt) <= (size_t)VN2_MAX_LDS;
}

static int vn_check_extents(int64_t n_cols, int32_t itot, int32_t jtot, int32_t ktot)
{
    if (n_cols < 0 || itot < 1 || jtot < 1 || ktot < 1 || (int64_t)itot * jtot > INT32_MAX / 2)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%svariability_nudge: bad extents");
    return SPC_OK;
}

// bytes of the transposed workspace: both planes (qt, qsat) of every level of every column
template <typename T> static int64_t vnudge_workspace_bytes(int64_t n_cols, int32_t itot, int32_t jtot, int32_t ktot)
{
    const int rc = vn_check_extents(n_cols, itot, jtot, ktot);
    return rc ? rc : n_cols * 2 * (int64_t)itot * jtot * ktot * (int64_t)sizeof(T);
}

// K6 for fields of T (double: spc_variability_nudge_f64; float: spc_variability_nudge_f32, the same struct with float fields
// and profiles, double R / beta / a_add)
template <typename T> static int vnudge_impl(const spc_vnudge_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = vn_check_extents(a->n_cols, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    if (a->n_cols == 0) return SPC_OK;
    REQUIRE(a->qt, "qt"); REQUIRE(a->qsat, "qsat"); REQUIRE(a->R, "R"); REQUIRE(a->ql_av, "ql_av"); REQUIRE(a->qt_av, "qt_av");
    REQUIRE(a->ql_ref, "ql_ref"); REQUIRE(a->beta, "beta"); REQUIRE(a->a_add, "a_add"); REQUIRE(a->qt_std, "qt_std");
    REQUIRE(a->status, "status");
    if (a->constantT) { REQUIRE(a->thl, "thl (constantT)"); REQUIRE(a->ql, "ql (constantT)"); REQUIRE(a->presf, "presf (constantT)"); }
    if (a->n_cols > 32767) return fail(SPC_ERR_UNSUPPORTED, "%svariability_nudge: more than 32767 columns per launch");
    VnPT<T> p;
    p.n_cols = a->n_cols; p.nij = a->itot * a->jtot; p.ktot = a->ktot; p.constantT = a->constantT; p.pad = 0;
    p.qsat = (const T *)a->qsat; p.R = (const double *)a->R; p.ql_av = (const T *)a->ql_av; p.qt_av = (const T *)a->qt_av;
    p.presf = (const T *)a->presf; p.ql_ref = (const T *)a->ql_ref; p.ql = (const T *)a->ql;
    p.qt = (T *)a->qt; p.thl = (T *)a->thl; p.beta = (double *)a->beta; p.a_add = (double *)a->a_add;
    p.qt_std = (T *)a->qt_std; p.status = a->status;
    // Where the planes live while the root finder runs: in the CU's LDS when KT levels' planes fit (KT x nij x 2 sizeof(T) <=
    // 150 KiB: up to ~9 000 points in double, ~18 000 in float; 64 x 64 planes: KT = 2), else -- double 128 x 128 and up,
    // float 136 x 136 and up -- in the caller's transposed workspace, one workgroup per level streaming its contiguous planes
    // (k_vnudge_solve<T, true>; SPC_VN_GLOBAL=1 forces it: tests).
    int kt, log2_kt, nleaf_max;
    const bool fits = vn_lds_fit<T>(p.nij, &kt, &log2_kt, &nleaf_max);
    if constexpr (std::is_same<T, float>::value) {
        // float planes where double ones fit too: the levels per workgroup of the double launch, not the twice as many the
        // LDS would hold -- those halve the workgroups and the threads per level and lose the register-cached R; measured on
        // 64 x 64 x 160 LES, the solve took 153 us at 2 LES and 2.50 ms at 256 against 78 us / 1.42 ms in double
        // (profiles/k6_f32.log).  Planes only float fits (~9 000 to ~18 000 points, 128 x 128) take KT = 1 from LDS.
        int kt64, log2_kt64, nleaf64;
        if (vn_lds_fit<double>(p.nij, &kt64, &log2_kt64, &nleaf64)) { kt = kt64; log2_kt = log2_kt64; }
    }
    const int64_t work_need = vnudge_workspace_bytes<T>(a->n_cols, a->itot, a->jtot, a->ktot);
    const bool have_work = a->work && a->work_bytes >= work_need && env_int("SPC_VN_TRANSPOSE", 1);
    const bool global = have_work && (!fits || env_int("SPC_VN_GLOBAL", 0));
    if (!fits && !have_work)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%svariability_nudge: planes of %lld points do not fit the LDS: `work` of "
                    "spc_vnudge_workspace_bytes() bytes is required", "", (long long)p.nij);
    auto lds_need = [&](int t) { return global ? (size_t)t * nleaf_max * 8 + VN2_THREADS * (sizeof(T) + 4) : vn_lds_need<T>(p.nij, nleaf_max, t); };
    // many workgroups (more than two rounds of one per CU): half the levels and half the threads per workgroup where
    // that lets TWO workgroups share a CU's LDS -- one's barriers and serial steps overlap the other's sums
    int nthreads = VN2_THREADS;
    if (global) { kt = 1; log2_kt = 0; }
    const int pair = env_int("SPC_VN_PAIR", 1);       // 0 never, 1 by workgroup count, 2 always (tests)
    if (!global && kt > 1 && lds_need(kt / 2) <= (size_t)(78 * 1024) &&
        (pair == 2 || (pair == 1 && a->n_cols * (int64_t)((a->ktot + kt - 1) / kt) > 512))) {
        kt >>= 1; --log2_kt; nthreads = VN2_THREADS / 2;
    }
    Vn2PT<T> q = {};
    q.p = p; q.kt = kt; q.log2_kt = log2_kt; q.nleaf_max = nleaf_max;
    for (int shape = 0; shape < 2; ++shape) {
        unsigned char ready[VN_MAXLEAF];
        vn_build_tree(shape == 0 ? 8192 : (p.nij % 8192 ? p.nij % 8192 : 8192), q.tab.lo[shape], q.tab.n[shape], q.tab.pl[shape],
                      q.tab.pr[shape], &q.tab.nleaf[shape]);
        q.tab.nround[shape] = vn_build_rounds(q.tab.nleaf[shape], q.tab.pl[shape], q.tab.pr[shape], q.tab.rnd[shape], ready);
        q.tab.balanced[shape] = vn_tree_balanced(q.tab.nleaf[shape], q.tab.pl[shape], q.tab.pr[shape], q.tab.rnd[shape]);
    }
    q.work = nullptr;
    if (have_work) {
        hipLaunchKernelGGL(k_vnudge_transpose<T>, dim3((unsigned)((p.nij + 63) / 64), (unsigned)((a->ktot + 15) / 16), (unsigned)(a->n_cols * 2)),
                           dim3(256), 0, (hipStream_t)stream, p, (T *)a->work);
        if ((rc = launch_status("k_vnudge_transpose"))) return rc;
        q.work = (const T *)a->work;
    }
    q.tiles = (a->ktot + kt - 1) / kt;
    q.tg = 16 / kt;                                       // tiles that share the 128-B lines of 16 levels
    q.gpc = (q.tiles + q.tg - 1) / q.tg;
    q.groups = a->n_cols * q.gpc;
    const size_t smem = lds_need(kt);
    // the noise plane in registers (k_vnudge_solve<T, false, true>): planes of one chunk with one leaf per 8-lane group
    const bool rcache = !global && p.nij <= 8192 && q.tab.nleaf[1] <= ((nthreads >> log2_kt) >> 3);
    void (*const solve)(const Vn2PT<T>) = global ? k_vnudge_solve<T, true> : (rcache ? k_vnudge_solve<T, false, true> : k_vnudge_solve<T, false>);
    if ((rc = ensure_lds(solve, smem, "variability_nudge"))) return rc;
    const int64_t nblk = (q.groups + 7) / 8 * 8 * q.tg;
    if (nblk > INT32_MAX) return fail(SPC_ERR_UNSUPPORTED, "%svariability_nudge: too many workgroups");
    hipLaunchKernelGGL(solve, dim3((unsigned)nblk), dim3(nthreads), smem, (hipStream_t)stream, q);
    if ((rc = launch_status("k_vnudge_solve"))) return rc;
    // the update (elementwise, wide) and qt.std (ordered sums, 16 levels per workgroup)
    const size_t usmem = (size_t)a->ktot * (sizeof(double) + 2 * sizeof(T) + sizeof(int));
    if ((rc = ensure_lds(k_vnudge_update<T>, usmem, "variability_nudge (update)"))) return rc;
    hipLaunchKernelGGL(k_vnudge_update<T>, dim3((unsigned)((p.nij + VU_ROWS - 1) / VU_ROWS), (unsigned)a->n_cols), dim3(256), usmem,
                       (hipStream_t)stream, p);
    if ((rc = launch_status("k_vnudge_update"))) return rc;
    const dim3 sgrid((unsigned)((a->ktot + 15) / 16), (unsigned)a->n_cols);
    const int rows = (int64_t)sgrid.x * sgrid.y <= 256 ? 512 : 256;
    void (*const kstd)(const VnPT<T>) = rows == 512 ? k_vnudge_std<T, 512> : k_vnudge_std<T, 256>;
    const size_t ssmem = (size_t)2 * rows * 16 * sizeof(T);
    if ((rc = ensure_lds(kstd, ssmem, "variability_nudge (std)"))) return rc;
    hipLaunchKernelGGL(kstd, sgrid, dim3(VS_THREADS), ssmem, (hipStream_t)stream, p);
    return launch_status("k_vnudge_std");
}
