// spc_k3.hpp -- K3 k_backward (LES slab means -> GCM tendencies, masked above the LES top).  Included by spc_hip.hip after
// spc_k1.hpp (cfloor_pow2); the conservative form K4 is spc_k4.hpp, the tables and rules that pick an instantiation are in
// spc_launch.hpp.
#pragma once

// =================================================================================================
// K3 backward: splib/spcpl.py:388-555, linear branch (468-478) + start_index (498) + tendencies
// (518-526) + masking (527-533).  LDS per column: t | qt | ql | ql_ice | u | v, each [nL]; then
// Zf [nG]; then h: [nL] when the LES grid is shared, else [CB x nL].
// =================================================================================================
template <typename T> struct GcmIn {
    T tt, sh, ql, qi, u, v, a, a_d;
};

template <typename T> __device__ __forceinline__ GcmIn<T> load_gcm(const BwdP<T> &p, int64_t g, int64_t g_rev)
{
    GcmIn<T> r;
    r.tt = ldg(&p.Tm[g]); r.sh = ldg(&p.SH[g]); r.ql = ldg(&p.QL[g]); r.qi = ldg(&p.QI[g]); r.u = ldg(&p.U[g]); r.v = ldg(&p.V[g]); r.a = ldg(&p.A[g]);
    r.a_d = ldg(&p.A_prof[g_rev]);                                                           // spcpl.py:404
    return r;
}

// PRE: the GCM-side inputs of a thread's first output level are loaded in the prologue (one memory round trip for a
// single-round launch).  Without it K3 needs 60 instead of 78 VGPRs (8 waves per SIMD instead of 6): +4-7 % at 2-4 k
// columns, nothing from 16 k on where K3 has saturated (profiles/r02_k3_pre_ab.log) -- used between 1 025 and 25 000 columns.
template <typename T, int NG, int NL, int WT, int BLK = BLOCK, bool PRE = true> __global__ __launch_bounds__(BLK) void k_backward(const BwdP<T> p)
{
    const DimsP &d = p.d;
    const int nG = NG ? NG : d.nG, nL = NL ? NL : d.nL, cb = d.cb, tid = threadIdx.x;
    const int64_t pitchG = NG ? NG : d.pitchG, pitchGh = NG ? NG + 1 : d.pitchGh, pitchL = NL ? NL : d.pitchL;
    const int p2L = NL ? cfloor_pow2(NL ? NL : 1) : d.p2L;
    const int64_t col0 = (int64_t)slab_index(d.xcd_remap) * cb;
    const int ncol = (int)((d.n_cols - col0) < cb ? (d.n_cols - col0) : cb);
    const size_t per_col = (size_t)6 * nL + nG;
    T *const lds = reinterpret_cast<T *>(spc_smem);
    T *const lh = lds + (size_t)cb * per_col;
    const int n1 = ncol * nG;
    STAMP(0);

    // Loads are issued in the order the data is NEEDED (memory returns roughly in issue order and
    // s_waitcnt vmcnt counts in issue order): first this thread's first staging element of every LES array
    // and of Zf, which the LDS writes in front of the barrier wait for; then the GCM-side inputs of its
    // first output level, which land while the staging completes.
    struct Stage { T t, qt, ql, qi, u, v, h; };
    auto load_stage = [&](int64_t o) {
        Stage r;
        r.t = ldg(&p.t_d[o]); r.qt = ldg(&p.qt_d[o]); r.ql = ldg(&p.ql_d[o]); r.qi = ldg(&p.ql_ice_d[o]);
        r.u = ldg(&p.u_d[o]); r.v = ldg(&p.v_d[o]);
        r.h = d.shared_grid ? T(0) : ldg(&p.zf[o]);
        return r;
    };
    auto load_zf = [&](int64_t col, int64_t g) {
        return p.Zf ? p.Zf[g] : div_grav(ldg(&p.Zgfull[g]) - ldg(&p.Zghalf[col * pitchGh + nG]));   // spcpl.py:198
    };
    const int n2 = ncol * nL;
    Stage st0 = {};
    T zf0 = T(0), hs0 = T(0);
    if (tid < n2) {
        const int c = tid / nL, l = tid - c * nL;
        st0 = load_stage((col0 + c) * pitchL + l);
    }
    if (tid < n1) {
        const int c = tid / nG, k = tid - c * nG;
        zf0 = load_zf(col0 + c, (col0 + c) * pitchG + k);
    }
    if (d.shared_grid && tid < nL) hs0 = ldg(&p.zf[tid]);
    // SPARE (PRE, 256 threads, one item per loop round): the waves behind the last GCM item have no use for `pre`.  Where
    // their lanes can take EVERY staging item from BLK on, they load them in this same round trip into pre's registers (one
    // variable: no register is added) and write them to LDS behind the staging loop, which then ends at BLK: at 91<->160
    // with two columns the second staging round, 64 items on wave 0 with three waves waiting at the barrier, is gone.
    // (Sharing the later items between spare lanes and loop was measured too: 137<->512 at one column, +2.4 %.)
    constexpr bool SPARE = PRE && sizeof(T) == 8 && BLK == BLOCK;   // (512 / 1024 threads: one item per thread, nothing later)
    const int spare0 = (n1 + 63) & ~63;                                     // first lane of the waves without a GCM item
    const bool spare = SPARE && n2 > BLK && n2 - BLK <= BLK - spare0;
    const int n2l = spare ? BLK : n2;                                       // staging items of the loop
    GcmIn<T> pre = {};
    if (PRE && tid < n1) {
        const int c = tid / nG, k = tid - c * nG;
        const int64_t cg = (col0 + c) * pitchG;
        pre = load_gcm(p, cg + k, cg + (nG - 1 - k));
    } else if (spare && tid >= spare0 && BLK + (tid - spare0) < n2) {
        const int e = BLK + (tid - spare0), c = e / nL, l = e - c * nL;
        const Stage sp = load_stage((col0 + c) * pitchL + l);
        pre.tt = sp.t; pre.sh = sp.qt; pre.ql = sp.ql; pre.qi = sp.qi; pre.u = sp.u; pre.v = sp.v; pre.a = sp.h;
    }
    STAMP(1);

    // UF work items per thread and loop round, all their loads issued before the first is used: 1 for double (the form of
    // rounds 1-4), 2 for float -- a 4-byte access puts half the bytes in flight.  Measured (profiles/r05_f32_ab.log): K3<float>
    // -5 % at config 3 with the quotients through fp64; the same scheme in K1<float> was SLOWER (86 against 78-80 us:
    // 63 instead of 48 VGPRs and 8 scalar spills) and is not used there.
    constexpr int UF = sizeof(T) == 4 ? 2 : 1;
    for (int e0 = tid; e0 < n2l; e0 += UF * BLK) {
        Stage st[UF];
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            const int e = e0 + u * BLK;
            if (e < n2l) {
                const int c = e / nL, l = e - c * nL;
                st[u] = (e == tid) ? st0 : load_stage((col0 + c) * pitchL + l);
            }
        }
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            const int e = e0 + u * BLK;
            if (e < n2l) {
                const int c = e / nL, l = e - c * nL;
                T *const s = lds + (size_t)c * per_col + l;
                s[0] = st[u].t;
                s[nL] = st[u].qt;
                s[2 * nL] = st[u].ql;
                s[3 * nL] = st[u].qi;
                s[4 * nL] = st[u].u;
                s[5 * nL] = st[u].v;
                if (!d.shared_grid) lh[e] = st[u].h;
            }
        }
    }
    if (spare && tid >= spare0 && BLK + (tid - spare0) < n2) {              // the items the spare lanes hold in `pre`
        const int e = BLK + (tid - spare0), c = e / nL, l = e - c * nL;
        T *const s = lds + (size_t)c * per_col + l;
        s[0] = pre.tt;
        s[nL] = pre.sh;
        s[2 * nL] = pre.ql;
        s[3 * nL] = pre.qi;
        s[4 * nL] = pre.u;
        s[5 * nL] = pre.v;
        if (!d.shared_grid) lh[e] = pre.a;
    }
    if (d.shared_grid)
        for (int e = tid; e < nL; e += BLK) lh[e] = (e == tid) ? hs0 : ldg(&p.zf[e]);
    for (int e = tid; e < n1; e += BLK) {
        const int c = e / nG, k = e - c * nG;
        const int64_t col = col0 + c;
        lds[(size_t)c * per_col + 6 * nL + k] = (e == tid) ? zf0 : load_zf(col, col * pitchG + k);
    }
    STAMP(2);
    __syncthreads();
    STAMP(3);

    const Divisor<T> ddt(p.dt);
    auto gcm_item = [&](int e, const GcmIn<T> &in) {
        const int c = e / nG, k = e - c * nG;
        const int64_t col = col0 + c, cg = col * pitchG, g = cg + k;
        const T *const s = lds + (size_t)c * per_col;
        const T *const h = d.shared_grid ? lh : lh + (size_t)c * nL;
        const T *const Zf = s + 6 * nL;
        const T x = Zf[k];
        const int start_index = ss_left_neg(Zf, nG, h[nL - 1]);                        // spcpl.py:498
        // (the branch-light interp_fields<7> form was measured here too: no gain at 1024 columns and -12 % at
        //  >= 35k columns, because interleaving 7 division chains costs 118 VGPRs and a third of the occupancy)
        const Bracket<T> b = bracket(h, nL, p2L, x);
        T t_i, qt_i, ql_i, qlw_i, qli_i, u_i, v_i;
        if (b.mode == 0) {
            const int j = b.j;
            const T ql0 = s[2 * nL + j], ql1 = s[2 * nL + j + 1], qi0 = s[3 * nL + j], qi1 = s[3 * nL + j + 1];
            const Divisor<T> dx(b.x1 - b.x0);
            t_i = lerp_np(x, b.x0, b.x1, s[j], s[j + 1], dx);                          // spcpl.py:471
            qt_i = lerp_np(x, b.x0, b.x1, s[nL + j], s[nL + j + 1], dx);               // spcpl.py:472
            ql_i = lerp_np(x, b.x0, b.x1, ql0, ql1, dx);                               // spcpl.py:473
            qlw_i = lerp_np(x, b.x0, b.x1, ql0 - qi0, ql1 - qi1, dx);                  // spcpl.py:402,474
            qli_i = lerp_np(x, b.x0, b.x1, qi0, qi1, dx);                              // spcpl.py:475
            u_i = lerp_np(x, b.x0, b.x1, s[4 * nL + j], s[4 * nL + j + 1], dx);        // spcpl.py:476
            v_i = lerp_np(x, b.x0, b.x1, s[5 * nL + j], s[5 * nL + j + 1], dx);        // spcpl.py:477
        } else if (b.mode == 1) {
            const int j = b.j;
            t_i = s[j];
            qt_i = s[nL + j];
            ql_i = s[2 * nL + j];
            qli_i = s[3 * nL + j];
            qlw_i = ql_i - qli_i;
            u_i = s[4 * nL + j];
            v_i = s[5 * nL + j];
        } else {
            t_i = qt_i = ql_i = qlw_i = qli_i = u_i = v_i = x;
        }
        T f_T = ddt.div(p.factor * (t_i - in.tt));                                        // spcpl.py:518
        T f_SH = ddt.div(p.factor * ((qt_i - ql_i) - in.sh));                            // spcpl.py:519
        T f_QL = ddt.div(p.factor * (qlw_i - in.ql));                                    // spcpl.py:520
        T f_QI = ddt.div(p.factor * (qli_i - in.qi));                                    // spcpl.py:521
        T f_U = ddt.div(p.factor * (u_i - in.u));                                         // spcpl.py:524
        T f_V = ddt.div(p.factor * (v_i - in.v));                                        // spcpl.py:525
        T f_A = ddt.div(p.factor * (in.a_d - in.a));                                     // spcpl.py:526
        if (k < start_index) {  // `f[0:start_index] *= 0` (spcpl.py:527-533): -x -> -0, NaN stays NaN
            const T zero = T(0);
            f_T *= zero; f_SH *= zero; f_QL *= zero; f_QI *= zero; f_U *= zero; f_V *= zero; f_A *= zero;
        }
        stg<WT>(&p.f_T[g], f_T);
        stg<WT>(&p.f_SH[g], f_SH);
        stg<WT>(&p.f_QL[g], f_QL);
        stg<WT>(&p.f_QI[g], f_QI);
        stg<WT>(&p.f_U[g], f_U);
        stg<WT>(&p.f_V[g], f_V);
        stg<WT>(&p.f_A[g], f_A);
        if (p.start_index && k == 0) p.start_index[col] = start_index;
    };
    for (int e0 = tid; e0 < n1; e0 += UF * BLK) {
        GcmIn<T> in[UF];
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            const int e = e0 + u * BLK;
            if (e < n1) {
                const int c = e / nG, k = e - c * nG;
                const int64_t cg = (col0 + c) * pitchG;
                in[u] = (PRE && e == tid) ? pre
                                          : load_gcm(p, cg + k, cg + (nG - 1 - k));
            }
        }
#pragma unroll
        for (int u = 0; u < UF; ++u)
            if (e0 + u * BLK < n1) gcm_item(e0 + u * BLK, in[u]);
    }
    STAMP(4);
    STAMP(5);
}
