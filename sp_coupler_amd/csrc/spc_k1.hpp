// spc_k1.hpp -- K1 k_forward (GCM state -> LES-level profiles and nudging forcings, with the fused index map, surface fluxes
// and rain rate) and K2 k_cloud_idx, K1's index map on its own.  Included by spc_hip.hip after spc_device.hpp; the float form
// with 8-byte accesses is spc_f32v.hpp, the tables and rules that pick an instantiation are in spc_launch.hpp.
#pragma once

// =================================================================================================
// K1 forward: splib/spcpl.py:171-246 (convert_profiles) + 299-385 (set_les_forcings) for CB columns
// per workgroup; optional fused K2 (spcpl.py:764) and surface fluxes (spcpl.py:136-167).
// LDS per column: xp=Zf reversed | thl_ | qt_ | QL | U | V, each [nG] in ascending-height order;
// then (idx only) zh: [nL] when the LES grid is shared, else [CB x nL].
// =================================================================================================
// LES-side inputs of one output level (loaded early so their latency hides behind phase 1)
template <typename T> struct LesIn {
    T h, ud, vd, thld, qtd, qld;
};

template <typename P, typename T = decltype(+*P().zf)>
__device__ __forceinline__ LesIn<T> load_les(const P &p, int l, int64_t o)
{
    LesIn<T> r;
    r.h = p.d.shared_grid ? ldg(&p.zf[l]) : ldg(&p.zf[o]);                                        // spcpl.py:222
    r.ud = ldg(&p.u_d[o]); r.vd = ldg(&p.v_d[o]); r.thld = ldg(&p.thl_d[o]); r.qtd = ldg(&p.qt_d[o]); r.qld = ldg(&p.ql_d[o]);
    return r;
}

constexpr int cfloor_pow2(int n) { int p = 1; while (p <= n / 2) p *= 2; return p; }   // (p * 2 <= n overflows from n = 2^30 on: the loop never ended)

// NG / NL != 0: level counts fixed at compile time and contiguous columns (pitch == level count): the
// flat-index divisions become multiply-shifts, the searches unroll, no pitch registers (hot geometries
// 91<->160, 137<->512, 19<->160); NG == NL == 0: everything from DimsP at run time.
// BLK: workgroup size.  256 everywhere except the small-batch path (small_block()): there one workgroup of 512 / 1024
// threads takes 2 / 4 columns, still one work item per thread, so that <= 256 workgroups cover the batch.
// PRE: issue the first work item's LES-side inputs and the per-column scalars in the prologue, so that ONE memory round
//      trip covers them and the GCM slab: what a single-round launch (<= 1024 columns) needs.  Multi-round launches run
//      with PRE = false: those ~20 registers are live across phase 1, whose pow() sets the kernel's register peak, and
//      without them K1 fits 6 waves per SIMD instead of 5 (75 vs 94 VGPRs) -- K1's rate follows its resident waves
//      (profiles/r02_occupancy_ab_hot.log): -7 % at 35 718 columns, +12 % at 1024 (profiles/r02_k1_occupancy6_ab.log).
//      PRE = false is also the REACH form (phase 1 split at the LES interpolation's reach, below): one more dependent
//      round trip per workgroup, which a multi-round launch hides behind its other resident workgroups.  A reach-form
//      workgroup is bound by the round trips it makes one after another, so in the lean double kernels (FOLD) the small
//      ones ride on phase A's: a thread's first two phase-A items, its first LES grid entries, the half levels of the
//      index map and the f_ps inputs are ONE trip, and the index entries and f_ps are written between the two barriers
//      of the reach search.
template <typename T, bool FULL, int NG, int NL, int WT, int BLK = BLOCK, bool PRE = true>
__global__ __launch_bounds__(BLK) void k_forward(const FwdP<T, FULL> p)
{
    const DimsP &d = p.d;
    // The ~20 optional pointers of the FULL variant are fetched from the kernarg block where they are used (a
    // volatile scalar load each) instead of living in SGPRs for the whole kernel: 68 -> few SGPR spills.
#define OPT(f) (*(decltype(FwdOpt<T>::f) const volatile __attribute__((address_space(4))) *)( \
    (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(FwdFull<T>, o) + offsetof(FwdOpt<T>, f)))
    const int nG = NG ? NG : d.nG, nL = NL ? NL : d.nL, cb = d.cb;
    const int64_t pitchG = NG ? NG : d.pitchG, pitchGh = NG ? NG + 1 : d.pitchGh, pitchL = NL ? NL : d.pitchL;
    const int p2G = NG ? cfloor_pow2(NG ? NG : 1) : d.p2G;
    const int tid = threadIdx.x;
    const int64_t col0 = (int64_t)slab_index(d.xcd_remap) * cb;
    const int ncol = (int)((d.n_cols - col0) < cb ? (d.n_cols - col0) : cb);
    T *const lds = reinterpret_cast<T *>(spc_smem);
    T *const lzh = lds + (size_t)cb * 6 * nG;
    // work items after the barrier: [0, n2) LES levels to interpolate, [n2, n2 + nI) index-map entries
    constexpr bool REACH = !PRE;
    // FOLD: the lean double reach form rides its small round trips on phase A's (below).  The FULL and the float reach forms keep
    // one trip per loop round: folded, two FULL instantiations gain scalar spills and the float ones 4-14 VGPRs.
    constexpr bool FOLD = REACH && !FULL && sizeof(T) == 8;
    constexpr int NE = FOLD ? 2 : 0;              // phase-A items per thread whose loads are issued before the first wait
    constexpr int HELD = NE * BLK;                // the index entries of phase-A items < HELD are written in the reach gap
    const int n1 = ncol * nG, n2 = ncol * nL, nI = p.idx ? (n1 > HELD ? n1 - HELD : 0) : 0, nitems = n2 + nI;
    // one fused-K2 entry (spcpl.py:764) and one f_ps (spcpl.py:332): the reach gap and the one-phase path share them
    auto put_idx = [&](int c, int64_t col, int m, T Zh_k) {
        const T *const zh = d.shared_grid ? lzh : lzh + (size_t)c * nL;
        p.idx[col * pitchG + m] = ss_right(zh, nL, Zh_k);
    };
    auto put_f_ps = [&](int64_t col, T sc_ps, T sc_psd) {
        stg<WT>(&p.f_ps[col], Divisor<T>(p.dt).div(p.factor * (sc_ps - sc_psd)));          // spcpl.py:332
    };
    STAMP(0);

    // ---- prologue: issue every load that depends on nothing, so ONE memory round trip covers the
    //      GCM slab, this thread's first work item and the per-column scalars.  (Issuing the GCM loads
    //      FIRST -- the order of need -- was A/B-tested: +4 % slower here, while the same reordering
    //      gains 4.5 % in K3.) ---------------------------------------------------------------------
    LesIn<T> pre2 = {};
    T pre_zgh = T(0), pre_zs = T(0);
    if (!PRE) {
    } else if (tid < n2) {
        const int c = tid / nL, l = tid - c * nL;
        pre2 = load_les<FwdP<T, FULL>, T>(p, l, (col0 + c) * pitchL + l);
    } else if (tid < nitems) {
        const int ei = tid - n2, c = ei / nG, m = ei - c * nG;
        const int64_t gh = (col0 + c) * pitchGh;
        pre_zgh = ldg(&p.Zghalf[gh + (nG - 1 - m)]);
        pre_zs = ldg(&p.Zghalf[gh + nG]);
    }
    const int sc = BLK - 1 - tid;          // the LAST threads own the per-column scalars
    T sc_ps = T(0), sc_psd = T(0), sc_rain = T(0), sc_rl = T(0);
    if (PRE && sc < ncol) {
        sc_ps = ldg(&p.Ph[(col0 + sc) * pitchGh + nG]);                                   // spcpl.py:246
        sc_psd = ldg(&p.ps_d[col0 + sc]);
        if constexpr (FULL)
            if (OPT(rainrate)) { sc_rain = OPT(rain)[col0 + sc]; sc_rl = OPT(rain_last)[col0 + sc]; }
    }
    if (PRE && p.idx) {  // stage the LES half levels for the fused index map (REACH: with phase A's loads, below)
        const int nz = d.shared_grid ? nL : n2;
        for (int e = tid; e < nz; e += BLK) {
            const int c = e / nL, l = e - c * nL;
            lzh[e] = d.shared_grid ? p.zh[e] : p.zh[(col0 + c) * pitchL + l];
        }
    }
    STAMP(1);

    // ---- phase 1: load GCM levels (flat over the [ncol x nG] slab), convert, stage reversed ----
    // REACH (multi-round launches, PRE = false): phase 1 is split in two.  Phase A stages Zf for every level and takes the
    // largest non-NaN LES height of the slab; one search of that height in each column's Zf then bounds every bracket
    // phase 2 can form (reach_top), and phase B loads and converts the other 7 fields only for the levels 0 ... top (in
    // ascending-height order).  Exact for any input: upper_count is monotone in x for ANY xp (a lane with the larger x
    // takes every branch the smaller one takes), so j0(x) <= j0(hmax) and j1(x) <= min(j0(hmax) + 1, nG - 1) for every
    // non-NaN x <= hmax, and a NaN height takes level 0.  LDS above the reach is never written nor read.
    // FOLD: phase A issues, before its first wait, every load of a thread's first items: LES half level tid (index map),
    // phase-A items tid and tid + BLK (with their own half level when the index map is fused), LES height tid and, on the
    // lanes that own a column's scalars, the f_ps inputs.  Later items (larger slabs, 137<->512) keep one trip per loop
    // round.  The index entries of the held items and f_ps are written between the two barriers of the reach search, which
    // the lanes with the fewest held items run (the LAST ncol); phase 2 carries the index entries of phase-A items >= HELD.
    int nR = nG;                                   // levels staged per column: the nR lowest (REACH) or all
    if constexpr (REACH) {
        __shared__ T s_wmax[BLK / 64];
        __shared__ int s_top;
        if (tid == 0) s_top = 0;
        const int nz = d.shared_grid ? nL : n2;           // LES grid entries this slab reads
        auto grid_at = [&](const T *q, int e) {
            const int c = e / nL, l = e - c * nL;
            return d.shared_grid ? ldg(&q[e]) : ldg(&q[(col0 + c) * pitchL + l]);
        };
        // (branch-free, so that no load waits for another: a lane without an item repeats the slab's last one, a launch
        //  without the index map reads zf and Zghalf[nG] once more -- lines the workgroup fetches anyway)
        T zh0 = T(0), h0 = T(0), a_zg[2] = {}, a_zs[2] = {}, a_zh[2] = {}, held[2] = {};
        if constexpr (FOLD) {
            const int tz = tid < nz ? tid : nz - 1;
            zh0 = grid_at(p.idx ? p.zh : p.zf, tz);
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int e = tid + u * BLK < n1 ? tid + u * BLK : n1 - 1, c = e / nG, k = e - c * nG;
                const int64_t col = col0 + c;
                a_zg[u] = ldg(&p.Zgfull[col * pitchG + k]);
                a_zs[u] = ldg(&p.Zghalf[col * pitchGh + nG]);
                a_zh[u] = ldg(&p.Zghalf[col * pitchGh + (p.idx ? k : nG)]);
            }
            h0 = grid_at(p.zf, tz);
            if (sc < ncol) {
                sc_ps = ldg(&p.Ph[(col0 + sc) * pitchGh + nG]);                               // spcpl.py:246
                sc_psd = ldg(&p.ps_d[col0 + sc]);
            }
        }
        if (p.idx) {  // stage the LES half levels for the fused index map
            if (FOLD && tid < nz) lzh[tid] = zh0;
            for (int e = tid + (FOLD ? BLK : 0); e < nz; e += BLK) lzh[e] = grid_at(p.zh, e);
        }
        auto stage_zf = [&](int c, int k, int64_t g, T zg, T zs) {
            const T zf_k = div_grav(zg - zs);                                                  // spcpl.py:198
            lds[(size_t)c * 6 * nG + (nG - 1 - k)] = zf_k;                                     // [::-1], spcpl.py:224
            if constexpr (FULL)
                if (OPT(Zf)) OPT(Zf)[g] = zf_k;                                                 // spcpl.py:200
        };
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            const int e = tid + u * BLK;
            if (e < n1) {
                const int c = e / nG, k = e - c * nG;
                stage_zf(c, k, (col0 + c) * pitchG + k, a_zg[u], a_zs[u]);
                if (p.idx) held[u] = div_grav(a_zh[u] - a_zs[u]);                              // spcpl.py:197
            }
        }
        for (int e = tid + HELD; e < n1; e += BLK) {
            const int c = e / nG, k = e - c * nG;
            const int64_t col = col0 + c, g = col * pitchG + k;
            stage_zf(c, k, g, ldg(&p.Zgfull[g]), ldg(&p.Zghalf[col * pitchGh + nG]));
        }
        T hmax = T(-__builtin_huge_val());
        if (FOLD && tid < nz) hmax = h0 > hmax ? h0 : hmax;                                    // NaN never wins
        for (int e = tid + (FOLD ? BLK : 0); e < nz; e += BLK) {
            const T h = grid_at(p.zf, e);
            hmax = h > hmax ? h : hmax;
        }
        for (int m = 32; m > 0; m >>= 1) {
            const T o = __shfl_xor(hmax, m, 64);
            hmax = o > hmax ? o : hmax;
        }
        if ((tid & 63) == 0) s_wmax[tid >> 6] = hmax;
        __syncthreads();
        const int rs = FOLD ? sc : tid;                   // the lane of column rs searches its reach
        if (rs < ncol) {
            for (int w = 0; w < BLK / 64; ++w) hmax = s_wmax[w] > hmax ? s_wmax[w] : hmax;
            const Br<T> b = bracket2(lds + (size_t)rs * 6 * nG, nG, p2G, hmax);
            atomicMax(&s_top, b.j0 + 1 >= nG ? nG - 1 : b.j0 + 1);
            if constexpr (FOLD) put_f_ps(col0 + sc, sc_ps, sc_psd);
        }
        if (FOLD && p.idx) {
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int e = tid + u * BLK;
                if (e < n1) {
                    const int c = e / nG, k = e - c * nG;
                    put_idx(c, col0 + c, nG - 1 - k, held[u]);
                }
            }
        }
        __syncthreads();
        nR = s_top + 1;
    }
    const float rcp_nR = 1.0f / (float)nR;
    for (int e = tid; e < ncol * nR; e += BLK) {
        int c, k;
        if constexpr (REACH) {         // e -> (column, level) for a run-time nR: float quotient, off by at most one
            c = (int)((float)e * rcp_nR);
            int r = e - c * nR;
            if (r < 0) { --c; r += nR; } else if (r >= nR) { ++c; r -= nR; }
            k = nG - nR + r;
        } else {
            c = e / nG; k = e - c * nG;
        }
        const int64_t col = col0 + c, g = col * pitchG + k;
        const T zsurf = REACH ? T(0) : ldg(&p.Zghalf[col * pitchGh + nG]);
        const T tt = ldg(&p.Tm[g]), sh = ldg(&p.SH[g]), ql = ldg(&p.QL[g]), qi = ldg(&p.QI[g]), pf = ldg(&p.Pf[g]);
        const T zg = REACH ? T(0) : ldg(&p.Zgfull[g]);
        const T uu = ldg(&p.U[g]), vv = ldg(&p.V[g]);
        T *const s = lds + (size_t)c * 6 * nG + (nG - 1 - k);                         // [::-1], spcpl.py:224
        if constexpr (!REACH) {
            const T zf_k = div_grav(zg - zsurf);                                      // spcpl.py:198
            s[0] = zf_k;
            if constexpr (FULL)
                if (OPT(Zf)) OPT(Zf)[g] = zf_k;                                         // spcpl.py:200
        }
        s[2 * nG] = sh + ql + qi;                                                       // spcpl.py:215
        s[3 * nG] = ql;
        s[4 * nG] = uu;
        s[5 * nG] = vv;
        const T iex = spc_pow(div_pref0(pf), (-K<T>::rd) / K<T>::cp);                   // sputils.py:34
        s[nG] = (tt - div_cp(K<T>::rlv * (ql + qi))) * iex;                             // spcpl.py:214
    }
    STAMP(2);
    __syncthreads();
    STAMP(3);

    // ---- per-column scalars (inputs already in registers; stores drain behind phase 2) ----------
    if (!FOLD && sc < ncol) {
        const int64_t col = col0 + sc;
        if (!PRE) {
            sc_ps = ldg(&p.Ph[col * pitchGh + nG]); sc_psd = ldg(&p.ps_d[col]);             // spcpl.py:246
            if constexpr (FULL)
                if (OPT(rainrate)) { sc_rain = OPT(rain)[col]; sc_rl = OPT(rain_last)[col]; }
        }
        put_f_ps(col, sc_ps, sc_psd);
        if constexpr (FULL) {
            if (OPT(ps)) OPT(ps)[col] = sc_ps;
            if (OPT(rainrate)) OPT(rainrate)[col] = (sc_rain - sc_rl) / p.dt;           // spcpl.py:325
            if (OPT(wthl)) {                                                            // spcpl.py:136-167
                const T rho = sc_ps / (K<T>::rd * ldg(&p.Tm[col * pitchG + (nG - 1)]));      // spcpl.py:153
                OPT(wqt)[col] = -(OPT(QLflux)[col] + OPT(QIflux)[col] + OPT(SHflux)[col]) / rho;     // spcpl.py:159
                OPT(wthl)[col] = -OPT(TSflux)[col] * spc_pow(div_pref0(sc_ps), (-K<T>::rd) / K<T>::cp)
                                / (K<T>::cp * rho);                                    // spcpl.py:161
                if (OPT(z0m)) OPT(z0m)[col] = OPT(Z0M)[col];
                if (OPT(z0h)) OPT(z0h)[col] = OPT(Z0H)[col];
            }
        }
    }

    // ---- phase 2: LES levels (interpolate 5 fields, form the forcings) and index-map entries ------
    const Divisor<T> ddt(p.dt);
    for (int e = tid; e < nitems; e += BLK) {
        if (e < n2) {
            const int c = e / nL, l = e - c * nL;
            const int64_t col = col0 + c, o = col * pitchL + l;
            const T *const s = lds + (size_t)c * 6 * nG;
            const LesIn<T> in = (PRE && e == tid) ? pre2 : load_les<FwdP<T, FULL>, T>(p, l, o);
            const Br<T> b = bracket2(s, nG, p2G, in.h);
            T f0[5], f1[5], r[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                f0[k] = s[(k + 1) * nG + b.j0];
                f1[k] = s[(k + 1) * nG + b.j1];
            }
            interp_fields<5>(b, f0, f1, r);
            const T thl = r[0], qt = r[1], ql = r[2], u = r[3], v = r[4];               // spcpl.py:224-228
            stg<WT>(&p.f_u[o], ddt.div(p.factor * (u - in.ud)));               // spcpl.py:328
            stg<WT>(&p.f_v[o], ddt.div(p.factor * (v - in.vd)));               // spcpl.py:329
            stg<WT>(&p.f_thl[o], ddt.div(p.factor * (thl - in.thld)));         // spcpl.py:330
            stg<WT>(&p.f_qt[o], ddt.div(p.factor * (qt - in.qtd)));            // spcpl.py:331
            stg<WT>(&p.f_ql[o], ddt.div(p.factor * (ql - in.qld)));            // spcpl.py:333
            stg<WT>(&p.ql_ref[o], ql);                                                         // spcpl.py:347-348
            if constexpr (FULL) {
                if (OPT(u)) OPT(u)[o] = u;
                if (OPT(v)) OPT(v)[o] = v;
                if (OPT(thl)) OPT(thl)[o] = thl;
                if (OPT(qt)) OPT(qt)[o] = qt;
            }
        } else {                                                                      // fused K2, spcpl.py:764
            // entry (c, m); FOLD: the entry of phase-A item ei = (c, k), m = nG - 1 - k
            const int ei = e - n2 + HELD, c = ei / nG, r = ei - c * nG, m = FOLD ? nG - 1 - r : r;
            const int64_t col = col0 + c, gh = col * pitchGh;
            const T zgh = (PRE && e == tid) ? pre_zgh : ldg(&p.Zghalf[gh + (nG - 1 - m)]);
            const T zs = (PRE && e == tid) ? pre_zs : ldg(&p.Zghalf[gh + nG]);
            const T Zh_k = div_grav(zgh - zs);                                        // spcpl.py:197
            put_idx(c, col, m, Zh_k);
        }
    }
    STAMP(4);

    // ---- half-level heights (optional output): spcpl.py:197 --------------------------------------
    if constexpr (FULL) {
        if (OPT(Zh)) {
            for (int e = tid; e < ncol * (nG + 1); e += BLK) {
                const int c = e / (nG + 1), k = e - c * (nG + 1);
                const int64_t gh = (col0 + c) * pitchGh;
                OPT(Zh)[gh + k] = div_grav(ldg(&p.Zghalf[gh + k]) - ldg(&p.Zghalf[gh + nG]));
            }
        }
    }
    STAMP(5);
#undef OPT
}

// =================================================================================================
// K2 standalone: splib/spcpl.py:26 / 764
// =================================================================================================
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_cloud_idx(const DimsP d, const T *zh_, const T *Zh_, int32_t *idx)
{
    const int nG = d.nG, nL = d.nL, cb = d.cb, tid = threadIdx.x;
    const int64_t col0 = (int64_t)slab_index(d.xcd_remap) * cb;
    const int ncol = (int)((d.n_cols - col0) < cb ? (d.n_cols - col0) : cb);
    T *const lzh = reinterpret_cast<T *>(spc_smem);
    const int nz = d.shared_grid ? nL : ncol * nL;
    for (int e = tid; e < nz; e += BLOCK) {
        const int c = e / nL, l = e - c * nL;
        lzh[e] = d.shared_grid ? zh_[e] : zh_[(col0 + c) * d.pitchL + l];
    }
    __syncthreads();
    for (int e = tid; e < ncol * nG; e += BLOCK) {
        const int c = e / nG, m = e - c * nG;
        const int64_t col = col0 + c;
        const T *const zh = d.shared_grid ? lzh : lzh + (size_t)c * nL;
        idx[col * d.pitchG + m] = ss_right(zh, nL, Zh_[col * d.pitchGh + (nG - 1 - m)]);
    }
}
