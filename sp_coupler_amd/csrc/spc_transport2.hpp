// spc_transport2.hpp -- K23: K22's unsplit flux-form step with a SECOND-ORDER face value: every face carries K22's donor-cell
// flux plus a correction from the (limited) slope of its upwind cell, centred in time.  Kernel and host side; spc_hip.hip
// includes it twice, like spc_transport.hpp, and after it both times: the parameter block LesTransportP, trn_neighbours,
// trn_faces and the probe launch are K22's, the tile, the chain and the atomicMax K17's, all unchanged.
//
// The rule (include/spc.h) per cell, in T, one rounding per operation, never an fma, no division, selects only.  Everything up
// to K22's twelve numbers pw, qw, ..., pt, qt and its six donor fluxes Fw ... Ft is K22's, bit for bit; so are mtop and cmax.
//   slope of a cell along an axis, m / p its neighbours there (periodic along i and j; along k +0 at k == 0 and k == ktot - 1):
//     a = x - x[m];  b = x[p] - x;  t = a + b;  c0 = 0.5 * t
//     NONE: s = c0      MC: a, b > 0: s = min(c0, min(2a, 2b));  a, b < 0: s = max(c0, max(2a, 2b));  otherwise +0
//   Aw = 0.5 * (pw * (1 - pw) * si[im] - qw * (1 + qw) * si[i]);   Ae = 0.5 * (pe * (1 - pe) * si[i] - qe * (1 + qe) * si[ip])
//   As, An likewise with sj;  vertical faces with the Courant number of the upwind cell:
//   At = 0.5 * (pt * (1 - pt * r[k]) * sk[k] - qt * (1 + qt * r[kp]) * sk[k + 1]);   Ab is At of k - 1
//   F.2 = F. + A.;   x' = (x - ((Fe2 - Fw2) + (Fn2 - Fs2))) - r[k] * (Ft2 - Fb2);   ftop = Ft2 at the lid
// Both cells of a face form its correction from the same operands in the same order (the slope of a neighbour is formed by the
// statements the neighbour uses for its own), so the conservation of K22 holds.
//
// The shape is K22's: phases 1 and 2 are its phases; phase 3 loads per field the cell and its neighbours at distance 1 and 2
// along each axis, 13 values.  Along k and j they lie in the workgroup's own contiguous run or next to it, the rows i +- 1 and
// i +- 2 come from the caches as K22's i +- 1 do: the HBM traffic stays 2 + 2 NF passes.  Along k every index is clamped
// BEFORE the load (a value loaded through a clamped index only feeds a slope that a select replaces by +0), so nothing is read
// outside the field.  n_fields == 0 is K22's probe kernel itself.
#ifndef SPC_TRANSPORT2_HOST

// the slope of a cell from its two neighbours along one axis
template <typename T, bool LIMITED> __device__ __forceinline__ T trn2_slope(const T xm, const T x, const T xp)
{
    const T zero = (T)0;
    const T a = x - xm;
    const T b = xp - x;
    const T t = a + b;
    const T c0 = (T)0.5 * t;
    if (!LIMITED) return c0;
    const T a2 = (T)2 * a;
    const T b2 = (T)2 * b;
    T s = zero;                                                  // an extremum, a zero or a NaN difference
    if (a > zero && b > zero) {
        const T lo = a2 < b2 ? a2 : b2;
        s = c0 < lo ? c0 : lo;
    } else if (a < zero && b < zero) {
        const T hi = a2 > b2 ? a2 : b2;
        s = c0 > hi ? c0 : hi;
    }
    return s;
}

// the correction of a horizontal face: p, q its two signed Courant numbers, su, sd the slopes of the cells upwind of p and of q
template <typename T> __device__ __forceinline__ T trn2_hface(const T p, const T q, const T su, const T sd)
{
    const T one = (T)1;
    const T tp = one - p;
    const T gp = p * tp;
    const T uq = one + q;
    const T hq = q * uq;
    const T m1 = gp * su;
    const T m2 = hq * sd;
    const T d = m1 - m2;
    return (T)0.5 * d;
}

// the correction of a vertical face: p, q the two signs of its mass flux, rl, ru 1 / g of the cells below and above it
template <typename T> __device__ __forceinline__ T trn2_vface(const T p, const T q, const T rl, const T ru, const T sl, const T su)
{
    const T one = (T)1;
    const T cp = p * rl;
    const T dq = q * ru;
    const T tp = one - cp;
    const T gp = p * tp;
    const T uq = one + dq;
    const T hq = q * uq;
    const T m1 = gp * sl;
    const T m2 = hq * su;
    const T d = m1 - m2;
    return (T)0.5 * d;
}

// grid ceil(ncols / C); dynamic LDS: C * col_pitch(ktot, 0) elements; NF >= 1
template <typename T, int NF, bool LIMITED> __global__ __launch_bounds__(TRN_THREADS) void k_les_transport2(const LesTransportP<T> p)
{
    extern __shared__ __align__(16) unsigned char trn2_lds[];
    T *tile = reinterpret_cast<T *>(trn2_lds);
    constexpr int TRN2_UNROLL = NF <= 2 ? NF : 1;                // the fields of a cell unrolled, or one after the other
    const int ktot = p.ktot, P = col_pitch(ktot, 0), C = p.cols;
    const int itot = p.itot, jtot = p.jtot;
    const ColRun tr(blockIdx.x, C, p.ncols, p.nij, ktot);
    const int64_t row = (int64_t)jtot * ktot;                    // cells of one row i
    // 1. e = g * ((ce - cw) + (cn - cs)) of every cell of the run -> LDS (K22's phase 1)
    for (int e = threadIdx.x; e < tr.len; e += TRN_THREADS) {
        const VadCell w = vad_cell(e, ktot, tr.l0, tr.rem0, (uint32_t)p.nij, (uint32_t)jtot);
        const int64_t o = tr.run + e;
        const TrnNb nb = trn_neighbours(o, w.i, w.j, itot, jtot, ktot, row);
        const TrnFaces<T> c = trn_faces<T>(p.u, p.v, o, nb, p.hx[w.l], p.hy[w.l]);
        const T gk = p.g[w.l * p.pitch_prof + w.k];
        const T dx = c.ce - c.cw;
        const T dy = c.cn - c.cs;
        const T d = dx + dy;
        tile[w.c * P + w.k] = gk * d;
    }
    __syncthreads();
    // 2. the mass flux through the upper faces, one column per lane
    if ((int)threadIdx.x < tr.nc) vad_column<T>(tile + threadIdx.x * P, ktot);
    __syncthreads();
    // 3. the six second-order fluxes of every cell of every field, mtop, ftop and the outflow Courant sums
    const T zero = (T)0;
    T smax = zero;
    int64_t lcur = -1;
    for (int e = threadIdx.x; e < tr.len; e += TRN_THREADS) {
        const VadCell w = vad_cell(e, ktot, tr.l0, tr.rem0, (uint32_t)p.nij, (uint32_t)jtot);
        const int64_t o = tr.run + e;
        const int k = w.k;
        const T *M = tile + w.c * P;
        const T Mb = k ? M[k - 1] : zero;
        const T Mt = M[k];
        if (p.mtop) p.mtop[o] = Mt;
        const int km = k ? k - 1 : 0;
        const int kp = k + 1 < ktot ? k + 1 : ktot - 1;
        const T *rl = p.r + w.l * p.pitch_prof;
        const T rk = rl[k], rm = rl[km], rp = rl[kp];
        const T pb = Mb > zero ? Mb : zero, qb = Mb < zero ? Mb : zero;
        const T pt = Mt > zero ? Mt : zero, qt = Mt < zero ? Mt : zero;
        const TrnNb nb = trn_neighbours(o, w.i, w.j, itot, jtot, ktot, row);
        const TrnFaces<T> c = trn_faces<T>(p.u, p.v, o, nb, p.hx[w.l], p.hy[w.l]);
        const T pw = c.cw > zero ? c.cw : zero, qw = c.cw < zero ? c.cw : zero;
        const T pe = c.ce > zero ? c.ce : zero, qe = c.ce < zero ? c.ce : zero;
        const T ps = c.cs > zero ? c.cs : zero, qs = c.cs < zero ? c.cs : zero;
        const T pn = c.cn > zero ? c.cn : zero, qn = c.cn < zero ? c.cn : zero;
        if (p.cmax) {
            const T sx = pe - qw;
            const T sy = pn - qs;
            const T sh = sx + sy;
            const T sz = pt - qb;
            const T sv = rk * sz;
            const T s = sh + sv;
            if (w.l != lcur) {                                   // the lane's cells come in ascending l
                if (lcur >= 0) vad_atomic_max<T>(p.cmax, lcur, smax);
                lcur = w.l;
                smax = zero;
            }
            smax = s > smax ? s : smax;
        }
        // the neighbours at distance 2: periodic again along i and j, clamped along k
        const int im = w.i ? w.i - 1 : itot - 1;
        const int ip = w.i + 1 < itot ? w.i + 1 : 0;
        const int jm = w.j ? w.j - 1 : jtot - 1;
        const int jp = w.j + 1 < jtot ? w.j + 1 : 0;
        const int imm = im ? im - 1 : itot - 1;
        const int ipp = ip + 1 < itot ? ip + 1 : 0;
        const int jmm = jm ? jm - 1 : jtot - 1;
        const int jpp = jp + 1 < jtot ? jp + 1 : 0;
        const int64_t oww = o + (int64_t)(imm - w.i) * row;
        const int64_t oee = o + (int64_t)(ipp - w.i) * row;
        const int64_t oss = o + (int64_t)(jmm - w.j) * ktot;
        const int64_t onn = o + (int64_t)(jpp - w.j) * ktot;
        const int64_t okm = k ? o - 1 : o;
        const int64_t okp = k + 1 < ktot ? o + 1 : o;
        const int64_t okmm = k > 1 ? o - 2 : okm;
        const int64_t okpp = k + 2 < ktot ? o + 2 : okp;
        const bool below = k > 1;                                // the cell below has a slope along k
        const bool inner = k > 0 && k + 1 < ktot;                // the cell itself has one
        const bool above = k + 2 < ktot;                         // the cell above has one
        // (unrolled across more than two fields the scalar registers spill: the field pointers and the face numbers stay live)
#pragma unroll TRN2_UNROLL
        for (int f = 0; f < NF; ++f) {
            const T *xf = p.field[f];
            const T x = xf[o], xw = xf[nb.ow], xe = xf[nb.oe], xs = xf[nb.os], xn = xf[nb.on], xm = xf[okm], xp = xf[okp];
            const T xww = xf[oww], xee = xf[oee], xss = xf[oss], xnn = xf[onn], xmm = xf[okmm], xpp = xf[okpp];
            const T w1 = pw * xw, w2 = qw * x;
            const T e1 = pe * x, e2 = qe * xe;
            const T s1 = ps * xs, s2 = qs * x;
            const T n1 = pn * x, n2 = qn * xn;
            const T b1 = pb * xm, b2 = qb * x;
            const T t1 = pt * x, t2 = qt * xp;
            const T Fw = w1 + w2;
            const T Fe = e1 + e2;
            const T Fs = s1 + s2;
            const T Fn = n1 + n2;
            const T Fb = b1 + b2;
            const T Ft = t1 + t2;
            const T siw = trn2_slope<T, LIMITED>(xww, xw, x);
            const T sic = trn2_slope<T, LIMITED>(xw, x, xe);
            const T sie = trn2_slope<T, LIMITED>(x, xe, xee);
            const T sjs = trn2_slope<T, LIMITED>(xss, xs, x);
            const T sjc = trn2_slope<T, LIMITED>(xs, x, xn);
            const T sjn = trn2_slope<T, LIMITED>(x, xn, xnn);
            const T skb = below ? trn2_slope<T, LIMITED>(xmm, xm, x) : zero;
            const T skc = inner ? trn2_slope<T, LIMITED>(xm, x, xp) : zero;
            const T skt = above ? trn2_slope<T, LIMITED>(x, xp, xpp) : zero;
            const T Aw = trn2_hface<T>(pw, qw, siw, sic);
            const T Ae = trn2_hface<T>(pe, qe, sic, sie);
            const T As = trn2_hface<T>(ps, qs, sjs, sjc);
            const T An = trn2_hface<T>(pn, qn, sjc, sjn);
            const T Ab = trn2_vface<T>(pb, qb, rm, rk, skb, skc);
            const T At = trn2_vface<T>(pt, qt, rk, rp, skc, skt);
            const T Fw2 = Fw + Aw;
            const T Fe2 = Fe + Ae;
            const T Fs2 = Fs + As;
            const T Fn2 = Fn + An;
            const T Fb2 = Fb + Ab;
            const T Ft2 = Ft + At;
            const T hi = Fe2 - Fw2;
            const T hj = Fn2 - Fs2;
            const T h = hi + hj;
            const T dz = Ft2 - Fb2;
            const T z = rk * dz;
            T y = x - h;
            y = y - z;
            p.out[f][o] = y;
            if (p.ftop && k == ktot - 1) p.ftop[f * p.ncols + tr.col0 + w.c] = Ft2;
        }
    }
    if (p.cmax) {
        long long lw = lcur;                                     // the last LES of the wave (-1: no lane had a cell)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const long long o = __shfl_xor(lw, d, 64);
            lw = o > lw ? o : lw;
        }
        if (__all(lcur < 0 || lcur == lw)) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const T o = __shfl_xor(smax, d, 64);
                smax = o > smax ? o : smax;
            }
            if ((threadIdx.x & 63) == 0 && lw >= 0) vad_atomic_max<T>(p.cmax, lw, smax);
        } else if (lcur >= 0) {
            vad_atomic_max<T>(p.cmax, lcur, smax);
        }
    }
}

#else  // SPC_TRANSPORT2_HOST ------------------------------------------------------------------------------------------------

// (the checks, the parameter block and the launch geometry are K17's: vad_family_args and vad_family_launch in spc_vadvect.hpp)
template <typename T, bool LIMITED> static int les_transport2_fields(const LesTransportP<T> &p, int n_fields, void *stream)
{
    switch (n_fields) {
    case 0: return les_transport_probe<T>(p, stream);              // K22's probe: the limiter has nothing to act on
    case 1: return vad_family_launch(k_les_transport2<T, 1, LIMITED>, "k_les_transport2", p, stream);
    case 2: return vad_family_launch(k_les_transport2<T, 2, LIMITED>, "k_les_transport2", p, stream);
    case 3: return vad_family_launch(k_les_transport2<T, 3, LIMITED>, "k_les_transport2", p, stream);
    case 4: return vad_family_launch(k_les_transport2<T, 4, LIMITED>, "k_les_transport2", p, stream);
    case 5: return vad_family_launch(k_les_transport2<T, 5, LIMITED>, "k_les_transport2", p, stream);
    default: return vad_family_launch(k_les_transport2<T, 6, LIMITED>, "k_les_transport2", p, stream);
    }
}

static int les_transport2_limiter(const spc_les_transport2_args *a)
{
    if (a->limiter != SPC_LIMITER_NONE && a->limiter != SPC_LIMITER_MC)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_transport2: limiter %lld is neither SPC_LIMITER_NONE nor SPC_LIMITER_MC", "", (long long)a->limiter);
    return SPC_OK;
}

template <typename T> static int les_transport2_impl(const spc_les_transport2_args *a, void *stream)
{
    LesTransportP<T> p = {};
    const int rc = vad_family_args<T>("les_transport2", a, p, stream, les_transport2_limiter);
    if (rc || !p.cols) return rc;
    return a->limiter == SPC_LIMITER_MC ? les_transport2_fields<T, true>(p, a->n_fields, stream) : les_transport2_fields<T, false>(p, a->n_fields, stream);
}

#endif
