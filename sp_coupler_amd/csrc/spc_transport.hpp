// spc_transport.hpp -- K22: one UNSPLIT donor-cell step in FLUX FORM of the transport of the device-resident LES fields along
// i, j and k by the horizontal winds and the mass flux that continuity gives them, kernel and host side.  spc_hip.hip includes
// it twice, like spc_vadvect.hpp: with the kernel among the device headers (after spc_advect.hpp and spc_vadvect.hpp, whose
// helpers it uses), and -- SPC_TRANSPORT_HOST defined -- after spc_launch.hpp and the host side of spc_slab.hpp.
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The rule
// (include/spc.h) per cell (l, i, j, k), in T, one rounding per operation, never an fma (the build has FP contraction off), no
// division, im / ip / jm / jp the periodic neighbours, g = rho dz and r = 1 / g the profiles [n_les x ktot]:
//   cw, ce, cs, cn  K16's face Courant numbers at level k (spc_advect.hpp)
//   d  = (ce - cw) + (cn - cs);   e = g[l][k] * d
//   M[0] = +0;   M[k + 1] = M[k] - e                      K17's chain (spc_vadvect.hpp); mtop[l][i][j][k] = M[k + 1]
//   pw = cw > 0 ? cw : 0;   qw = cw < 0 ? cw : 0          likewise (pe, qe), (ps, qs), (pn, qn), (pb, qb) of M[k], (pt, qt) of M[k + 1]
//   Fw = pw * x[im] + qw * x;   Fe = pe * x + qe * x[ip];   Fs = ps * x[jm] + qs * x;   Fn = pn * x + qn * x[jp]
//   Fb = pb * x[km] + qb * x;   Ft = pt * x + qt * x[kp]  km = k ? k - 1 : 0, kp = k + 1 < ktot ? k + 1 : ktot - 1
//   h  = (Fe - Fw) + (Fn - Fs);   z = r[l][k] * (Ft - Fb);   x' = (x - h) - z
//   s  = ((pe - qw) + (pn - qs)) + r[l][k] * (pt - qb);   cmax[l] = max over the cells of LES l of s
//   ftop[f][l][i][j] = Ft at k = ktot - 1
// The flux through a face is formed from the SAME operands in the same order by both cells that share it (Fe of i is Fw of ip:
// ce of i is cw of ip, bit for bit), so what leaves one cell enters its neighbour and sum g x changes only by ftop and rounding.
//
// The shape is K17's: a workgroup takes C = col_cols consecutive columns of the flat column index, a contiguous run of
// C * ktot cells that may span rows i and LES; phase 1 (all lanes, coalesced: e -> LDS, odd pitch) and phase 2 (one lane per
// column: the chain) are K17's.  Phase 3 walks the run again: M[k], M[k + 1] from LDS, the four horizontal face numbers FORMED
// AGAIN from the six wind values of the cell (the lines phase 1 of this workgroup fetched a moment ago: L1 / L2 hits), and per
// field the cell and its six neighbours from global memory.  Keeping cw, ce, cs, cn in LDS instead would make the tile five
// times as large and C five times as small (at ktot = 160 in f64: 6 columns for 32), and the chain of phase 2 would occupy 6
// lanes of 256 -- the winds' second read costs less than that (DESIGN.md 7.3 has the numbers).  The flat run along j is kept:
// the j +- 1 neighbours lie ktot cells away in the run (other lanes fetch them as their own cells), the i +- 1 neighbours one
// row away, where the neighbouring workgroups fetch them as their own cells: with 5 fields a tile of 32 columns of 160 levels
// reads 0.2 MiB, far below the 4 MiB of L2 per XCD, so they come from the caches as they do for K16.  cmax and its atomicMax
// are K17's.  The outputs are separate buffers written whole, so no workgroup waits for another.
#ifndef SPC_TRANSPORT_HOST

constexpr int TRN_THREADS = VAD_THREADS;
constexpr int TRN_MAXF = 6;

template <typename T> struct LesTransportP {
    const T *u, *v;
    const T *field[TRN_MAXF];
    T *out[TRN_MAXF];
    const T *hx, *hy;
    const T *g, *r;
    T *cmax;                       // or nullptr
    T *mtop;                       // or nullptr
    T *ftop;                       // [n_fields][ncols], or nullptr
    int64_t ncols;                 // n_les * itot * jtot
    int64_t pitch_prof;
    int32_t itot, jtot, ktot;
    int32_t nij;                   // itot * jtot
    int32_t cols;                  // C: columns per workgroup
};

// the offsets of the four horizontal neighbours of cell o in row i, column j (periodic)
struct TrnNb {
    int64_t ow, oe, os, on;
};

__device__ __forceinline__ TrnNb trn_neighbours(const int64_t o, const int i, const int j, const int itot, const int jtot, const int ktot, const int64_t row)
{
    TrnNb n;
    n.ow = o + (i ? -row : (int64_t)(itot - 1) * row);
    n.oe = o + (i + 1 < itot ? row : -(int64_t)(itot - 1) * row);
    n.os = o + (j ? -(int64_t)ktot : (int64_t)(jtot - 1) * ktot);
    n.on = o + (j + 1 < jtot ? (int64_t)ktot : -(int64_t)(jtot - 1) * ktot);
    return n;
}

// K16's face Courant numbers of cell o
template <typename T> struct TrnFaces {
    T cw, ce, cs, cn;
};

template <typename T> __device__ __forceinline__ TrnFaces<T> trn_faces(const T *u, const T *v, const int64_t o, const TrnNb &n, const T hx, const T hy)
{
    const T uw = u[n.ow], uc = u[o], ue = u[n.oe];
    const T vs = v[n.os], vc = v[o], vn = v[n.on];
    const T aw = uw + uc, ae = uc + ue, as = vs + vc, an = vc + vn;
    TrnFaces<T> c;
    c.cw = aw * hx;
    c.ce = ae * hx;
    c.cs = as * hy;
    c.cn = an * hy;
    return c;
}

// grid ceil(ncols / C); dynamic LDS: C * col_pitch(ktot, 0) elements
template <typename T, int NF> __global__ __launch_bounds__(TRN_THREADS) void k_les_transport(const LesTransportP<T> p)
{
    extern __shared__ __align__(16) unsigned char trn_lds[];
    T *tile = reinterpret_cast<T *>(trn_lds);
    const int ktot = p.ktot, P = col_pitch(ktot, 0), C = p.cols;
    const int itot = p.itot, jtot = p.jtot;
    const ColRun tr(blockIdx.x, C, p.ncols, p.nij, ktot);
    const int64_t row = (int64_t)jtot * ktot;                    // cells of one row i
    // 1. e = g * ((ce - cw) + (cn - cs)) of every cell of the run -> LDS
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
    // 3. the six fluxes of every cell of every field, mtop, ftop and the outflow Courant sums
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
        const T rk = p.r[w.l * p.pitch_prof + k];
        const T pb = Mb > zero ? Mb : zero, qb = Mb < zero ? Mb : zero;
        const T pt = Mt > zero ? Mt : zero, qt = Mt < zero ? Mt : zero;
        if (NF == 0 && !p.cmax) continue;                        // the probe of mtop alone
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
        const int64_t okm = k ? o - 1 : o;
        const int64_t okp = k + 1 < ktot ? o + 1 : o;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const T *xf = p.field[f];
            const T x = xf[o], xw = xf[nb.ow], xe = xf[nb.oe], xs = xf[nb.os], xn = xf[nb.on], xm = xf[okm], xp = xf[okp];
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
            const T hi = Fe - Fw;
            const T hj = Fn - Fs;
            const T h = hi + hj;
            const T dz = Ft - Fb;
            const T z = rk * dz;
            T y = x - h;
            y = y - z;
            p.out[f][o] = y;
            if (p.ftop && k == ktot - 1) p.ftop[f * p.ncols + tr.col0 + w.c] = Ft;
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

#else  // SPC_TRANSPORT_HOST -------------------------------------------------------------------------------------------------

// (the checks, the parameter block and the launch geometry are K17's: vad_family_args and vad_family_launch in spc_vadvect.hpp)
static_assert(TRN_THREADS == VAD_THREADS && TRN_MAXF == VAD_MAXF, "K22 launches as K17 does: spc_vadvect.hpp's host path");

template <typename T> static int les_transport_probe(const LesTransportP<T> &p, void *stream)   // no field: cmax and / or mtop (K23's too)
{
    return vad_family_launch(k_les_transport<T, 0>, "k_les_transport", p, stream);
}

template <typename T> static int les_transport_impl(const spc_les_transport_args *a, void *stream)
{
    static_assert(SPC_TRANSPORT_MAX_FIELDS == TRN_MAXF, "include/spc.h and spc_transport.hpp disagree on the fields per launch");
    LesTransportP<T> p = {};
    const int rc = vad_family_args<T>("les_transport", a, p, stream);
    if (rc || !p.cols) return rc;
    switch (a->n_fields) {
    case 0: return les_transport_probe<T>(p, stream);
    case 1: return vad_family_launch(k_les_transport<T, 1>, "k_les_transport", p, stream);
    case 2: return vad_family_launch(k_les_transport<T, 2>, "k_les_transport", p, stream);
    case 3: return vad_family_launch(k_les_transport<T, 3>, "k_les_transport", p, stream);
    case 4: return vad_family_launch(k_les_transport<T, 4>, "k_les_transport", p, stream);
    case 5: return vad_family_launch(k_les_transport<T, 5>, "k_les_transport", p, stream);
    default: return vad_family_launch(k_les_transport<T, 6>, "k_les_transport", p, stream);
    }
}

#endif
