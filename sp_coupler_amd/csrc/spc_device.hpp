// spc_device.hpp -- what more than one kernel family uses on the device: constants, the inline pow(), the streaming
// accesses, the prepared divisor, numpy's searches and the two numpy.interp forms, the fixed-trip searches on padded LDS
// rows, the kernel parameter blocks, the slab mapping and the STAMP instrument.  First in spc_hip.hip's include chain.
#pragma once

constexpr int BLOCK = 256;
constexpr int MAX_LDS_BYTES = 64 * 1024;    // preferred ceiling (default dynamic-LDS limit, >= 2 workgroups per CU)
constexpr int HARD_LDS_BYTES = 160 * 1024;  // gfx950: 160 KiB per CU, reachable for one column per workgroup

// ---- constants: splib/sputils.py:14-20 ----------------------------------------------------------
template <typename T> struct K {
    static constexpr T pref0 = T(1e5), rd = T(287.04), rv = T(461.5), cp = T(1004.), rlv = T(2.53e6),
                       grav = T(9.81);
};

// x**y for the two exponents of this path, y = -+rd/cp (sputils.py:28-34), |y| <= 1: spc_pow.h (one source for this file and
// for the host accuracy sweep tools/csrc/pow_accuracy.c; round 4: <= 0.56 ulp against an 80-bit reference, was 1.2).
// Arguments outside (0, inf) get C99 pow()'s special values for a non-integer exponent, inline (0 -> inf or 0, inf -> 0 or
// inf, negative -> NaN, -inf like +inf, NaN -> NaN); subnormal x goes through the same code (frexp normalises it).  No
// call: an out-of-line ocml pow() made every K1 wave reserve ITS 100 registers (4 waves per SIMD instead of 6).
#define SPC_POW_FN __device__ __forceinline__
#include "spc_pow.h"
// C99 pow()'s value for an x outside (0, inf) and a non-integer y
__device__ __forceinline__ double spc_pow_special(double x, double y)
{
    if (x != x) return x;                                                          // NaN
    const double big = __builtin_huge_val();
    if (x == 0.0) return y < 0.0 ? big : 0.0;                                      // +-0 (not an odd integer y)
    if (x == big || x == -big) return y < 0.0 ? 0.0 : big;                         // +-inf (not an odd integer y)
    return __builtin_nan("");                                                      // negative finite x, non-integer y
}
__device__ __forceinline__ double spc_pow(double x, double y)
{
    if (!(x > 0.0 && x <= 1.7976931348623157e308)) return spc_pow_special(x, y);
    return spc_pow_pos(x, y);
}
// (p / pref0) ** y of the standalone exner operator (sputils.py:29,34), which is bound by VALU issue: the polynomial
// coefficients come from scalar registers (spc_pow.h: spc_pow_pos_tab), and pressures in [2^-900, 2^900] -- all there are -- take
// the quotient from Markstein's iteration (spc_pow.h: correctly rounded, 5 operations) and are known to be positive and
// finite afterwards; anything else divides and may end in the special values.  Same bits as spc_pow(p / pref0, y).
__device__ __forceinline__ double spc_exner_pow(double p, double y)
{
    double x;
    if (__builtin_expect(p >= 0x1p-900 && p <= 0x1p+900, 1)) {
        x = spc_div_pref0_markstein(p);
    } else {
        x = p / 1e5;
        if (!(x > 0.0 && x <= 1.7976931348623157e308)) return spc_pow_special(x, y);
    }
    return spc_pow_pos_tab(x, y);
}
// the fp32 variant's power: spc_powf.h -- evaluated inside double arithmetic and rounded once (<= 0.5 + 2^-14 ulp, the host
// sweep computes the device's bits), inline; rounds 1-4 called ocml's powf() out of line.  Special values as for double.
#include "spc_powf.h"
__device__ __forceinline__ float spc_pow(float x, float y)
{
    if (!(x > 0.0f && x <= 3.4028234663852886e38f)) {
        if (x != x) return x;                                                      // NaN
        const float big = __builtin_huge_valf();
        if (x == 0.0f) return y < 0.0f ? big : 0.0f;
        if (x == big || x == -big) return y < 0.0f ? 0.0f : big;
        return __builtin_nanf("");
    }
    return spc_powf_pos(x, y);
}
__device__ __forceinline__ float spc_exner_pow(float p, float y) { return spc_pow(p / 1e5f, y); }

// Streaming accesses of the hot kernels: every input element is read once and every output written
// once per launch.  Plain loads and stores: non-temporal ones were measured and lost.
template <typename T> __device__ __forceinline__ T ldg(const T *q) { return *q; }
// WT = 1: write-through (sc1) store: nothing is left dirty in L2 for the end-of-kernel release to
// flush.  Measured on MI355X: -5 % (K1) / -7 % (K3) at 1024 columns where that flush is ~1 us of a
// ~10 us kernel, but +6 % on K3 at 35k columns -- so only the small-batch launches use it.
template <int WT, typename T> __device__ __forceinline__ void stg(T *q, T v)
{
    if constexpr (WT == 1)
        __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *q = v;
}

// Every quotient on this path is a true IEEE division (x / y), never x * (1/y): the reference divides,
// and bit-parity of the u/v/qt/ql forcings and of all tendencies depends on it.  (Tried and measured
// slower on gfx950: RN(1/y) shared by the 5-7 slopes of a level + two FMA Newton steps + v_div_fixup;
// the magnitude-window checks it needs cost more than hipcc's v_div_scale/v_rcp/v_div_fmas expansion.)
//
// Divisor<T>: a divisor prepared once and applied to several dividends (the 5-7 slopes of a level share x1 - x0, every forcing
// of a launch divides by dt).  double: the division itself, nothing prepared -- same instructions, same bits as before.
// float (the fp32 arithmetic variant, round 5): a / b = (float)((double)a * r) with r = 1 / (double)b to ~2^-52 -- the
// CORRECTLY ROUNDED float quotient for every normal result: a quotient of two 24-bit floats is never closer than 2^-49
// (relative) to a rounding boundary of the 24-bit format, and the double product is within 2^-51.  v_cvt / v_mul_f64 / v_cvt
// issue at the rate of v_fma_f32 (tools/issue_rate.py, profiles/r05_issue_rate.log): 3 instructions per quotient + ~7 per
// distinct divisor against the ~12 (with two denormal-mode switches) of the compiler's IEEE float division; measured on the
// fp32 K1 / K3: profiles/r05_f32_div_ab.log.  0, inf and NaN divisors keep v_rcp_f64's own answer (the Newton steps would
// turn it into NaN), so x / 0 = +-inf, 0 / 0 = NaN, x / inf = 0 as IEEE has them; a subnormal QUOTIENT may differ from the
// IEEE one in its last bit (double rounding), nothing on this path is that small.
template <typename T> struct Divisor;
template <> struct Divisor<double> {
    double b;
    __device__ __forceinline__ explicit Divisor(double b_) : b(b_) {}
    __device__ __forceinline__ double div(double a) const { return a / b; }
};
template <> struct Divisor<float> {
    double r;
    __device__ __forceinline__ explicit Divisor(float b)
    {
        const double bd = (double)b, r0 = __builtin_amdgcn_rcp(bd);
        double r1 = __builtin_fma(r0, __builtin_fma(-bd, r0, 1.0), r0);
        r1 = __builtin_fma(r1, __builtin_fma(-bd, r1, 1.0), r1);
        r = (r0 != 0.0 && r0 - r0 == 0.0) ? r1 : r0;                     // finite and non-zero: refined
    }
    __device__ __forceinline__ explicit Divisor(double r_, int) : r(r_) {}       // r = RN(1 / b) known at compile time
    __device__ __forceinline__ float div(float a) const { return (float)((double)a * r); }
};
template <typename T> __device__ __forceinline__ T div_grav(T x) { return x / K<T>::grav; }
template <typename T> __device__ __forceinline__ T div_cp(T x) { return x / K<T>::cp; }
template <typename T> __device__ __forceinline__ T div_pref0(T x) { return x / K<T>::pref0; }
template <> __device__ __forceinline__ float div_grav<float>(float x) { return Divisor<float>(1.0 / (double)K<float>::grav, 0).div(x); }
template <> __device__ __forceinline__ float div_cp<float>(float x) { return Divisor<float>(1.0 / (double)K<float>::cp, 0).div(x); }
template <> __device__ __forceinline__ float div_pref0<float>(float x) { return Divisor<float>(1.0 / (double)K<float>::pref0, 0).div(x); }

// numpy NaN-aware "a < b" used by searchsorted (NaN sorts to the end)
template <typename T> __device__ __forceinline__ bool np_lt(T a, T b) { return a < b || (b != b && a == a); }

// numpy.searchsorted(a, key, side='right'): first i with key < a[i]   (splib/sputils.py:88-91)
template <typename T> __device__ __forceinline__ int ss_right(const T *a, int n, T key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        int mid = lo + ((hi - lo) >> 1);
        if (np_lt(key, a[mid])) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// numpy.searchsorted(a, v, side='left'): first i with !(a[i] < v)   (splib/sputils.py:88-91)
template <typename T> __device__ __forceinline__ int ss_left(const T *a, int n, T key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (np_lt(a[mid], key)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// numpy.searchsorted(-a, -v) (side='left'): first i with !(-a[i] < -v)   (splib/spcpl.py:498)
template <typename T> __device__ __forceinline__ int ss_left_neg(const T *a, int n, T v)
{
    const T key = -v;
    int lo = 0, hi = n;
    while (lo < hi) {
        int mid = lo + ((hi - lo) >> 1);
        if (np_lt(-a[mid], key)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Count of xp[i] <= x for ascending xp (== numpy.interp's j + 1), fixed trip count: `p2` is the
// largest power of two <= n, so every lane runs the same floor(log2 n)+1 steps (no divergence).
template <typename T> __device__ __forceinline__ int upper_count(const T *xp, int n, int p2, T x)
{
    int pos = 0;
    for (int s = p2; s > 0; s >>= 1) {
        const int t = pos + s;
        const int ti = (t <= n ? t : n) - 1;
        if (t <= n && xp[ti] <= x) pos = t;
    }
    return pos;
}

// One numpy.interp evaluation given the bracketing samples (arr_interp of numpy 2.2):
//   slope = (f1-f0)/(x1-x0); r = slope*(x-x0)+f0; NaN fallbacks as in numpy.
template <typename T, typename D> __device__ __forceinline__ T lerp_np(T x, T x0, T x1, T f0, T f1, const D &dx)
{
    const T slope = dx.div(f1 - f0);               // (f1 - f0) / (x1 - x0), the divisor prepared once per level
    T r = slope * (x - x0) + f0;
    if (r != r) {
        r = slope * (x - x1) + f1;
        if (r != r && f0 == f1) r = f0;
    }
    return r;
}

template <typename T> __device__ __forceinline__ T lerp_np(T x, T x0, T x1, T f0, T f1)
{
    const T slope = (f1 - f0) / (x1 - x0);
    T r = slope * (x - x0) + f0;
    if (r != r) {
        r = slope * (x - x1) + f1;
        if (r != r && f0 == f1) r = f0;
    }
    return r;
}

// Interpolation state shared by all fields of one output level.
template <typename T> struct Bracket {
    int j;       // clamped lower sample index (0..n-2), valid when mode == 0
    int mode;    // 0 interpolate, 1 take sample `j`, 2 result is x itself (NaN)
    T x, x0, x1;
};

template <typename T> __device__ __forceinline__ Bracket<T> bracket(const T *xp, int n, int p2, T x)
{
    Bracket<T> b;
    b.x = x;
    if (n == 1) { b.mode = 1; b.j = 0; b.x0 = b.x1 = x; return b; }   // numpy lenxp == 1: fp[0], NaN x included
    if (x != x) { b.mode = 2; b.j = 0; b.x0 = b.x1 = x; return b; }
    const int j = upper_count(xp, n, p2, x) - 1;
    if (j < 0) { b.mode = 1; b.j = 0; b.x0 = b.x1 = x; return b; }                  // x < xp[0] -> fp[0]
    if (j >= n - 1) { b.mode = 1; b.j = n - 1; b.x0 = b.x1 = x; return b; }         // x >= xp[n-1] -> fp[n-1]
    b.j = j;
    b.x0 = xp[j];
    b.x1 = xp[j + 1];
    b.mode = (b.x0 == x) ? 1 : 0;                                                   // exact hit -> fp[j]
    return b;
}

template <typename T> __device__ __forceinline__ T interp_at(const Bracket<T> &b, const T *fp)
{
    if (b.mode == 2) return b.x;
    if (b.mode == 1) return fp[b.j];
    return lerp_np(b.x, b.x0, b.x1, fp[b.j], fp[b.j + 1]);
}

// ---- branch-light form used by the hot kernels -------------------------------------------------
// Every case of numpy.interp expressed as ONE predicated code path, so that the 5 (K1) / 7 (K3)
// independent slope divisions of a level sit in one basic block and interleave:
//   take : the result is the sample fp[j0] itself (x outside [xp[0], xp[n-1]], x == xp[j], n == 1)
//   nanx : the result is x itself (NaN x, n > 1)
//   else : numpy's slope form between samples j0 and j1 = j0 + 1
// For take / nanx lanes (x0, x1) = (0, 1) and j1 == j0, so the (discarded) slope arithmetic stays finite.
template <typename T> struct Br {
    int j0, j1;
    bool take, nanx;
    T x, x0, x1;
};

template <typename T> __device__ __forceinline__ Br<T> bracket2(const T *xp, int n, int p2, T x)
{
    Br<T> b;
    const int j = upper_count(xp, n, p2, x) - 1;           // NaN x: every comparison false -> j = -1
    const bool below = j < 0, above = j >= n - 1;
    const int jmax = n >= 2 ? n - 2 : 0;
    const int jc = j < 0 ? 0 : (j > jmax ? jmax : j);
    const T x0 = xp[jc], x1 = xp[jc + 1 < n ? jc + 1 : n - 1];
    b.take = (n == 1) | below | above | (x0 == x);
    b.nanx = (x != x) & (n != 1);
    b.j0 = above ? n - 1 : jc;
    b.j1 = b.take ? b.j0 : jc + 1;
    b.x = x;
    b.x0 = b.take ? T(0) : x0;
    b.x1 = b.take ? T(1) : x1;
    return b;
}

// r[k] = numpy.interp result of field k given the samples f0[k] = fp_k[j0], f1[k] = fp_k[j1]
template <int NF, typename T> __device__ __forceinline__ void interp_fields(const Br<T> &b, const T (&f0)[NF], const T (&f1)[NF], T (&r)[NF])
{
    const T t0 = b.x - b.x0;
    const Divisor<T> dx(b.x1 - b.x0);
    T slope[NF];
    bool any_nan = false;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        slope[k] = dx.div(f1[k] - f0[k]);
        r[k] = slope[k] * t0 + f0[k];
        any_nan |= (r[k] != r[k]);
    }
    if (any_nan & !b.take & !b.nanx) {   // numpy's NaN fallbacks: rare, one masked block for all fields
        const T t1 = b.x - b.x1;
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            if (r[k] != r[k]) {
                T q = slope[k] * t1 + f1[k];
                if (q != q && f0[k] == f1[k]) q = f0[k];
                r[k] = q;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) r[k] = b.nanx ? b.x : (b.take ? f0[k] : r[k]);
}

// first k in [1, n-1] with !(z[k] < a), minus 1: the `while z[i+1] < a: i += 1` scan of integral()
// (splib/sputils.py:122-127) for ascending z
template <typename T> __device__ __forceinline__ int scan_cell(const T *z, int n, T a)
{
    int lo = 1, hi = n - 1;   // the scan cannot pass n-2 because a <= z[n-1] was checked
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (z[mid] < a) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// ---- searches on LDS rows: fixed trip count, no bounds check -------------------------------------------------------
// The three searches of this file -- numpy.interp's bracket (count of xp[i] <= x), numpy.searchsorted (count of entries
// in front of the insertion point) and integral()'s cell scan (count of z[k] < a) -- are prefix counts over an ascending
// row.  A staged row is PADDED WITH NaN up to 2 p2 entries (p2 = the largest power of two <= its length): the greedy
// power-of-two descent of upper_count() then needs no `t <= n` test, because no predicate used here advances on a NaN
// (searchsorted with a NaN key is the one exception and clamps), and with the trip count a template argument (SL =
// log2 p2 + 1) every probe is one ds_read with an immediate offset + compare + select: 3 VALU instructions per step
// instead of 8-12 (round 4: the first K7 generation was bound by VALU issue, 100-150 instructions per output,
// profiles/r04_k7_counters.log).  SL = 0: the same descent with p2 at run time; SL = -1: nothing staged (rows beyond
// the LDS), the operators fall back to the loops on global memory.
__host__ __device__ inline int su_pad(int p2) { return 2 * p2 + 2; }      // entries of a padded row (+2: rows off each other's banks)

// the descent carries the ADDRESS of the first entry not counted (row + count), not the count: a step is then one
// ds_read at [address + immediate], one add, one compare and one select -- no index-to-address shift per probe
template <int SL, typename T, typename Pred> __device__ __forceinline__ const T *su_seek(const T *row, int p2, const Pred &adv)
{
    const T *p = row;
    if constexpr (SL > 0) {
#pragma unroll
        for (int s = 1 << (SL - 1); s > 0; s >>= 1) {
            const T *const nx = p + s;
            p = adv(p[s - 1]) ? nx : p;
        }
    } else {
        for (int s = p2; s > 0; s >>= 1) {
            const T *const nx = p + s;
            p = adv(p[s - 1]) ? nx : p;
        }
    }
    return p;
}

template <int SL, typename T, typename Pred> __device__ __forceinline__ int su_count(const T *row, int p2, const Pred &adv)
{
    return (int)(((unsigned)(size_t)su_seek<SL>(row, p2, adv) - (unsigned)(size_t)row) / (unsigned)sizeof(T));   // 32-bit: LDS addresses
}

// ---- kernel parameter blocks (typed copies of the C structs) ------------------------------------
struct DimsP {
    int64_t n_cols, pitchG, pitchGh, pitchL;
    int nG, nL, cb, p2G, p2L, shared_grid, xcd_remap;
};

struct Empty {};

// optional outputs / surface coupling of the forward pass: only in the FULL kernel variant, so that the
// lean hot-path variant keeps its ~26 pointers in SGPRs without spilling
template <typename T> struct FwdOpt {
    const T *rain, *rain_last;
    T *u, *v, *thl, *qt, *ps, *Zf, *Zh, *rainrate;
    const T *Z0M, *Z0H, *QLflux, *QIflux, *SHflux, *TSflux;
    T *z0m, *z0h, *wthl, *wqt;
};

template <typename T, bool FULL> struct FwdP {
    DimsP d;
    const T *U, *V, *Tm, *SH, *QL, *QI, *Pf, *Ph, *Zgfull, *Zghalf, *zf, *zh;
    const T *u_d, *v_d, *thl_d, *qt_d, *ql_d, *ps_d;
    T factor, dt;
    T *f_u, *f_v, *f_thl, *f_qt, *f_ql, *ql_ref, *f_ps;
    int32_t *idx;
    typename std::conditional<FULL, FwdOpt<T>, Empty>::type o;
};

template <typename T> using FwdFull = FwdP<T, true>;

template <typename T> struct BwdP {
    DimsP d;
    const T *Tm, *SH, *QL, *QI, *U, *V, *A, *Zf, *Zgfull, *Zghalf, *zf;
    const T *t_d, *qt_d, *ql_d, *ql_ice_d, *u_d, *v_d, *A_prof;
    const T *zh, *Zh, *rhobf_d;    // conservative coarsening only (K4)
    T factor, dt;
    T *f_T, *f_SH, *f_QL, *f_QI, *f_U, *f_V, *f_A;
    int32_t *start_index;
};

template <typename T> struct DiagP {
    DimsP d;
    const T *Tm, *SH, *QL, *QI, *Pf, *Zgfull, *Zghalf, *zf, *thl_d, *ql_d, *ql_ice_d;
    T *Tv, *THL, *QT, *Zf, *Zh, *pf, *t, *ql_water;
};

extern __shared__ __align__(16) unsigned char spc_smem[];

// XCD-aware workgroup -> column-slab mapping.  The dispatcher deals workgroups round-robin over the 8
// XCDs (b and b+8 share one, each XCD has its own L2), while rows of 91 doubles (728 B) are not 128-B
// aligned: with the identity mapping the cache line shared by two neighbouring slabs is fetched by two
// different XCDs.  Giving each XCD a CONTIGUOUS range of slabs keeps those lines in one L2.  Speed only,
// never correctness (every slab is still processed exactly once).  Used for slabs of <= 2 columns, where
// slab boundaries are frequent (K3: +4-6 % at 35k-349k columns; 8-column slabs of K1: -1.5 %, so not there).
__device__ __forceinline__ unsigned slab_index(int remap)
{
    if (remap) {
        const unsigned b = blockIdx.x, nb = gridDim.x, x = b & 7u, j = b >> 3, q = nb >> 3, r = nb & 7u;
        return x * q + (x < r ? x : r) + j;
    }
    return blockIdx.x;
}

// Diagnostic build only (-DSPC_STAMPS, tools/stamps.py): thread 0 of each workgroup drains its memory
// counters and writes the 100 MHz wall clock at phase boundaries into a buffer no kernel code reads.
#ifdef SPC_STAMPS
__device__ unsigned long long *g_stamps = nullptr;
#define STAMP(i)                                                                     \
    do {                                                                             \
        if (threadIdx.x == 0 && g_stamps && (SPC_STAMPS == 1 || (i) == 0 || (i) == 5)) {  \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");              \
            g_stamps[(size_t)blockIdx.x * 8 + (i)] = wall_clock64();                 \
        }                                                                            \
    } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

