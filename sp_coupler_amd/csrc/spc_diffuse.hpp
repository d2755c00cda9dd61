// spc_diffuse.hpp -- K15: one backward-Euler step of the vertical diffusion of the device-resident LES fields, with the
// kinematic surface flux entering the lowest layer, kernel and host side.  spc_hip.hip includes it twice, like spc_micro.hpp:
// with the kernel among the device headers, and -- SPC_DIFFUSE_HOST defined -- after spc_launch.hpp and the host side of
// spc_slab.hpp (slab_check_extents).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets (spc_slab.hpp).  The matrix of the
// step depends on (l, k) only: sp_coupler_amd/diffusion.py eliminates it ONCE per LES in float64 and hands over a (the lower
// diagonal), m (the reciprocal pivots) and cp (the eliminated upper diagonal), [n_les x ktot], and s0 = dt / dz[0], [n_les].
// The rule (include/spc.h) per column (l, i, j) of field f, in T, one rounding per operation, never an fma (the build has FP
// contraction off), no division:
//   d    = flux[f] ? x[0] + s0[l] * flux[f][l] : x[0]
//   y[0] = d * m[l][0];   y[k] = (x[k] - a[l][k] * y[k - 1]) * m[l][k]      k = 1 ... ktot - 1
//   x'[ktot - 1] = y[ktot - 1];   x'[k] = y[k] - cp[l][k] * x'[k + 1]       k = ktot - 2 ... 0
// The shape is the first of this project with a recurrence along k, the contiguous axis: one serial chain per column.  It is the
// column tile of spc_coltile.hpp with (tiles, faces) = (1, 0), one field per blockIdx.y:
//   1. all DIF_THREADS lanes copy the run into the tile (col_move);
//   2. lane c < C of the first wave runs both sweeps of column c in LDS, y overwriting x, x' overwriting y.  l is per lane:
//      a tile may span several LES.  a and m (forward) and cp (backward) do not depend on the chain: the reads of chunk
//      j + 1 (DIF_U levels) are issued before the arithmetic of chunk j, as are the LDS reads of x.  Where a tile spans at
//      most DIF_STAGE = 2 LES (every tile of an LES of 64 or more columns) and the LDS budget has room, phase 1 also stages
//      those rows of a, m and cp in LDS behind the columns and the sweeps read them there.  Tiles of more LES
//      read them from global memory, where the lanes of one LES share an address;
//   3. all lanes write the run back the way it came.
// A workgroup stores only what it loaded, so the in-place update needs no ordering beyond program order.  The phases of one
// tile do not overlap each other; they overlap those of the other workgroups of the CU (three at 160 levels in either dtype);
// 16 columns may take the whole 160 KiB so that f64 columns of up to 1 279 levels are carried.
#ifndef SPC_DIFFUSE_HOST

constexpr int DIF_THREADS = 256;
constexpr int DIF_MAXF = 4;
constexpr int DIF_U = 8;                        // levels per chunk of a sweep
constexpr int DIF_UB = 4;                       // 16-byte vectors per lane and batch of the load and store phases

template <typename T> struct LesDiffuseP {
    T *field[DIF_MAXF];
    const T *flux[DIF_MAXF];
    const T *a, *m, *cp, *s0;
    int64_t ncols;                 // n_les * itot * jtot
    int64_t pitch_prof;
    int32_t nij, ktot;
    int32_t stage;                 // DIF_STAGE where the rows fit the LDS budget behind the tile, else 0
};

// both sweeps of one column in LDS; a, m, cp: the rows of the column's LES
template <typename T> __device__ __forceinline__ void dif_column(T *x, const T *a, const T *m, const T *cp, const T d, const int ktot)
{
    T y = d * m[0];
    x[0] = y;
    int k = 1;
    if (k + DIF_U <= ktot) {
        T ca[DIF_U], cm[DIF_U];
#pragma unroll
        for (int u = 0; u < DIF_U; ++u) { ca[u] = a[k + u]; cm[u] = m[k + u]; }
        for (; k + DIF_U <= ktot; k += DIF_U) {
            const bool more = k + 2 * DIF_U <= ktot;             // another whole chunk follows: its loads go out first
            T na[DIF_U], nm[DIF_U], cx[DIF_U];
            if (more) {
#pragma unroll
                for (int u = 0; u < DIF_U; ++u) { na[u] = a[k + DIF_U + u]; nm[u] = m[k + DIF_U + u]; }
            }
#pragma unroll
            for (int u = 0; u < DIF_U; ++u) cx[u] = x[k + u];
#pragma unroll
            for (int u = 0; u < DIF_U; ++u) {
                const T t = ca[u] * y;
                y = (cx[u] - t) * cm[u];
                x[k + u] = y;
            }
            if (more) {
#pragma unroll
                for (int u = 0; u < DIF_U; ++u) { ca[u] = na[u]; cm[u] = nm[u]; }
            }
        }
    }
    for (; k < ktot; ++k) {
        const T t = a[k] * y;
        y = (x[k] - t) * m[k];
        x[k] = y;
    }
    // back substitution: y holds x'[ktot - 1]
    k = ktot - 2;
    if (k - DIF_U + 1 >= 0) {
        T cc[DIF_U];
#pragma unroll
        for (int u = 0; u < DIF_U; ++u) cc[u] = cp[k - u];
        for (; k - DIF_U + 1 >= 0; k -= DIF_U) {
            const bool more = k - 2 * DIF_U + 1 >= 0;
            T nc[DIF_U], cx[DIF_U];
            if (more) {
#pragma unroll
                for (int u = 0; u < DIF_U; ++u) nc[u] = cp[k - DIF_U - u];
            }
#pragma unroll
            for (int u = 0; u < DIF_U; ++u) cx[u] = x[k - u];
#pragma unroll
            for (int u = 0; u < DIF_U; ++u) {
                const T t = cc[u] * y;
                y = cx[u] - t;
                x[k - u] = y;
            }
            if (more) {
#pragma unroll
                for (int u = 0; u < DIF_U; ++u) cc[u] = nc[u];
            }
        }
    }
    for (; k >= 0; --k) {
        const T t = cp[k] * y;
        y = x[k] - t;
        x[k] = y;
    }
}

// grid (ceil(ncols / C), n_fields); dynamic LDS: C * col_pitch(ktot, 0) elements, and 3 * DIF_STAGE * ktot more where p.stage
template <typename T, int C> __global__ __launch_bounds__(DIF_THREADS) void k_les_diffuse(const LesDiffuseP<T> p)
{
    extern __shared__ __align__(16) unsigned char dif_lds[];
    T *tile = reinterpret_cast<T *>(dif_lds);
    const int f = blockIdx.y;
    const int ktot = p.ktot, P = col_pitch(ktot, 0);
    const int64_t col0 = (int64_t)blockIdx.x * C;
    const int64_t left = p.ncols - col0;
    const int nc = left < C ? (int)left : C;                     // the last tile is partial
    T *run = p.field[f] + col0 * ktot;
    col_move<T, DIF_THREADS, DIF_UB, false>(run, tile, nc * ktot, ktot, P);
    // the rows of a, m and cp of the tile's LES, [3][DIF_STAGE][ktot] behind the columns, where the tile spans at most p.stage LES
    const int64_t l0 = col0 / p.nij;
    const int nl = (int)((col0 + nc - 1) / p.nij - l0) + 1;
    const bool staged = nl <= p.stage;                           // the same for every lane of the workgroup
    T *prof = tile + C * P;
    if (staged) {
        for (int e = threadIdx.x; e < 3 * nl * ktot; e += DIF_THREADS) {
            const int r = e / ktot, k = e - r * ktot;
            const int which = r / nl, dl = r - which * nl;
            const T *src = which == 0 ? p.a : (which == 1 ? p.m : p.cp);
            prof[(which * DIF_STAGE + dl) * ktot + k] = src[(l0 + dl) * p.pitch_prof + k];
        }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < nc) {
        const int64_t l = (col0 + c) / p.nij;                    // per lane: a tile may span several LES
        const int64_t o = l * p.pitch_prof;
        T *x = tile + c * P;
        T d = x[0];
        const T *flux = p.flux[f];
        if (flux) {
            const T t = p.s0[l] * flux[l];
            d = d + t;
        }
        if (staged) {
            const T *row = prof + (int)(l - l0) * ktot;
            dif_column<T>(x, row, row + DIF_STAGE * ktot, row + 2 * DIF_STAGE * ktot, d, ktot);
        } else {
            dif_column<T>(x, p.a + o, p.m + o, p.cp + o, d, ktot);
        }
    }
    __syncthreads();
    col_move<T, DIF_THREADS, DIF_UB, true>(run, tile, nc * ktot, ktot, P);
}

#else  // SPC_DIFFUSE_HOST ---------------------------------------------------------------------------------------------------

template <typename T> static int les_diffuse_impl(const spc_les_diffuse_args *a, void *stream)
{
    if (!a) return fail(SPC_ERR_INVALID_ARGUMENT, "%sargs is NULL");
    int rc = slab_check_extents("les_diffuse", a->n_les, a->itot, a->jtot, a->ktot);
    if (rc) return rc;
    static_assert(SPC_DIFFUSE_MAX_FIELDS == DIF_MAXF, "include/spc.h and spc_diffuse.hpp disagree on the fields per launch");
    if (a->n_fields < 1 || a->n_fields > SPC_DIFFUSE_MAX_FIELDS)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_diffuse: field count %lld outside 1 ... %lld", "", (long long)a->n_fields, SPC_DIFFUSE_MAX_FIELDS);
    if (a->pitch_prof < a->ktot)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_diffuse: pitch_prof %lld smaller than ktot", "", (long long)a->pitch_prof);
    if (a->n_les == 0) return SPC_OK;
    REQUIRE(a->a, "a"); REQUIRE(a->m, "m"); REQUIRE(a->cp, "cp");
    LesDiffuseP<T> p = {};
    uintptr_t bits = (uintptr_t)a->a | (uintptr_t)a->m | (uintptr_t)a->cp | (uintptr_t)a->s0;
    // (equal base pointers are what is detected, as in K11 and K14: partially overlapping views are the caller's to avoid)
    for (int f = 0; f < a->n_fields; ++f) {
        REQUIRE(a->fields[f], "fields[f]");
        for (int g = 0; g < f; ++g)
            if (a->fields[g] == a->fields[f])
                return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_diffuse: fields[%lld] and fields[%lld] are the same field", "", g, f);
        if (a->fields[f] == a->a || a->fields[f] == a->m || a->fields[f] == a->cp || a->fields[f] == a->s0 || a->fields[f] == a->flux[f])
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_diffuse: fields[%lld] is also a profile, s0 or its flux (it is written while they are read)", "", f);
        if (a->flux[f] && !a->s0)
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_diffuse: flux[%lld] without s0", "", f);
        p.field[f] = (T *)a->fields[f];
        p.flux[f] = (const T *)a->flux[f];
        bits |= (uintptr_t)a->fields[f] | (uintptr_t)a->flux[f];
    }
    if (bits % sizeof(T)) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_diffuse: a pointer is not aligned to its element type");
    const int C = col_cols(a->ktot, (int)sizeof(T), 1, 0);
    if (!C)
        return fail(SPC_ERR_UNSUPPORTED, "%sles_diffuse: ktot %lld above the %lld levels of which 16 columns fit the LDS", "", (long long)a->ktot,
                    (long long)col_max_ktot((int)sizeof(T), 1, 0));
    p.a = (const T *)a->a; p.m = (const T *)a->m; p.cp = (const T *)a->cp; p.s0 = (const T *)a->s0;
    p.nij = a->itot * a->jtot;
    p.ncols = a->n_les * (int64_t)p.nij;
    p.pitch_prof = a->pitch_prof;
    p.ktot = a->ktot;
    return col_dispatch(C, [&](auto c) {
        return col_stage_launch<T>(k_les_diffuse<T, decltype(c)::value>, "k_les_diffuse", "les_diffuse", p, C, 1, a->n_fields, DIF_THREADS, stream);
    });
}

#endif
