/*
 * TEST INFRASTRUCTURE ONLY -- plain-C CPU restatement of the reference coupling math, batched, in float64 and in float32.
 *
 * Second, independent restatement (the first is oracle/spcpl_oracle.py, which calls numpy.interp /
 * numpy.searchsorted like the reference does; its float32 twin is tests/f32_ref.py).  It takes the SAME argument structs
 * as the product's C ABI (include/spc.h) but with HOST pointers, so parity tests hand identical structs to both.
 * It may be linked / loaded only by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
 *
 * Pinning: see the header of oracle/spcpl_oracle.py ("parity unpinned" beyond exner/iexner/rms and
 * the cloud-fraction index map, which the reference's own tests pin).  This file is additionally
 * checked bit-for-bit (interp, indices) / to 1e-13 (pow) against the NumPy oracle in tests/.
 *
 * One body (spc_oracle_body.h), compiled twice: oracle_*_f64 and oracle_*_f32 take the same structs, with double or float
 * arrays.  The float32 contract -- the reference's lines as NumPy 2 evaluates them on float32 arrays:
 *   - every operation is a float32 operation (and -ffp-contract=off: no FMA), quotients are C's correctly rounded float `/`;
 *   - constant expressions the reference writes with Python floats (rv / rd - 1, rd / cp, -rd / cp, 9.81, rlv, cp, pref0)
 *     are NEP 50 weak scalars: evaluated in double and rounded to float ONCE (KR below), as tests/vnudge_f32_ref.py does;
 *   - sums are NumPy's pairwise tree with float32 adds;
 *   - the power is spc_powf_pos (sp_coupler_amd/csrc/spc_powf.h, pinned against the exact power by
 *     tests/test_pow_accuracy.py), with C99 pow()'s special values, instead of the C library's powf NumPy would call.
 * Exceptions, where NumPy itself would compute in float64 and this oracle (like the kernels) stays in float32:
 *   - numpy.interp (sputils.py:86) converts to float64; here it is arr_interp with every operation in float32;
 *   - interp_c / interp_rho (sputils.py:173-197) fill float64 numpy.zeros buffers; here the buffers are float32.
 * The float64 entries are unchanged by this: for R = double every KR(x) is x and POW is pow().
 *
 * Citations are file:line relative to the reference root (/root/reference).
 * Build: see oracle/Makefile (gcc -O2 -ffp-contract=off: no FMA, like the NumPy build).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/spc.h"
#include "../sp_coupler_amd/csrc/spc_powf.h"

/* splib/sputils.py:14-20 */
static const double pref0 = 1e5, rd = 287.04, rv = 461.5, cp = 1004., rlv = 2.53e6, grav = 9.81;

static int check_dims(const spc_dims *d)
{
    if (!d || d->n_cols < 0 || d->nG < 1 || d->nL < 1) return SPC_ERR_INVALID_ARGUMENT;
    if (d->pitchG < d->nG || d->pitchGh < d->nG + 1 || d->pitchL < d->nL) return SPC_ERR_INVALID_ARGUMENT;
    return SPC_OK;
}

/* x ** y in float32: spc_powf_pos with C99 pow()'s values for x outside (0, inf) and a non-integer y (the kernels' spc_pow) */
static float powf_oracle(float x, float y)
{
    if (!(x > 0.0f && x <= 3.4028234663852886e38f)) {
        if (x != x) return x;
        if (x == 0.0f) return y < 0.0f ? HUGE_VALF : 0.0f;
        if (x == HUGE_VALF || x == -HUGE_VALF) return y < 0.0f ? 0.0f : HUGE_VALF;
        return nanf("");
    }
    return spc_powf_pos(x, y);
}

/* exported for tests/f32_ref.py: out[i] = x[i] ** y */
void oracle_powf(const float *x, float y, float *out, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) out[i] = powf_oracle(x[i], y);
}

#define R double
#define FN(name) name##_f64
#define KR(x) ((double)(x))
#define POW(x, y) pow(x, y)
#include "spc_oracle_body.h"
#undef R
#undef FN
#undef KR
#undef POW

#define R float
#define FN(name) name##_f32
#define KR(x) ((float)(x))
#define POW(x, y) powf_oracle(x, y)
#include "spc_oracle_body.h"
#undef R
#undef FN
#undef KR
#undef POW

/* the float64 pairwise sum under its historical name (tests/test_properties.py) */
double oracle_pairwise_sum(const double *a, int64_t n) { return oracle_pairwise_sum_f64(a, n); }
