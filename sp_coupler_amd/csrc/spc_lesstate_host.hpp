// spc_lesstate_host.hpp -- argument checks and launches of K9, the initial LES state of spcpl.set_les_state (kernels, plan and
// jump polynomials: spc_lesstate.hpp); included by spc_hip.hip after spc_launch.hpp (fail, REQUIRE, launch_status, device_cus).
#pragma once

int les_state_check(int64_t n_les, int64_t n_elems, int32_t pos_in)
{
    if (n_les < 0 || n_elems < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_state: negative count");
    if (pos_in < 0 || pos_in > MT_N) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_state: pos %lld outside 0 ... 624", "", pos_in);
    if (n_elems > (int64_t(1) << 58)) return fail(SPC_ERR_UNSUPPORTED, "%sles_state: more than 2^58 elements");
    return SPC_OK;
}

int les_state_impl(const spc_les_state_args *a, void *stream)
{
    REQUIRE(a, "args");
    REQUIRE(a->key_in, "key_in"); REQUIRE(a->key_out, "key_out"); REQUIRE(a->pos_out, "pos_out");
    int rc = les_state_check(a->n_les, 0, a->pos_in);
    if (rc) return rc;
    if (a->n_les > 0) { REQUIRE(a->elem_off, "elem_off"); REQUIRE(a->ktot, "ktot"); }
    const int64_t n = a->n_les;
    if (n > 0 && a->elem_off[0] != 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_state: elem_off[0] must be 0");
    for (int64_t l = 0; l < n; l++) {
        const int64_t V = a->elem_off[l + 1] - a->elem_off[l];
        if (V < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_state: elem_off decreases at LES %lld", "", l);
        if (V >= (int64_t(1) << 30)) return fail(SPC_ERR_UNSUPPORTED, "%sles_state: LES %lld holds 2^30 elements or more", "", l);
        if (a->ktot[l] < 1 || a->ktot[l] > a->pitch_prof || V % a->ktot[l] != 0)
            return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_state: ktot of LES %lld is < 1, > pitch_prof or does not divide its %lld elements", "", l, V);
    }
    const int64_t n_elems = n > 0 ? a->elem_off[n] : 0;
    if ((rc = les_state_check(n, n_elems, a->pos_in))) return rc;
    if (n_elems == 0) {
        memcpy(a->key_out, a->key_in, MT_N * sizeof(uint32_t));
        *a->pos_out = a->pos_in;
        return SPC_OK;
    }
    for (int f = 0; f < 4; f++) {
        REQUIRE(a->prof[f], "prof");
        REQUIRE(a->out[f], "out");
        if ((uintptr_t)a->out[f] % 8 || (uintptr_t)a->prof[f] % 8) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_state: prof / out not 8-byte aligned");
    }
    REQUIRE(a->work, "work");
    const LsPlan pl = ls_plan(8 * n_elems, a->pos_in, a->gens_per_substream, device_cus());
    if (pl.K > 0x7fffffff) return fail(SPC_ERR_UNSUPPORTED, "%sles_state: more than 2^31 substreams");
    const int64_t need = ls_workspace_bytes(n, pl);
    if (a->work_bytes < need) return fail(SPC_ERR_INVALID_ARGUMENT, "%sles_state: work_bytes < %lld", "", need);
    // workspace: key0 | final | elem_off | ktot | states | polynomials
    char *w = (char *)a->work;
    uint32_t *key0 = (uint32_t *)w, *fin = key0 + MT_N;
    int64_t *eo = (int64_t *)(w + ls_align(2 * MT_N * 4));
    int32_t *kt = (int32_t *)((char *)eo + ls_align((n + 1) * 8));
    uint32_t *states = (uint32_t *)((char *)kt + ls_align(n * 4));
    int32_t *coefs = (int32_t *)((char *)states + ls_align(pl.K * MT_N * 4));
    std::vector<int32_t> hpoly((size_t)pl.rounds * MT_DEG), ncoef(pl.rounds, 0);    // set coefficients of each round's g
    for (int b = 0; b < pl.rounds; b++) {
        const Gf2Poly g = mt_jump_poly(((uint64_t)MT_N * (uint64_t)pl.L) << b);
        int32_t *dst = hpoly.data() + (size_t)b * MT_DEG;
        for (int w = 0; w < MT_PW; w++)
            for (uint64_t c = g[w]; c; c &= c - 1) dst[ncoef[b]++] = 64 * w + __builtin_ctzll(c);   // degree < 19937
    }
    hipStream_t st = (hipStream_t)stream;
    // every exit after the first copy waits for the stream: the copies read host memory of this frame (hpoly, key_in ...)
    auto finish = [st](int code) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (code == SPC_OK) return fail(SPC_ERR_LAUNCH, "%sles_state: synchronize failed");
        }
        return code;
    };
    if (hipMemcpyAsync(key0, a->key_in, MT_N * 4, hipMemcpyHostToDevice, st) != hipSuccess
        || hipMemcpyAsync(eo, a->elem_off, (n + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess
        || hipMemcpyAsync(kt, a->ktot, n * 4, hipMemcpyHostToDevice, st) != hipSuccess
        || (pl.rounds && hipMemcpyAsync(coefs, hpoly.data(), hpoly.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess))
        return finish(launch_status("les_state: upload"));
    for (int b = 0; b < pl.rounds; b++) {
        hipLaunchKernelGGL(k_mt_jump, dim3((unsigned)pl.K), dim3(LS_THREADS), 0, st, key0, states, coefs + (size_t)b * MT_DEG, ncoef[b], b,
                           pl.K);
        if ((rc = launch_status("k_mt_jump"))) return finish(rc);
    }
    LsP P;
    P.key0 = key0; P.states = states; P.final_key = fin;
    P.K = pl.K; P.L = pl.L; P.T = pl.T;
    P.p = a->pos_in; P.q = a->pos_in + 8 * n_elems;
    P.elem_off = eo; P.ktot = kt; P.n_les = n; P.pitch = a->pitch_prof;
    for (int f = 0; f < 4; f++) { P.prof[f] = a->prof[f]; P.amp[f] = a->amp[f]; P.out[f] = a->out[f]; }
    hipLaunchKernelGGL(k_les_state, dim3((unsigned)pl.K), dim3(LS_THREADS), 0, st, P);
    if ((rc = launch_status("k_les_state"))) return finish(rc);
    if (pl.T > 0) {
        if (hipMemcpyAsync(a->key_out, fin, MT_N * 4, hipMemcpyDeviceToHost, st) != hipSuccess) return finish(launch_status("les_state: download"));
        *a->pos_out = (int32_t)(P.q - (int64_t)MT_N * pl.T);
    } else {
        memcpy(a->key_out, a->key_in, MT_N * sizeof(uint32_t));
        *a->pos_out = (int32_t)P.q;
    }
    return finish(SPC_OK);
}

int64_t les_state_workspace_impl(int64_t n_les, int64_t n_elems, int32_t pos_in, int64_t gens_per_substream)
{
    const int rc = les_state_check(n_les, n_elems, pos_in);
    if (rc) return rc;
    return ls_workspace_bytes(n_les, ls_plan(8 * n_elems, pos_in, gens_per_substream, device_cus()));
}

// the host jump-ahead on its own (spc_mt19937_jump, spc_mt19937_jump_poly: no device)
int mt_jump_impl(const uint32_t *key_in, int32_t pos_in, int64_t n_words, uint32_t *key_out, int32_t *pos_out)
{
    REQUIRE(key_in, "key_in"); REQUIRE(key_out, "key_out"); REQUIRE(pos_out, "pos_out");
    if (pos_in < 0 || pos_in > MT_N) return fail(SPC_ERR_INVALID_ARGUMENT, "%smt19937_jump: pos %lld outside 0 ... 624", "", pos_in);
    if (n_words < 0 || n_words > INT64_MAX - MT_N) return fail(SPC_ERR_INVALID_ARGUMENT, "%smt19937_jump: n_words out of range");
    mt_jump_host(key_in, pos_in, n_words, key_out, pos_out);
    return SPC_OK;
}

int mt_jump_poly_impl(uint64_t J, uint64_t *out)
{
    REQUIRE(out, "out");
    if (J >> 63) return fail(SPC_ERR_INVALID_ARGUMENT, "%smt19937_jump_poly: J >= 2^63");
    const Gf2Poly g = mt_jump_poly(J);
    memcpy(out, g.data(), MT_PW * sizeof(uint64_t));
    return SPC_OK;
}
