#!/usr/bin/env python3
"""Mutation control of the semantic tests (round-4 verdict, next 2: "each property fails when the corresponding line of the
kernel is perturbed").  Each mutant is ONE slip a transcription of the reference could contain, kept here as text edits of the
kernel sources (MUTANTS); the shipped sources hold only the shipped code.  --build copies sp_coupler_amd/csrc/ to
build/mutants/src<n>/, applies mutant n's edits and compiles build/mutants/libspc_mutant<n>.so (on any host: hipcc
cross-compiles gfx950).  A run without --build (GPU) runs the properties of tests/semantic_props.py through the HIP kernels of
the shipped library and of every mutant library, in ONE process (Engine(lib_path=...)).  Expected: the shipped library passes
all, every mutant fails at least the property that guards its line.  Prints a table; exit status 1 if a mutant survives or
the shipped library fails.  tests/test_mutation_table.py checks on the CPU that every edit still applies to the tree.
Mutants 28 ... are slips of K10 (spc_slab.hpp); their guards are the bodies of tests/slab_edges.py.
Every other kernel has a table numbered on its own, chosen with its flag; TABLES and LATER_TABLES below list them: the flag, the kernel, the
module under tests/ whose bodies guard the table, and the GPU test that runs those bodies on the shipped library.  A run of
such a table ends with the edits of its *_EQUIVALENT table where it has one (edits proved to change no output: expected to
fail NO body) and with the guards that existed before its module on the mutants the new bodies were written for (K8: the
earlier bodies of tests/geo_edges.py; K9: OLD_BODIES of tests/les_state_ref.py; K6: the shape matrix of tests/test_vnudge.py
on every mutant).  CHAIN_MUTANTS (--chain) holds slips of what K10, K11, K12, K14 and K20 share (spc_chain.hpp and their walks); its guards
are the ``chain`` bodies of all five modules.
usage: python tools/mutation_control.py --build [n ...] [-j N]
       python tools/mutation_control.py > profiles/mutation_control.log
       python tools/mutation_control.py --only 28 29 30 31 32 33 34 35 > profiles/mutation_control_slab.log
       python tools/mutation_control.py --<flag> --build && python tools/mutation_control.py --<flag> > profiles/mutation_control_<flag>.log"""
import argparse
import collections
import os
import shutil
import subprocess
import sys
import traceback
from concurrent.futures import ThreadPoolExecutor
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC, HIP_FLAGS  # noqa: E402  (the shipped library's compiler and flags)

CSRC = os.path.join(ROOT, "sp_coupler_amd", "csrc")
OUT = os.path.join(ROOT, "build", "mutants")
K1, K3, K5, K4, VN2, SU = "spc_k1.hpp", "spc_k3.hpp", "spc_k5.hpp", "spc_k4.hpp", "spc_vnudge2.hpp", "spc_sputils.hpp"
VN, VN_HOST = "spc_vnudge.hpp", "spc_vnudge_host.hpp"
SU_HOST = "spc_sputils_host.hpp"
SLAB = "spc_slab.hpp"
CHAIN = "spc_chain.hpp"
ADVANCE = "spc_advance.hpp"
THERMO = "spc_thermo.hpp"
WATERPATH = "spc_waterpath.hpp"
MICRO = "spc_micro.hpp"
DIFFUSE = "spc_diffuse.hpp"
ADVECT = "spc_advect.hpp"
VADVECT = "spc_vadvect.hpp"
RADIATE = "spc_radiate.hpp"
QTLOCAL = "spc_qtlocal.hpp"
MOMENTS = "spc_moments.hpp"
BUOYANCY = "spc_buoyancy.hpp"
MIX = "spc_mix.hpp"
VMIX = "spc_vmix.hpp"
HMIX = "spc_hmix.hpp"
TRANSPORT = "spc_transport.hpp"
TRANSPORT2 = "spc_transport2.hpp"
GEO = "spc_geo.hpp"
LESSTATE = "spc_lesstate.hpp"
LESSTATE_HOST = "spc_lesstate_host.hpp"
A9 = "(col0 + ((c ^ 1) < ncol ? (c ^ 1) : c)) * pitchG"     # the neighbouring column of the slab (mutant 9)


def body_guard(module, name, dtypes=None):
    """guard of a mutant: the body ``name`` of tests/``module``.py on the engines of the library, one per dtype (``dtypes``:
    names of torch dtypes; default the module's DTYPES, float64 and float32)"""
    def guard(engine_of):
        import importlib
        import torch
        m = importlib.import_module("tests." + module)
        failed = []
        for dtype in (m.DTYPES if dtypes is None else [getattr(torch, d) for d in dtypes]):
            failed += m.check_everything(engine_of(dtype))
        return name in failed, sorted(set(failed))
    guard.__name__ = module + "." + name
    return guard


slab_edges = partial(body_guard, "slab_edges")
advance_body = partial(body_guard, "les_advance_ref")
thermo_body = partial(body_guard, "les_thermo_ref")
waterpath_body = partial(body_guard, "les_water_paths_ref")
micro_body = partial(body_guard, "les_micro_ref")
diffuse_body = partial(body_guard, "les_diffuse_ref")
advect_body = partial(body_guard, "les_advect_ref")
vadvect_body = partial(body_guard, "les_vadvect_ref")
radiate_body = partial(body_guard, "les_radiate_ref")
buoyancy_body = partial(body_guard, "les_buoyancy_ref")
mix_body = partial(body_guard, "les_mix_ref")
vmix_body = partial(body_guard, "les_vmix_ref")
hmix_body = partial(body_guard, "les_hmix_ref")
geo_body = partial(body_guard, "geo_edges", dtypes=("float64",))
lesstate_body = partial(body_guard, "les_state_ref", dtypes=("float64",))
qtlocal_body = partial(body_guard, "les_qt_local_ref")
moments_body = partial(body_guard, "les_moments_ref")
vnudge_body = partial(body_guard, "vnudge_edges")
transport_body = partial(body_guard, "les_transport_ref")
transport2_body = partial(body_guard, "les_transport2_ref")
sputils_body = partial(body_guard, "sputils_slabs")


# n: (the slip, the property of tests/semantic_props.py that guards it -- or a callable guard(engine_of) -> (detected, names of
#     everything that failed), engine_of(dtype) an Engine on the library under test,
#     edits: (file under csrc/, exact old text, new text[, occurrences of the old text, default 1]), applied in order)
MUTANTS = {
    1: ("K1 thl: exponent +rd/cp instead of -rd/cp (exner for iexner, sputils.py:28-34)", "isentropic_column_has_constant_thl",
        [(K1, "const T iex = spc_pow(div_pref0(pf), (-K<T>::rd) / K<T>::cp);", "const T iex = spc_pow(div_pref0(pf), K<T>::rd / K<T>::cp);")]),
    2: ("K1 forcings: u_d and v_d swapped (spcpl.py:328-329)", "zero_forcings_when_the_les_equals_the_interpolated_gcm_profile",
        [(K1, "ddt.div(p.factor * (u - in.ud))", "ddt.div(p.factor * (u - in.vd))"),
         (K1, "ddt.div(p.factor * (v - in.vd))", "ddt.div(p.factor * (v - in.ud))")]),
    3: ("K3 f_QL from ql instead of ql_water = ql - ql_ice (spcpl.py:402, 520)", "total_water_tendency_closes",
        [(K3, "T f_QL = ddt.div(p.factor * (qlw_i - in.ql));", "T f_QL = ddt.div(p.factor * (ql_i - in.ql));")]),
    4: ("K3 masking one level too far: k <= start_index (spcpl.py:527-533)", "masking_above_the_les_top",
        [(K3, "if (k < start_index) {", "if (k <= start_index) {")]),
    5: ("K2 index map with side='left' instead of 'right' (spcpl.py:764)", "index_map_is_a_count",
        [(K1, "p.idx[col * pitchG + m] = ss_right(zh, nL, Zh_k);", "p.idx[col * pitchG + m] = ss_left(zh, nL, Zh_k);")]),
    6: ("K1 staging: U not reversed (spcpl.py:227)", "reversal_is_index_arithmetic_only",
        [(K1, "s[4 * nG] = uu;", "(lds + (size_t)c * 6 * nG + k)[4 * nG] = uu;")]),
    7: ("K7 interp_c: numerator without the weight rho (sputils.py:152-154)", "conservative_coarsening_conserves",
        [(SU, "ltn[e] = WEIGHTED ? (wv[u] * qv[u]) * dz : qv[u] * dz;", "ltn[e] = qv[u] * dz;")]),
    8: ("K1 thl: latent term added instead of subtracted (spcpl.py:214)", "isentropic_column_has_constant_thl",
        [(K1, "s[nG] = (tt - div_cp(K<T>::rlv * (ql + qi))) * iex;", "s[nG] = (tt + div_cp(K<T>::rlv * (ql + qi))) * iex;")]),
    9: ("K3 cloud fraction A_d read from the neighbouring column of the slab (spcpl.py:404)", "columns_are_independent",
        [(K3, "load_gcm(p, cg + k, cg + (nG - 1 - k))", "load_gcm(p, cg + k, " + A9 + " + (nG - 1 - k))", 2)]),
    10: ("K5 t: exponent -rd/cp instead of +rd/cp (spcpl.py:409)", "isentropic_column_has_constant_thl",
         [(K5, "thl * spc_pow(div_pref0(pf), K<T>::rd / K<T>::cp)", "thl * spc_pow(div_pref0(pf), (-K<T>::rd) / K<T>::cp)")]),
    11: ("K4 f_T: numerator without the weight rho (spcpl.py:482, sputils.py:152)", "conservative_coarsening_conserves",
         [(K4, "s[0] = w * t;", "s[0] = t;")]),
    12: ("K1 qt_ = SH + QL, the ice forgotten (spcpl.py:215)", "reversal_is_index_arithmetic_only",
         [(K1, "s[2 * nG] = sh + ql + qi;", "s[2 * nG] = sh + ql;")]),
    13: ("K3 f_SH from qt instead of qt - ql (spcpl.py:519: SH is vapour only)", "total_water_tendency_closes",
         [(K3, "T f_SH = ddt.div(p.factor * ((qt_i - ql_i) - in.sh));", "T f_SH = ddt.div(p.factor * (qt_i - in.sh));")]),
    14: ("K1 f_ps with the opposite sign (spcpl.py:332)", "zero_forcings_when_the_les_equals_the_interpolated_gcm_profile",
         [(K1, "Divisor<T>(p.dt).div(p.factor * (sc_ps - sc_psd))", "Divisor<T>(p.dt).div(p.factor * (sc_psd - sc_ps))")]),
    15: ("K1 surface branch: density from T at the model top instead of the lowest level (spcpl.py:153)",
         "surface_fluxes_are_the_ifs_fluxes_over_the_surface_density",
         [(K1, "ldg(&p.Tm[col * pitchG + (nG - 1)])", "ldg(&p.Tm[col * pitchG + 0])")]),
    16: ("k_surface: wqt without the ice flux QIflux (spcpl.py:159)", "surface_fluxes_are_the_ifs_fluxes_over_the_surface_density",
         [(K5, "wqt[i] = -(QLflux[i] + QIflux[i] + SHflux[i]) / rho;", "wqt[i] = -(QLflux[i] + T(0) + SHflux[i]) / rho;")]),
    17: ("K1 surface branch: wthl with exner instead of iexner (spcpl.py:161)", "surface_fluxes_are_the_ifs_fluxes_over_the_surface_density",
         [(K1, "spc_pow(div_pref0(sc_ps), (-K<T>::rd) / K<T>::cp)", "spc_pow(div_pref0(sc_ps), K<T>::rd / K<T>::cp)")]),
    18: ("K6 update: qt += (beta - 1) qt, the level mean forgotten (spcpl.py:724)", "variability_nudge_reaches_the_gcm_cloud_amount",
         [(VN2, "v = (T)((double)v + coef * (double)(v - qt_av));", "v = (T)((double)v + coef * (double)v);")]),
    19: ("K6 constantT: dTHL with the opposite sign (spcpl.py:731)", "variability_nudge_reaches_the_gcm_cloud_amount",
         [(VN2, "s_tc[k] = th ? (-K<T>::rlv) / (", "s_tc[k] = th ? K<T>::rlv / (")]),
    20: ("K6: 'significant cloud' threshold 1e-6 instead of 1e-9 (spcpl.py:665)", "variability_nudge_reaches_the_gcm_cloud_amount",
         [(VN2, "if (ql_ref > 1e-9) {", "if (ql_ref > 1e-6) {")]),
    21: ("K6 additive noise subtracted instead of added (spcpl.py:716-719)", "variability_nudge_reaches_the_gcm_cloud_amount",
         [(VN2, "v = (T)((double)v + coef * R[ij]);", "v = (T)((double)v - coef * R[ij]);")]),
    22: ("K3 f_U from the LES v instead of u (spcpl.py:524)", "tendencies_relax_the_gcm_towards_the_les_profile",
         [(K3, "T f_U = ddt.div(p.factor * (u_i - in.u));", "T f_U = ddt.div(p.factor * (v_i - in.u));")]),
    23: ("K1 rainrate with the opposite sign (spcpl.py:325)", "tendencies_relax_the_gcm_towards_the_les_profile",
         [(K1, "OPT(rainrate)[col] = (sc_rain - sc_rl) / p.dt;", "OPT(rainrate)[col] = (sc_rl - sc_rain) / p.dt;")]),
    24: ("K3 f_T with the opposite sign (spcpl.py:518)", "tendencies_relax_the_gcm_towards_the_les_profile",
         [(K3, "T f_T = ddt.div(p.factor * (t_i - in.tt));", "T f_T = ddt.div(p.factor * (in.tt - t_i));")]),
    25: ("K5 Tv: the condensate load added instead of subtracted (spcpl.py:176)", "gcm_level_diagnostics_mean_what_their_names_say",
         [(K5, "tt * (T(1) + cc * sh - (ql + qi))", "tt * (T(1) + cc * sh - (-(ql + qi)))")]),
    26: ("K5 QT without the ice (spcpl.py:215)", "gcm_level_diagnostics_mean_what_their_names_say",
         [(K5, "stg<WT>(&p.QT[g], sh + ql + qi);", "stg<WT>(&p.QT[g], sh + ql + T(0));")]),
    27: ("K5 Zh above the lowest FULL-level interface instead of the surface (spcpl.py:197)",
         "gcm_level_diagnostics_mean_what_their_names_say",
         [(K5, "stg<WT>(&p.Zh[gh + k], div_grav(ldg(&p.Zghalf[gh + k]) - ldg(&p.Zghalf[gh + nG])));",
           "stg<WT>(&p.Zh[gh + k], div_grav(ldg(&p.Zghalf[gh + k]) - ldg(&p.Zghalf[gh + (nG - 1)])));")]),
    # K10 (spc_slab.hpp).  Every mutant only computes wrong numbers: none reads or writes outside what the shipped kernel
    # touches.  The guards `b < nb` of the loads and `q < nb` of the count loop of k_slab_cloud_count are a redundant pair:
    # dropping either ALONE changes no output (rows past nb load as 0 and count nothing; masks of rows past nb are never
    # counted), and dropping only the load guard reads past the field.  Mutant 28 is the slip both of them guard against, with
    # the row index clamped so that it stays inside the field: the last row is loaded and counted for the missing ones.
    28: ("K10 cloud count: a wave with fewer than SLAB_CF_RB rows left loads and counts SLAB_CF_RB rows (the last one again)",
         slab_edges("cloud_plane"),
         [(SLAB, "x[b] = (b < nb && k < ktot) ? base[(int64_t)(row + b) * ktot + k] : (T)0;",
           "x[b] = (k < ktot) ? base[(int64_t)min(row + b, row1 - 1) * ktot + k] : (T)0;"),
          (SLAB, "for (int q = 0; q < nb; ++q) c +=", "for (int q = 0; q < SLAB_CF_RB; ++q) c +=")]),
    29: ("K10 slab_any_bit: a layer that ends ON a 64-level word boundary masks the whole word away (hi <= b0 + 64)",
         slab_edges("cloud_layers"),
         [(SLAB, "if (hi < b0 + 64) m &= (1ull << (hi - b0)) - 1ull;", "if (hi <= b0 + 64) m &= (1ull << (hi - b0)) - 1ull;")]),
    30: ("K10 cloud count: the final sum over the waves runs once, layers r >= 256 never reach the output",
         slab_edges("cloud_layers"),
         [(SLAB, "    for (int r = tid; r < nG; r += SLAB_THREADS) {\n        int c = 0;",
           "    for (int r = tid; r < min(nG, SLAB_THREADS); r += SLAB_THREADS) {\n        int c = 0;")]),
    31: ("K10 layer bounds: a negative index clipped as an unsigned number (to ktot instead of 0)",
         slab_edges("cloud_layers"),
         [(SLAB, "const int hi = min(max(idx[r], 0), ktot);", "const int hi = (int)min((unsigned)idx[r], (unsigned)ktot);")]),
    32: ("K10 slab means: the remainder loop starts at r + 1 (the last row of a plane with nij % 8 != 0 left out)",
         slab_edges("means_plane"),
         [(SLAB, "    for (; r < p.nij; ++r) {", "    for (++r; r < p.nij; ++r) {")]),
    33: ("K10 slab means, ktot == 1: a sequential sum instead of numpy's pairwise one", slab_edges("means_k1"),
         [(SLAB, "const T sum = vn_npsum([&](int i) { return src[i]; }, p.nij);",
           "T sum = (T)0;\n    for (int i = 0; i < p.nij; ++i) sum += src[i];")]),
    34: ("K10 slab_any_bit: the first level of a layer that starts inside a word is masked away (lo - b0 + 1)",
         slab_edges("cloud_layers"),
         [(SLAB, "if (lo > b0) m &= ~0ull << (lo - b0);", "if (lo > b0) m &= (~0ull << (lo - b0)) << 1;")]),
    35: ("K10 cloud count: the per-wave counters of layers r >= 256 are added to the counters of wave 0 only",
         slab_edges("cloud_layers"),
         [(SLAB, "for (int w = 0; w < SLAB_CF_WAVES; ++w) c += cnt[w * nG + r];",
           "for (int w = 0; w < (r < SLAB_THREADS ? SLAB_CF_WAVES : 1); ++w) c += cnt[w * nG + r];")]),
}



# K11 (spc_advance.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches (mutant 6 stores the rows of the batch before once more, inside the field).
_OLD = [(ADVANCE, "    if (upd) {\n#pragma unroll\n        for (int v = 0; v < V; ++v) x.v[v] = x.v[v] + inc.v[v];",
         "    const SlabVec<T, V> old = x;\n    if (upd) {\n#pragma unroll\n        for (int v = 0; v < V; ++v) x.v[v] = x.v[v] + inc.v[v];")]
ADVANCE_MUTANTS = {
    1: ("K11 update: tend * dt contracted into the add (one rounding, an fma, instead of two)", advance_body("parity"),
        [(ADVANCE, "for (int v = 0; v < V; ++v) inc.v[v] = t.v[v] * p.dt;", "for (int v = 0; v < V; ++v) inc.v[v] = t.v[v];"),
         (ADVANCE, "const SlabVec<T, V> &inc, bool upd, T *dst, T *ql,", "const SlabVec<T, V> &inc, bool upd, T dtm, T *dst, T *ql,"),
         (ADVANCE, "inc, upd, dst", "inc, upd, p.dt, dst", 2),
         (ADVANCE, "x.v[v] = x.v[v] + inc.v[v];", "x.v[v] = __builtin_fma(inc.v[v], dtm, x.v[v]);")]),
    2: ("K11 update: the last row (itot-1, jtot-1) of a plane that ends in single rows is summed but not updated",
        advance_body("parity"),
        [(ADVANCE, "adv_row<T, V, SAT>(x1, s1, inc, upd, dst, ql, acc, accq);", "adv_row<T, V, SAT>(x1, s1, inc, upd && r + 1 < nij, dst, ql, acc, accq);")]),
    3: ("K11 saturation: q taken from QT before its update", advance_body("parity"),
        _OLD + [(ADVANCE, "const T d = x.v[v] - s.v[v];", "const T d = old.v[v] - s.v[v];")]),
    4: ("K11 saturation: d >= 0 keeps d, so d == -0.0 gives -0.0", advance_body("special"),
        [(ADVANCE, "q.v[v] = d > (T)0 ? d : (d != d ? d : (T)0);", "q.v[v] = d >= (T)0 ? d : (d != d ? d : (T)0);")]),
    5: ("K11 means: the sum taken of the field before its update", advance_body("parity"),
        _OLD + [(ADVANCE, "for (int v = 0; v < V; ++v) acc.v[v] += x.v[v];", "for (int v = 0; v < V; ++v) acc.v[v] += old.v[v];")]),
    6: ("K11 look-ahead: the guard of the next batch off by one (r + 2 U < nij): the last whole batch is not loaded", advance_body("planes"),
        [(ADVANCE, "const bool more = r + 2 * U <= nij;", "const bool more = r + 2 * U < nij;")]),
}



# K12 (spc_thermo.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches (mutant 1 keeps the index inside the table).
THERMO_MUTANTS = {
    1: ("K12 lookup: the knot index off by one (the segment above the one that holds Tc)", thermo_body("parity"),
        [(THERMO, "const int m = x >= (T)0 ? min((int)x, P.n_tab - 2) : 0;", "const int m = x >= (T)0 ? min((int)x + 1, P.n_tab - 2) : 0;")]),
    2: ("K12 lookup: the weight w taken from the unclamped Tk (extrapolation beyond the ends of the table)", thermo_body("special"),
        [(THERMO, "const T w = x - (T)m;", "const T w = (Tk - P.t_lo) * P.inv_step - (T)m;")]),
    3: ("K12 qs: om = 1 - eps replaced by eps in the denominator", thermo_body("parity"),
        [(THERMO, "const T den = p - ThermoK<T>::om * e;", "const T den = p - ThermoK<T>::eps * e;")]),
    4: ("K12 Newton: the branch taken with qt >= qs instead of qt > qs", thermo_body("table"),
        [(THERMO, "Tk = qt > s ? Tk - step : Tl;", "Tk = qt >= s ? Tk - step : Tl;")]),
    5: ("K12: the final sat call dropped, qs is the one of the last iteration's Tk", thermo_body("parity"),
        [(THERMO, "T Tk = Tl, dqs;", "T Tk = Tl, dqs, last = (T)0;"),
         (THERMO, "const T s = th_sat<T, true>(P, es, Tk, p, epsp, dqs);", "const T s = last = th_sat<T, true>(P, es, Tk, p, epsp, dqs);"),
         (THERMO, "qs = th_sat<T, false>(P, es, Tk, p, epsp, dqs);", "qs = P.n_iter > 0 ? last : th_sat<T, false>(P, es, Tk, p, epsp, dqs);")]),
    6: ("K12 q rule: dq >= 0 keeps dq, so dq == -0.0 gives -0.0", thermo_body("table"),
        [(THERMO, "q = dq > (T)0 ? dq : (dq != dq ? dq : (T)0);", "q = dq >= (T)0 ? dq : (dq != dq ? dq : (T)0);")]),
    7: ("K12 means: the sums divided by itot * jtot + 1", thermo_body("parity"),
        [(THERMO, "const T cnt = (T)nij;", "const T cnt = (T)(nij + 1);")]),
    8: ("K12 dqs: the factor inv_step (5 entries per kelvin) missing from the slope", thermo_body("parity"),
        [(THERMO, "if (DQS) dqs = (epsp * (d * P.inv_step)) / (den * den);", "if (DQS) dqs = (epsp * d) / (den * den);")]),
}



# K13 (spc_waterpath.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches (mutant 6 reads the weight row of the LES before, LES 0 its own; mutant 8 adds to cover[0], inside the output).  A row offset truncated to 32 bits
# is not in the table: it shows only in a field of more than 2^31 elements, where it reads in front of the field.
_WP_SEQ = """    if (n <= WP_MAXK) {                                      // (mutant) the k loop
        T res = T(0);
        for (int i = 0; i < n; ++i) {
            const T x = ldg(a + lo + i);
            res += x * ldg(w + lo + i);
            top = x > T(0) ? lo + i : top;
        }
        return res;
    }
    const int n8 = n - (n % 8);"""
WATERPATH_MUTANTS = {
    1: ("K13 sum: the row summed in order of k instead of pairwise with eight accumulators", waterpath_body("parity"),
        [(WATERPATH, "    const int n8 = n - (n % 8);", _WP_SEQ)]),
    2: ("K13 product: field * w contracted into the add (one rounding, an fma, instead of two)", waterpath_body("parity"),
        [(WATERPATH, "        rj += x * ldg(w + k);", "        rj = __builtin_fma(x, ldg(w + k), rj);"),
         (WATERPATH, "rj += x0 * w0; rj += x1 * w1; rj += x2 * w2; rj += x3 * w3;",
          "rj = __builtin_fma(x0, w0, rj); rj = __builtin_fma(x1, w1, rj); rj = __builtin_fma(x2, w2, rj); rj = __builtin_fma(x3, w3, rj);")]),
    3: ("K13 tree: the split point n2 = n / 2 not rounded down to a multiple of 8", waterpath_body("parity"),
        [(WATERPATH, "        n2 -= n2 % 8;\n        const T left", "        const T left"),
         (WATERPATH, "                n2 -= n2 % 8;\n                s_right", "                s_right")]),
    4: ("K13 cloud test: field >= 0 instead of field > 0 (zeros and -0.0 are cloudy)", waterpath_body("cloud"),
        [(WATERPATH, "x > T(0) ? lo + i : top;", "x >= T(0) ? lo + i : top;", 2),
         (WATERPATH, "top = v0 > T(0) ? lo + j : top;", "top = v0 >= T(0) ? lo + j : top;"),
         (WATERPATH, "top = x > T(0) ? k : top;", "top = x >= T(0) ? k : top;"),
         (WATERPATH, "top = x0 > T(0) ? k : top; top = x1 > T(0) ? k + 8 : top; top = x2 > T(0) ? k + 16 : top; top = x3 > T(0) ? k + 24 : top;",
          "top = x0 >= T(0) ? k : top; top = x1 >= T(0) ? k + 8 : top; top = x2 >= T(0) ? k + 16 : top; top = x3 >= T(0) ? k + 24 : top;")]),
    5: ("K13 top: taken from the lowest cloudy k instead of the highest", waterpath_body("cloud"),
        [(WATERPATH, "x > T(0) ? lo + i : top;", "x > T(0) && top < 0 ? lo + i : top;", 2),
         (WATERPATH, "top = v0 > T(0) ? lo + j : top;", "top = v0 > T(0) && top < 0 ? lo + j : top;"),
         (WATERPATH, "top = x > T(0) ? k : top;", "top = x > T(0) && top < 0 ? k : top;"),
         (WATERPATH, "top = x0 > T(0) ? k : top; top = x1 > T(0) ? k + 8 : top; top = x2 > T(0) ? k + 16 : top; top = x3 > T(0) ? k + 24 : top;",
          "top = x0 > T(0) && top < 0 ? k : top; top = x1 > T(0) && top < 0 ? k + 8 : top; top = x2 > T(0) && top < 0 ? k + 16 : top; "
          "top = x3 > T(0) && top < 0 ? k + 24 : top;"),
         (WATERPATH, "    top = max(top, __shfl_xor(top, 1));\n    top = max(top, __shfl_xor(top, 2));\n    top = max(top, __shfl_xor(top, 4));",
          "    for (int m = 1; m < 8; m <<= 1) { const int o = __shfl_xor(top, m); top = top < 0 ? o : (o < 0 ? top : min(top, o)); }")]),
    6: ("K13 weights: the row of LES l - 1 (LES 0 keeps its own)", waterpath_body("parity"),
        [(WATERPATH, "const T *const wr = p.w + l * p.pitch_w;", "const T *const wr = p.w + (l > 0 ? l - 1 : 0) * p.pitch_w;")]),
    7: ("K13 cover: the count divided by itot * jtot + 1", waterpath_body("cloud"),
        [(WATERPATH, "p.cover[l] = (T)c / (T)p.nij;", "p.cover[l] = (T)c / (T)(p.nij + 1);")]),
    8: ("K13 cover: a dead group of a wave counts as LES 0 (the row it walks on), so a wave of fewer than 8 live rows over several "
        "LES adds them all to the first", waterpath_body("few_rows"),
        [(WATERPATH, "const int64_t lc = live ? l : -1;", "const int64_t lc = l;")]),
}



# K14 (spc_micro.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches (mutant 3 reads level 0 of the lane's own column; mutant 2 uses the lane's own new values, so it
# shows where a lane owns more than one element).
MICRO_MUTANTS = {
    1: ("K14 s: the accretion product and the sum contracted to an fma", micro_body("parity"),
        [(MICRO, "T s = P.ka * xx + (P.kc * ql) * qs;", "T s = (T)__builtin_fma((double)(P.kc * ql), (double)qs, (double)(P.ka * xx));")]),
    2: ("K14 sedimentation: the NEW qr of the level above on the upwind side (the lane's own elements, top down)", micro_body("parity"),
        [(MICRO, "    for (int v = 0; v < V; ++v) {\n        const T qr = x.qr.v[v], ql = x.ql.v[v];", "    for (int v = V - 1; v >= 0; --v) {\n        const T qr = x.qr.v[v], ql = x.ql.v[v];"),
         (MICRO, "const T qu = v + 1 < V ? x.qr.v[v + 1 < V ? v + 1 : v] : x.up;", "const T qu = v + 1 < V ? nqr.v[v + 1 < V ? v + 1 : v] : x.up;")]),
    3: ("K14 top level: qr_up is level 0 of the same column instead of +0.0", micro_body("neighbour"),
        [(MICRO, "x.up = top ? (T)0 : P.qr[o + V];", "x.up = P.qr[top ? o + V - P.ktot : o + V];")]),
    4: ("K14 cap: s >= ql takes ql, so s == +0.0 against ql == -0.0 becomes -0.0", micro_body("special"),
        [(MICRO, "s = s > ql ? ql : s;", "s = s >= ql ? ql : s;")]),
    5: ("K14 cloud ice: ql instead of ql - s", micro_body("parity"),
        [(MICRO, "qi.v[v] = (ql - s) * fi;", "qi.v[v] = ql * fi;")]),
    6: ("K14 surface rain: the flux out of the lane's second element (k == 1) instead of k == 0", micro_body("parity"),
        [(MICRO, "if (v == 0) out0 = out;", "if (v == (V > 1 ? 1 : 0)) out0 = V > 1 ? out : (T)0;")]),
    7: ("K14 means: the sums divided by itot * jtot + 1", micro_body("parity"),
        [(MICRO, "const T cnt = (T)nij;", "const T cnt = (T)(nij + 1);")]),
    8: ("K14 threshold: x without the NaN branch (shows with a NaN qc0: a NaN ql reaches s through the accretion anyway)", micro_body("special"),
        [(MICRO, "const T xx = d > (T)0 ? d : (d != d ? d : (T)0);", "const T xx = d > (T)0 ? d : (T)0;")]),
}




# K16 (spc_advect.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches (mutant 1 reads row i for row i + 1 at the last row; mutant 2 wraps j - 1 by the SMALLER of itot and
# jtot rows, which stays inside the run of the row -- wrapping by itot rows where itot > jtot would leave it; mutant 8 reads
# u[ip], which the east face reads anyway).
ADVECT_MUTANTS = {
    1: ("K16 ip: clamped at the last row instead of wrapped to row 0", advect_body("parity"),
        [(ADVECT, "const int ip = i + 1 == itot ? 0 : i + 1;", "const int ip = i + 1 == itot ? i : i + 1;")]),
    2: ("K16 jm: wrapped by itot rows (where itot < jtot) instead of jtot", advect_body("parity"),
        [(ADVECT, "        if (qs < 0) qs += row;", "        if (qs < 0) qs += (int64_t)(p.itot < p.jtot ? p.itot : p.jtot) * ktot;")]),
    3: ("K16 pe: taken from ce > 0 (the east face lets in what leaves)", advect_body("signs"),
        [(ADVECT, "const T pe = ce < (T)0 ? -ce : (T)0;", "const T pe = ce > (T)0 ? ce : (T)0;")]),
    4: ("K16 east term: the product and the add contracted to an fma", advect_body("parity"),
        [(ADVECT, "                r = r + te;", "                r = (T)__builtin_fma((double)pe, (double)de, (double)r);")]),
    5: ("K16 sum: the south and north terms added before the west and east terms", advect_body("parity"),
        [(ADVECT, "                T r = x + tw;\n                r = r + te;\n                r = r + ts;\n                r = r + tn;",
          "                T r = x + ts;\n                r = r + tn;\n                r = r + tw;\n                r = r + te;")]),
    6: ("K16 cs: hx used for hy", advect_body("rows"),
        [(ADVECT, "const T cs = as * hy;", "const T cs = as * hx;")]),
    7: ("K16 cmax: the sum without pn", advect_body("probe"),
        [(ADVECT, "            s = s + pn;\n", "")]),
    8: ("K16 west face: built from u[ip] instead of u[im]", advect_body("parity"),
        [(ADVECT, "const T aw = uw + uc,", "const T aw = ue + uc,")]),
}



# K17 (spc_vadvect.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches (mutant 1 stores M[k] where M[k + 1] belongs, in the same LDS cell; mutant 4 reads r at the clamped
# k + 1; mutant 6 reads x[km], which the cell reads anyway, for the top cell's x[kp]; mutant 7 reads the profiles, hx, hy and
# cmax of the LES of the tile's first column, which the tile touches anyway).
VADVECT_MUTANTS = {
    1: ("K17 M: started one level high (the lower face's flux stored for the upper face)", vadvect_body("parity"),
        [(VADVECT, "            M = M - ce[u];\n            x[k + u] = M;", "            x[k + u] = M;\n            M = M - ce[u];"),
         (VADVECT, "        M = M - x[k];\n        x[k] = M;", "        const T e1 = x[k];\n        x[k] = M;\n        M = M - e1;")]),
    2: ("K17 M: + e for - e (convergence sends the air down)", vadvect_body("columns"),
        [(VADVECT, "M = M - ce[u];", "M = M + ce[u];"), (VADVECT, "M = M - x[k];", "M = M + x[k];")]),
    3: ("K17 pt: taken from ct > 0 (the upper face lets in what leaves)", vadvect_body("columns"),
        [(VADVECT, "const T pt = ct < (T)0 ? -ct : (T)0;", "const T pt = ct > (T)0 ? ct : (T)0;")]),
    4: ("K17 ct: r of level k + 1 (clamped) for r of level k", vadvect_body("parity"),
        [(VADVECT, "const T ct = Mt * rk;", "const T ct = Mt * p.r[w.l * p.pitch_prof + (k + 1 < ktot ? k + 1 : k)];")]),
    5: ("K17 upper term: the product and the add contracted to an fma", vadvect_body("parity"),
        [(VADVECT, "            y = y + tt;", "            y = (T)__builtin_fma((double)pt, (double)dt, (double)y);")]),
    6: ("K17 kp: the top cell takes the cell below it for the air that enters through the lid", vadvect_body("parity"),
        [(VADVECT, "const int64_t okp = k + 1 < ktot ? o + 1 : o;", "const int64_t okp = k + 1 < ktot ? o + 1 : okm;")]),
    7: ("K17 l: the LES of the tile's first column for every lane", vadvect_body("rows"),
        [(VADVECT, "w.l = l0 + dl;", "w.l = l0;")]),
    8: ("K17 cmax: the sum without pb", vadvect_body("probe"),
        [(VADVECT, "const T s = pb + pt;", "const T s = pt;")]),
}



# K18 (spc_radiate.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches (mutant 1 stores A[k + 1] where A[k] belongs, in the same LDS cell; mutant 2 reads the B of its own
# face twice; mutant 6 keeps both table indices inside the table: with n_tab - 1 alone the upper one would leave it by one
# entry; mutant 7 reads f0 and f1 of the tile's first LES; mutant 8 extrapolates the last segment, whose index the min() keeps).
RADIATE_MUTANTS = {
    1: ("K18 A: started one level off (the depth above the upper face stored for the lower face)", radiate_body("parity"),
        [(RADIATE, "            A = A + ct[u];\n            x[k - u] = A;", "            x[k - u] = A;\n            A = A + ct[u];"),
         (RADIATE, "        A = A + x[k];\n        x[k] = A;", "        const T t1 = x[k];\n        x[k] = A;\n        A = A + t1;")]),
    2: ("K18 F: B for A in the f0 term (the cloud top sees the water below it)", radiate_body("parity"),
        [(RADIATE, "const T Ea = rad_E<T>(etab, A,", "const T Ea = rad_E<T>(etab, B,")]),
    3: ("K18 thl: + for - (a flux that diverges warms)", radiate_body("parity"),
        [(RADIATE, "    return x - t;", "    return x + t;")]),
    4: ("K18 flux: F[k] for F[k + 1] (the flux at the lower face)", radiate_body("outputs"),
        [(RADIATE, "    up = F[k + 1];\n    const T dF = up - lo;", "    const T hi = F[k + 1];\n    up = lo;\n    const T dF = hi - lo;")]),
    5: ("K18 lookup: the product and the add of the interpolation contracted to an fma", radiate_body("parity"),
        [(RADIATE, "    const T t = fr * d;\n    return e0 + t;", "    return (T)__builtin_fma((double)fr, (double)d, (double)e0);")]),
    6: ("K18 lookup: n_tab - 1 for n_tab - 2 (x_hi falls on the last node with fr = 0, not on the last segment with fr = 1)", radiate_body("lookup"),
        [(RADIATE, "min((int)s, n_tab - 2)", "min((int)s, n_tab - 1)"),
         (RADIATE, "const T d = etab[m + 1] - e0;", "const T d = etab[m + 1 < n_tab ? m + 1 : m] - e0;")]),
    7: ("K18 l: the LES of the tile's first column for the f0 and f1 of every lane", radiate_body("rows"),
        [(RADIATE, "const int64_t l = tr.l0 + (tr.rem0 + (uint32_t)c) / (uint32_t)p.nij;", "const int64_t l = tr.l0;")]),
    8: ("K18 lookup: the clamp at x_hi dropped (the last segment extrapolated)", radiate_body("lookup"),
        [(RADIATE, "const T xc = x < (T)0 ? (T)0 : (x > x_hi ? x_hi : x);", "const T xc = x < (T)0 ? (T)0 : x;")]),
}



# K21 (spc_buoyancy.hpp), numbered on its own.  Every mutant changes a VALUE only: no address, loop bound, barrier or launch
# extent differs from the shipped kernels' (mutant 5 makes the chain visit the same ktot cells of its own column of the tile
# in the opposite order; mutant 6 uses the register that already holds phi[ip]).
BUOYANCY_MUTANTS = {
    1: ("K21 tv: the product and the subtraction of t0 contracted to an fma", buoyancy_body("parity"),
        [(BUOYANCY, "    const T tv = tl * m;\n    const T d = tv - p.t0[po];", "    const T d = (T)__builtin_fma((double)tl, (double)m, -(double)p.t0[po]);")]),
    2: ("K21 m: c1 for c2 (liquid water weighed like vapour)", buoyancy_body("parity"),
        [(BUOYANCY, "const T w = p.c2 * ql;", "const T w = p.c1 * ql;")]),
    3: ("K21 tl: the lex term dropped (THL for the liquid-water-free temperature)", buoyancy_body("parity"),
        [(BUOYANCY, "const T e = QL ? p.lex[po] * ql : (T)0;", "const T e = (T)0;")]),
    4: ("K21 chain: + b for - b in q (the lower half layer taken off again)", buoyancy_body("parity"),
        [(BUOYANCY, "            q = f - cb[u];", "            q = f + cb[u];"),
         (BUOYANCY, "        q = f - b;", "        q = f + b;")]),
    5: ("K21 chain: started at k = 0 (integrated upward from the ground)", buoyancy_body("parity"),
        [(BUOYANCY, "{ return ktot - 1 - s; }", "{ return s; }")]),
    6: ("K21 gx: ip for im (phi[ip] - phi[ip])", buoyancy_body("parity"),
        [(BUOYANCY, "const T gx = fp - fm;", "const T gx = fp - fp;")]),
    7: ("K21 dv: hx for hy", buoyancy_body("rows"),
        [(BUOYANCY, "const T dv = hy * gy;", "const T dv = hx * gy;")]),
    8: ("K21 amax: without |dv|", buoyancy_body("parity"),
        [(BUOYANCY, "const T a = au + av;", "const T a = au;")]),
}


# K24 (spc_mix.hpp), numbered on its own.  Every mutant changes a VALUE only: no loop bound, barrier or launch extent differs from
# the shipped kernels', and the one edit inside brackets (mutant 3) reads the lane's other clamped neighbour, an offset the
# shipped kernel reads in the same statement.
MIX_MUTANTS = {
    1: ("K24 d: a added once instead of twice (the normal strains weighed like the shear)", mix_body("parity"),
        [(MIX, "const T a2 = a + a, sh2 = sh * sh;", "const T a2 = a, sh2 = sh * sh;")]),
    2: ("K24 sh: uy - vx (the vorticity for the shear strain)", mix_body("parity"),
        [(MIX, "const T sh = uy + vx;", "const T sh = uy - vx;")]),
    3: ("K24 theta: kq for kp (theta[kq] - theta[kq]: no stratification)", mix_body("clamp"),
        [(MIX, "tu = p.theta[bi + qu];", "tu = p.theta[bi + qd];")]),
    4: ("K24 d: + for - in front of the stratification term (stable air mixes, unstable air does not)", mix_body("special"),
        [(MIX, "d = d - n2;", "d = d + n2;")]),
    5: ("K24 km: the comparison of the cap reversed (the larger of kk and kcap)", mix_body("cap"),
        [(MIX, "p.km[bi + q] = kk < kcap ? kk : kcap;", "p.km[bi + q] = kk > kcap ? kk : kcap;")]),
    6: ("K24 kmax: taken after the cap", mix_body("cap"),
        [(MIX, "top = kk > top ? kk : top;", "top = (kk < kcap ? kk : kcap) > top ? (kk < kcap ? kk : kcap) : top;")]),
    7: ("K24 ke: km[im] for km[ip] (the east face weighed like the west one)", mix_body("parity"),
        [(MIX, "ke = mc + me,", "ke = mc + mw,")]),
    8: ("K24 fe: ay for ax", mix_body("rows"),
        [(MIX, "ce = ke * ax[f],", "ce = ke * ay[f],")]),
}


# K15 (spc_diffuse.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches (mutant 2 reads cp[k + 1] for k <= ktot - 2, mutant 4 the rows of the LES of the tile's first column,
# mutant 6 cp's row in place of a's; mutants 5 and 7 leave a level of the tile as it is).
DIFFUSE_MUTANTS = {
    1: ("K15 forward sweep: the product and the subtraction contracted to an fma", diffuse_body("parity"),
        [(DIFFUSE, "                const T t = ca[u] * y;\n                y = (cx[u] - t) * cm[u];",
          "                y = (T)__builtin_fma(-(double)ca[u], (double)y, (double)cx[u]) * cm[u];")]),
    2: ("K15 back substitution: cp[k + 1] for cp[k] (the levels behind the whole chunks)", diffuse_body("parity"),
        [(DIFFUSE, "const T t = cp[k] * y;", "const T t = cp[k + 1] * y;")]),
    3: ("K15 surface flux: the product and the add contracted to an fma", diffuse_body("parity"),
        [(DIFFUSE, "            const T t = p.s0[l] * flux[l];\n            d = d + t;", "            d = (T)__builtin_fma((double)p.s0[l], (double)flux[l], (double)d);")]),
    4: ("K15 l: the LES of the tile's first column for every lane", diffuse_body("rows"),
        [(DIFFUSE, "const int64_t l = (col0 + c) / p.nij;", "const int64_t l = col0 / p.nij;")]),
    5: ("K15 back substitution: started one level low (level ktot - 2 keeps y)", diffuse_body("parity"),
        [(DIFFUSE, "    k = ktot - 2;", "    k = ktot - 3;")]),
    6: ("K15 forward sweep: a read from cp's rows", diffuse_body("parity"),
        [(DIFFUSE, "dif_column<T>(x, p.a + o, p.m + o, p.cp + o, d, ktot);", "dif_column<T>(x, p.cp + o, p.m + o, p.cp + o, d, ktot);")]),
    7: ("K15 forward sweep: the levels behind the whole chunks stop one short of the top", diffuse_body("parity"),
        [(DIFFUSE, "    for (; k < ktot; ++k) {\n        const T t = a[k] * y;", "    for (; k < ktot - 1; ++k) {\n        const T t = a[k] * y;")]),
    8: ("K15 level 0 without a flux: + 0.0 added, so -0.0 becomes +0.0", diffuse_body("special"),
        [(DIFFUSE, "T d = x[0];", "T d = x[0] + (T)0;")]),
}



# K8 (spc_geo.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches, none changes a barrier or an index; mutant 6 makes the tile loop (uniform over the workgroup) end
# one trip earlier, mutant 9 reads ring_role[r - 1] for r >= 1, which the shipped kernel has read one ring before.
# The bodies exact_tails, tile_seams, image_lon and non_finite_points exist for mutants 1, 6, 14 and 15.  Mutant 2 (no
# tails at all) is also seen by the earlier naive_flips points: 18 of those 28 have a tail in b - c (24.25 - y, 17.3 - x) and
# at 8 of them the head-only expansion has the wrong sign; none has a tail in a - c (0.5 - x, 0.5 - y are exact), which is
# what mutant 1 drops, and none is collinear.  GEO_OLD_GUARDS names the mutants on which the run ends by showing what the
# guards from before tests/geo_edges.py make of them.
_STORE = "p.out[(int64_t)cur_poly * p.n_points + i] = finite ? (uint16_t)(code_p | (code_q << 8)) : (uint16_t)GEO_EXTERIOR;"
GEO_MUTANTS = {
    1: ("K8 exact orientation: the four two-products with the tails of a - c left out (8 of the 16 terms summed)", geo_body("exact_tails"),
        [(GEO, "geo_two_prod(acx[i], bcy[j], t[4 * i + 2 * j], t[4 * i + 2 * j + 1]);",
          "geo_two_prod(i ? 0.0 : acx[i], bcy[j], t[4 * i + 2 * j], t[4 * i + 2 * j + 1]);"),
         (GEO, "geo_two_prod(-acy[i], bcx[j], t[8 + 4 * i + 2 * j], t[8 + 4 * i + 2 * j + 1]);",
          "geo_two_prod(i ? 0.0 : -acy[i], bcx[j], t[8 + 4 * i + 2 * j], t[8 + 4 * i + 2 * j + 1]);")]),
    2: ("K8 exact orientation: TwoDiff replaced by a plain difference (no tails)", geo_body("exact_tails"),
        [(GEO, "    e = (a - (d + bb)) + (bb - b);", "    e = 0.0 * bb;")]),
    3: ("K8 orientation: the filter's error bound replaced by 0 (the naive sign decides)", geo_body("naive_flips"),
        [(GEO, "const double errbound = 3.3306690738754716e-16 * detsum;", "const double errbound = 0.0 * detsum;")]),
    4: ("K8 segment: 'wholly to the left' with <= (a vertical edge through the point is skipped)", geo_body("adversarial"),
        [(GEO, "if (x1 < px && x2 < px) return;", "if (x1 <= px && x2 <= px) return;")]),
    5: ("K8 segment: upward edges include their end as well as their start (a ray through a vertex crosses both its edges)",
        geo_body("adversarial"),
        [(GEO, "if ((y1 > py && y2 <= py) || (y2 > py && y1 <= py)) {", "if ((y1 > py && y2 <= py) || (y2 >= py && y1 <= py)) {")]),
    6: ("K8 tiles: a last tile that holds exactly one edge is skipped (t0 + 2 < e)", geo_body("tile_seams"),
        [(GEO, "for (int64_t t0 = s; t0 + 1 < e; t0 += GEO_TILE) {", "for (int64_t t0 = s; t0 + 2 < e; t0 += GEO_TILE) {")]),
    7: ("K8 segment: o = -o dropped for downward edges", geo_body("adversarial"),
        [(GEO, "if (y2 < y1) o = -o;  ", "                      ")]),
    8: ("K8 fold: a hole's BOUNDARY folded to INTERIOR", geo_body("adversarial"),
        [(GEO, "ring_code == GEO_BOUNDARY ? GEO_BOUNDARY : GEO_INTERIOR;", "ring_code == GEO_BOUNDARY ? GEO_INTERIOR : GEO_INTERIOR;")]),
    9: ("K8 fold: every hole after a polygon's first is ignored", geo_body("adversarial"),
        [(GEO, "        code_p = geo_fold(code_p, rp, role);\n        code_q = geo_fold(code_q, rq, role);",
          "        if (!(role == SPC_RING_HOLE && r >= 1 && p.ring_role[r - 1] == SPC_RING_HOLE)) {\n"
          "            code_p = geo_fold(code_p, rp, role);\n            code_q = geo_fold(code_q, rq, role);\n        }")]),
    10: ("K8 rectangle rule with <= (the bounds belong to the rectangle)", geo_body("adversarial"),
         [(GEO, "rp = in_y && x0 < px && px < x1 ? GEO_INTERIOR : GEO_EXTERIOR;", "rp = in_y && x0 <= px && px <= x1 ? GEO_INTERIOR : GEO_EXTERIOR;")]),
    11: ("K8 image: r += 360 dropped (C's fmod instead of Python's %)", geo_body("adversarial"),
         [(GEO, "if (r < 0.0) r += 360.0;", "if (r < 0.0) r += 0.0;")]),
    12: ("K8 store: q's code in the low byte, p's in the high byte", geo_body("adversarial"),
         [(GEO, _STORE, _STORE.replace("code_p | (code_q << 8)", "code_q | (code_p << 8)"), 2)]),
    13: ("K8 haversine: dlat and dlng swapped in the sines", geo_body("haversine"),
         [(GEO, "const double sl = sin((lat2 - lat1) * 0.5), sg = sin((lng2 - lng1) * 0.5);",
           "const double sl = sin((lng2 - lng1) * 0.5), sg = sin((lat2 - lat1) * 0.5);")]),
    14: ("K8 image: formed as (lon + 180) % 360 - 180 (the sum rounds where the difference is exact)", geo_body("image_lon"),
         [(GEO, "const double x = lon - 180.0;", "const double x = lon + 180.0;")]),
    15: ("K8 non-finite points: only p is made EXTERIOR, q keeps the code its arithmetic gave", geo_body("non_finite_points"),
         [(GEO, _STORE, _STORE.replace(": (uint16_t)GEO_EXTERIOR", ": (uint16_t)(code_q << 8)"), 2)]),
}
#: the mutants of the exact stage and of the tile loop: main_table runs the guards that existed before tests/geo_edges.py
#: on them once (the scale test of tests/test_geo_gpu.py included) and prints what they find; this is information, not a check
GEO_OLD_GUARDS = (1, 2, 6)
# edits proved to change no output (expected to fail no body).  A: r is -0.0 only after fmod(-360 k, 360); -0.0 - 180 and
# +0.0 - 180 are the same double.  B: the crossing rule half-open at the OTHER end throughout (every edge includes its upper
# end and excludes its lower one) is the mirrored convention: a ray through a vertex then counts the edges that leave it
# downwards instead of those that leave it upwards, the parity is the same, and a point on a vertex or on an edge is found
# by the tests before the rule.
GEO_EQUIVALENT = {
    "A": ("K8 image: a zero remainder keeps fmod's sign (r = 0.0 dropped)",
          [(GEO, "        r = 0.0;                  // CPython", "        r = r;                    // CPython")]),
    "B": ("K8 segment: the crossing rule half-open at the other end for upward and downward edges alike (the mirrored convention)",
          [(GEO, "if ((y1 > py && y2 <= py) || (y2 > py && y1 <= py)) {", "if ((y1 >= py && y2 < py) || (y2 >= py && y1 < py)) {")]),
}



# K9 (spc_lesstate.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernels touch, none changes a barrier; mutant 6 drops a loop; mutant 13 plans one generation more when the launch
# ends on the last word of a generation (plan, workspace size and launch all follow the same T: one more twist in LDS, no
# word emitted from it).  Two slips one would list first are NOT here:
# * ls_seek's binary search with < for <= : proved to change no output -- the search then ends on an earlier LES and the
#   loop `while (4 * elem_off[l + 1] <= e) l++` behind it walks to the right one; it is LESSTATE_EQUIVALENT["A"], run to
#   confirm that no body fails.  A search that overshoots instead is not a "wrong numbers" mutant: el = e - 4 off wraps.
# * that loop as an `if` (one LES advanced at most): an element two LES further on gets el >= 4 V, f >= 4, and out[f] is
#   a wild pointer.  Mutants 7 and 8 are the slips of the same lines that stay inside the fields: the level index taken as
#   the slowest dimension, and the cursor's ktot not refreshed when the element crosses into the next LES.
# Mutant 9 writes final_key from workgroup 0 only (its last generation) instead of "from every workgroup": the same slip
# without the race between workgroups that would make the outcome depend on their order.
# Mutant 11 stands for "floor(log2 K) jump rounds instead of ceil": that edit makes k_les_state read substream starts that
# no round wrote -- inside the workspace, but what the allocator left there, possibly the RIGHT starts of an earlier launch
# of the same process, so its outcome is not determined.  The deterministic slip of the same place: the last round applies
# the polynomial of the round before it.  Any K >= 3 shows it, forced_short_substreams included.
# Mutants 12 and 13 were written for the bodies seek_boundaries and odd_substream_counts; LESSTATE_OLD_GUARDS names
# them, and the run ends by showing what the bodies from before tests/les_state_ref.py (OLD_BODIES) make of them: 13 is
# seen by odd_substream_counts alone; 12 is ALSO seen by forced_short_substreams and twist_boundary, because the search
# runs for every thread's first element and their small LES put an LES start there: seek_boundaries closes no demonstrated
# gap (profiles/mutation_control_lesstate.log).
# * 12: ls_seek's search with < is neutral only because everything the cursor holds is set AFTER the walk behind it.  The
#   mutant is that search together with a cursor whose ktot and profile row are those of the LES the search ended on (the
#   walk corrects l, off, end4 and V): wrong exactly when an LES begins on a workgroup's first element, and then the
#   profile of the LES before is added, with its ktot (k < ktot <= pitch, row < n_les: inside prof).
# * 13: T = q div 624 instead of (q - 1) div 624: wrong exactly when the launch ends on the last word of a generation
#   (NumPy leaves pos = 624 and does not twist); the fields are right, the returned state is one twist ahead with pos 0.
LESSTATE_MUTANTS = {
    1: ("K9 uniform: the second word shifted by 5 instead of 6", lesstate_body("mixed_shapes"),
        [(LESSTATE, "(double)(wb >> 6)", "(double)(wb >> 5)")]),
    2: ("K9 straddling double: its second word taken from the current generation (G[0]) instead of the next", lesstate_body("forced_short_substreams"),
        [(LESSTATE, "j + 1 < MT_N ? G[j + 1] : mt_mix(G[0], G[1], G[MT_M])", "j + 1 < MT_N ? G[j + 1] : G[0]")]),
    3: ("K9 emit: the parity correction lo++ dropped (from an odd pos the pairs of later generations start one word early)",
        lesstate_body("forced_short_substreams"),
        [(LESSTATE, "    if ((lo - P.p) & 1) lo++;\n", "")]),
    4: ("K9 twist: word 623 mixed with the OLD word 0 (o[0]) instead of the new one", lesstate_body("mixed_shapes"),
        [(LESSTATE, "nw[j] = mt_mix(o[j], nw[0], nw[MT_M - 1]);", "nw[j] = mt_mix(o[j], o[0], nw[MT_M - 1]);")]),
    5: ("K9 jump rounds: k_mt_jump always starts from key0 (the lower bits' jumps are lost)", lesstate_body("forced_short_substreams"),
        [(LESSTATE, "? states + s * MT_N : key0;", "? key0 : key0;")]),
    6: ("K9 jump rounds: the remainder loop over n_coef % 8 coefficients dropped", lesstate_body("forced_short_substreams"),
        [(LESSTATE, "    for (; q < n_coef; q++) {\n        const int i = coef[q];", "    for (; q < q; q++) {\n        const int i = coef[q];")]),
    7: ("K9 broadcast: the profile level taken as the slowest dimension of the field (idx / (itot * jtot)) instead of the fastest",
        lesstate_body("mixed_shapes"),
        [(LESSTATE, "const uint32_t k = idx % c.kt;", "const uint32_t k = idx / (c.V / c.kt);")]),
    8: ("K9 cursor: ktot not refreshed when an element crosses into the next LES", lesstate_body("mixed_shapes"),
        [(LESSTATE, "    c.kt = (uint32_t)P.ktot[c.l];", "    if (c.kt == 1) c.kt = (uint32_t)P.ktot[c.l];")]),
    9: ("K9 final state: written by workgroup 0 after ITS last generation instead of by the workgroup that twists generation T",
        lesstate_body("forced_short_substreams"),
        [(LESSTATE, "if (gen == P.T)\n", "if (gen == g1 && s == 0)\n")]),
    10: ("K9 amplitude: amp[3 - f], the amplitude of another field", lesstate_body("mixed_shapes"),
         [(LESSTATE, "const double v = P.amp[f] * r;", "const double v = P.amp[3 - f] * r;")]),
    11: ("K9 jump rounds: the last round applies the polynomial of the round before it (x^(624 L 2^(b-1)) for x^(624 L 2^b))",
         lesstate_body("forced_short_substreams"),
         [(LESSTATE_HOST, "const Gf2Poly g = mt_jump_poly(((uint64_t)MT_N * (uint64_t)pl.L) << b);",
           "const Gf2Poly g = mt_jump_poly(((uint64_t)MT_N * (uint64_t)pl.L) << (b > 0 && b + 1 == pl.rounds ? b - 1 : b));")]),
    12: ("K9 ls_seek: the search with <, and the cursor of a thread's first element keeps ktot and the profile row of the LES "
         "the search ended on", lesstate_body("seek_boundaries"),
         [(LESSTATE, "if (4 * P.elem_off[mid] <= e) lo_l = mid; else hi_l = mid - 1;", "if (4 * P.elem_off[mid] < e) lo_l = mid; else hi_l = mid - 1;"),
          (LESSTATE, "    if (c.l < 0) {                                             // the first element",
           "    const bool first = c.l < 0;\n    if (first) {                                             // the first element"),
          (LESSTATE, "        c.l = lo_l;\n", "        c.l = lo_l;\n        c.kt = (uint32_t)P.ktot[c.l];\n        c.row = c.l * P.pitch;\n"),
          (LESSTATE, "    c.kt = (uint32_t)P.ktot[c.l];\n    c.row = c.l * P.pitch;\n}",
           "    if (!first) {\n        c.kt = (uint32_t)P.ktot[c.l];\n        c.row = c.l * P.pitch;\n    }\n}")]),
    13: ("K9 plan: T = q div 624 instead of (q - 1) div 624 (a launch that ends on the last word of a generation twists once more)",
         lesstate_body("odd_substream_counts"),
         [(LESSTATE, "pl.T = q <= MT_N ? 0 : (q - 1) / MT_N;", "pl.T = q <= MT_N ? 0 : q / MT_N;")]),
}
#: the mutants the new bodies were written for: main_table runs OLD_BODIES of tests/les_state_ref.py on them once
LESSTATE_OLD_GUARDS = (12, 13)
LESSTATE_EQUIVALENT = {
    "A": ("K9 ls_seek: the binary search with < for <= (the loop behind it walks to the right LES)",
          [(LESSTATE, "if (4 * P.elem_off[mid] <= e) lo_l = mid; else hi_l = mid - 1;", "if (4 * P.elem_off[mid] < e) lo_l = mid; else hi_l = mid - 1;")]),
}



# K19 (spc_qtlocal.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernels touch and none can hang (mutant 2 reads ql, a field of the shape of qt, on the levels where the shipped kernel
# reads qt; mutant 5 divides by T(0) for the dry share of a level that has no dry cell and never adds it; mutant 6 reads row 0 of
# the two profiles; mutant 7 leaves the counts of the other parts out of the sum, the zeroed words stay zeroed).
QTLOCAL_MUTANTS = {
    1: ("K19 a > 0: qt >= m for qt > m, in both walks (a cell ON the mean is wet)", qtlocal_body("ties"),
        [(QTLOCAL, "mode[v] == 1 ? x[u].v[v] > m[v]", "mode[v] == 1 ? x[u].v[v] >= m[v]"),
         (QTLOCAL, "mode[v] == 1 ? t > m[v]", "mode[v] == 1 ? t >= m[v]")]),
    2: ("K19 a > 0: the predicate of a < 0 (the cloudy cells, not the cells above the mean)", qtlocal_body("parity"),
        [(QTLOCAL, "mode[v] = a[v] > (T)0 ? 1 :", "mode[v] = a[v] > (T)0 ? 2 :")]),
    3: ("K19 shares: N - c and c swapped (the wet cells share what the dry ones should)", qtlocal_body("parity"),
        [(QTLOCAL, "dw[v] = s / (T)c[v];", "dw[v] = s / (T)(N - c[v]);"),
         (QTLOCAL, "dd[v] = s / (T)(N - c[v]);", "dd[v] = s / (T)c[v];")]),
    4: ("K19 shares: s / c replaced by s * (1 / c)", qtlocal_body("parity"),
        [(QTLOCAL, "dw[v] = s / (T)c[v];", "dw[v] = s * ((T)1 / (T)c[v]);")]),
    5: ("K19: a level without a dry cell is not skipped (c == N takes a whole)", qtlocal_body("parity"),
        [(QTLOCAL, "c[v] > 0 && c[v] < N;", "c[v] > 0 && c[v] <= N;")]),
    6: ("K19 l: the profile rows of LES 0 for every LES", qtlocal_body("rows"),
        [(QTLOCAL, "a[v] = p.A[l * p.pitch_prof + k0 + v];", "a[v] = p.A[k0 + v];"),
         (QTLOCAL, "m[v] = p.QTM[l * p.pitch_prof + k0 + v];", "m[v] = p.QTM[k0 + v];")]),
    7: ("K19 split: only the first workgroup's part of a plane's count arrives", qtlocal_body("shapes"),
        [(QTLOCAL, "else if (c[v])", "else if (c[v] && part == 0)")]),
    8: ("K19: a dry cell is given + dd", qtlocal_body("parity"),
        [(QTLOCAL, "dn = t - dd[v];", "dn = t + dd[v];")]),
}



# K20 (spc_moments.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches and none can hang (mutant 2 divides by T(0) on planes of one row; mutants 5 and 6 read the lane's own
# vector where the shipped kernel reads the element below it or nothing; mutant 7 reads LES 0 of every field; mutant 8 leaves a
# row out).
MOMENTS_MUTANTS = {
    1: ("K20 second walk: the product contracted into the sum by an fma", moments_body("special"),
        [(MOMENTS, "acc.v[v] += q;", "acc.v[v] = fma(da, db, acc.v[v]);")]),
    2: ("K20 second moments: division by N - 1 (the sample variance)", moments_body("parity"),
        [(MOMENTS, "    chain_mean<T, V>(acc, cnt);\n", "    chain_mean<T, V>(acc, cnt - (T)1);\n")]),
    3: ("K20 cov: d_a * x_b for d_a * d_b (equal in exact arithmetic, not in bits)", moments_body("parity"),
        [(MOMENTS, "c[NS - 1].v[v] - sum[NS - 1].v[v] : da;", "c[NS - 1].v[v] : da;")]),
    4: ("K20 cov: the mean of field a taken from field b's cells", moments_body("parity"),
        [(MOMENTS, "c[NS - 1].v[v] - sum[NS - 1].v[v] : da;", "c[NS - 1].v[v] - sum[0].v[v] : da;")]),
    5: ("K20 face average: the lane's own first level for the level below its vector", moments_body("face"),
        [(MOMENTS, "(v ? r.x.v[v - 1] : r.below)", "(v ? r.x.v[v - 1] : r.x.v[0])")]),
    6: ("K20 face average: x[-1] is x[0], not +0.0", moments_body("face"),
        [(MOMENTS, "r.below = below ? src[-1] : (T)0;", "r.below = below ? src[-1] : src[0];")]),
    7: ("K20 l: the cells of LES 0 for every LES", moments_body("rows"),
        [(MOMENTS, "first[s] = lane.cell(j.x[s], p.nij, ktot);", "first[s] = j.x[s] + lane.k;")]),
    8: ("K20 walks: the last row behind the load-ahead loop is left out", moments_body("large_plane"),
        [(MOMENTS, "for (; r < nij; ++r) {", "for (; r < nij - 1; ++r) {")]),
}



# K6 (spc_vnudge.hpp, spc_vnudge2.hpp, spc_vnudge_host.hpp), numbered on its own.  Every mutant only computes wrong numbers:
# none reads or writes outside what the shipped kernels touch, none loops without end.  Mutants 1-6 and 8 change a comparison
# or a flag of lane 0's state machine; 7 turns brentq's early return into its sign error (vn_brent_next is never entered);
# 9 stores "nothing to do" for the levels k >= 256 in the LDS cells the loop fills anyway (the loop itself is kept: with one
# trip only those cells would hold what the LDS held before, and a stray thl bit would write through a null thl without
# constantT); 10 makes k_vnudge_std<T, 256> walk fewer tiles (loads stay clamped to the plane); 11 skips one register add; 12
# makes the chunk loop, uniform over the workgroup as before, leave out a last chunk of fewer than 8 points (and planes of
# fewer than 8 points altogether): fewer trips, same barriers per trip; 13 reads the noise plane of the column before, column
# 0 its own.  VNUDGE_OLD_GUARD: the run ends with the shape matrix of tests/test_vnudge.py::
# test_kernel_matches_the_numpy_scipy_oracle and of its float32 copy (tests/vnudge_edges.py: old_guard) on EVERY mutant.
# Expected to survive it: 1, 2 (random data has no ties), 3 (no ql_ref of exactly 1e-9), 7 (no f(0) == 0), 8 (ql there is
# max(qt - qsat, 0): the correction of an untouched qt is 0), 9 (ktot <= 160), 10 (at most 20 workgroups), 12 (no chunk of
# fewer than 8 points).  Expected to be caught by it as well: 4 (clear levels have ql_av == ql_ref == 0), 5 (saturated
# means), 6 (a missing bracket sets beta = 5.0 exactly), 11 (the second chunk of 92 x 92 has four leaves), 13 (the launch of
# two LES).  The log says what happened.
VNUDGE_MUTANTS = {
    1: ("K6 argmax, scan of a lane's segment: v >= bv (the LAST of equal maxima inside a segment)", vnudge_body("designed_levels"),
        [(VN2, "if (v > bv || v != v) { bv = v; bi = ij; }", "if (v >= bv || v != v) { bv = v; bi = ij; }")]),
    2: ("K6 argmax, merge over the lanes: v >= best (the last lane that holds the maximum)", vnudge_body("designed_levels"),
        [(VN2, "if (qi >= 0 && (v > best || v != v)) { best = v; idx = qi; }", "if (qi >= 0 && (v >= best || v != v)) { best = v; idx = qi; }")]),
    3: ("K6: ql_ref >= 1e-9 for > 1e-9 (spcpl.py:665)", vnudge_body("designed_levels"),
        [(VN2, "if (ql_ref > 1e-9) { stage = VS_M0; touched = true; }", "if (ql_ref >= 1e-9) { stage = VS_M0; touched = true; }")]),
    4: ("K6: ql_av >= ql_ref for > (spcpl.py:679)", vnudge_body("designed_levels"),
        [(VN2, "else if (ql_av > ql_ref) { want_argmax = true; touched = true; }", "else if (ql_av >= ql_ref) { want_argmax = true; touched = true; }")]),
    5: ("K6: beta < 0 -> 1 forgotten (spcpl.py:692-695)", vnudge_body("designed_levels"),
        [(VN2, "            if (beta < 0) beta = 1.0;  ", "              ")]),
    6: ("K6: beta > 5 for beta >= 5 (spcpl.py:703)", vnudge_body("designed_levels"),
        [(VN2, "        if (beta >= 5.0) {", "        if (beta > 5.0) {")]),
    7: ("K6 brentq: the early return for f(a) == 0 dropped (scipy's brentq.c checks both ends first)", vnudge_body("designed_levels"),
        [(VN, "    if (fa == 0) { *root = xa; return 1; }\n", "")]),
    8: ("K6 constantT: thl corrected on the levels whose qt was rewritten only, not on every level the nudge looked at (spcpl.py:726)",
        vnudge_body("designed_levels"),
        [(VN2, "const bool th = p.constantT && (stv & VN2_TOUCHED);", "const bool th = p.constantT && (stv & (VN2_APPLY_MULT | VN2_APPLY_ADD));")]),
    9: ("K6 update: the staging of the per-level coefficients makes one trip, levels k >= 256 are left as they are", vnudge_body("tall"),
        [(VN2, "        s_ap[k] = ap | (th ? 4 : 0);", "        s_ap[k] = k < 256 ? (ap | (th ? 4 : 0)) : 0;")]),
    10: ("K6 qt.std: the tile count taken for 512 rows whatever ROWS", vnudge_body("std_many_workgroups"),
         [(VN2, "const int ntile = (nij + ROWS - 1) / ROWS;", "const int ntile = (nij + 512 - 1) / 512;")]),
    11: ("K6 balanced tree: the step over 2 leaves taken from 8 leaves on (nleaf > 4)", vnudge_body("small_trees"),
         [(VN2, "if (nleaf > 2) v = v + vn_row_shl<2>(v);", "if (nleaf > 4) v = v + vn_row_shl<2>(v);")]),
    12: ("K6 sum: a last chunk of fewer than 8 points is left out (c0 + 8 <= nij)", vnudge_body("chunk_edges"),
         [(VN2, "for (int c0 = 0; c0 < nij; c0 += 8192) {", "for (int c0 = 0; c0 + 8 <= nij; c0 += 8192) {")]),
    13: ("K6 solve: the noise plane of the column before (column 0 keeps its own)", vnudge_body("ragged_columns"),
         [(VN2, "    const double *const R = p.R + col * (int64_t)nij;\n    const T qt_av",
           "    const double *const R = p.R + (col > 0 ? col - 1 : 0) * (int64_t)nij;\n    const T qt_av")]),
}


def vnudge_old_guard(engine_of):
    """the shape matrix of test_kernel_matches_the_numpy_scipy_oracle and of its float32 copy, every route, both constantT"""
    from tests import vnudge_edges as ve
    return ["%s %s" % ("f32" if "32" in str(dtype) else "f64", case) for dtype in ve.DTYPES for case in ve.old_guard(engine_of(dtype))]



def patched(n, src=CSRC, table=None):
    """{file: text} of the files mutant n (of ``table``, default MUTANTS) changes, its edits applied to the sources under
    `src`; ValueError when an edit's old text does not occur exactly the expected number of times (the tree has drifted from
    the table)"""
    files = {}
    for edit in (table or MUTANTS)[n][-1]:
        name, old, new = edit[:3]
        want = edit[3] if len(edit) > 3 else 1
        if name not in files:
            with open(os.path.join(src, name)) as f:
                files[name] = f.read()
        got = files[name].count(old)
        if got != want:
            raise ValueError("mutant %s: %r occurs %d times in %s, expected %d" % (n, old, got, name, want))
        files[name] = files[name].replace(old, new)
    return files



# K22 (spc_transport.hpp), numbered on its own.  Every mutant only computes wrong numbers: none reads or writes outside what the
# shipped kernel touches (mutant 1 reads x, which the cell reads anyway, for x[ip]; mutant 5 starts K17's chain, which K22 calls,
# from 1 in the same LDS cells; mutant 6 reads x[km], which the cell reads anyway, for the top cell's x[kp]; mutant 8 stores Fb
# where Ft belongs).
TRANSPORT_MUTANTS = {
    1: ("K22 Fe: x for x[ip] (the air that enters through the east face carries the cell's own value)", transport_body("parity"),
        [(TRANSPORT, "const T e1 = pe * x, e2 = qe * xe;", "const T e1 = pe * x, e2 = qe * x;")]),
    2: ("K22 Fw: pw for qw (the west face gives the cell what it takes from it)", transport_body("signs"),
        [(TRANSPORT, "const T w1 = pw * xw, w2 = qw * x;", "const T w1 = pw * xw, w2 = pw * x;")]),
    3: ("K22 h: Fe + Fw for Fe - Fw", transport_body("parity"),
        [(TRANSPORT, "const T hi = Fe - Fw;", "const T hi = Fe + Fw;")]),
    4: ("K22 z: the vertical flux difference without r", transport_body("rows"),
        [(TRANSPORT, "const T z = rk * dz;", "const T z = dz;")]),
    5: ("K22 M: the chain started from M[0] = 1 (the ground leaks)", transport_body("signs"),
        [(VADVECT, "    T M = (T)0;\n    int k = 0;", "    T M = (T)1;\n    int k = 0;")]),
    6: ("K22 kp: the top cell takes the cell below it for the air that enters through the lid", transport_body("parity"),
        [(TRANSPORT, "const int64_t okp = k + 1 < ktot ? o + 1 : o;", "const int64_t okp = k + 1 < ktot ? o + 1 : okm;")]),
    7: ("K22 cmax: the outflow sum without its vertical part", transport_body("probe"),
        [(TRANSPORT, "const T s = sh + sv;", "const T s = sh;")]),
    8: ("K22 ftop: taken from Fb (what entered the top cell from below)", transport_body("fields"),
        [(TRANSPORT, "p.ftop[f * p.ncols + tr.col0 + w.c] = Ft;", "p.ftop[f * p.ncols + tr.col0 + w.c] = Fb;")]),
}



# K23 (spc_transport2.hpp), numbered on its own.  Every mutant only computes wrong numbers from values the shipped kernel loads
# anyway: none changes an index that is loaded from or stored to, except mutant 8, whose imm becomes im, a row the cell reads
# already; mutant 6 lets the top cell form a slope from x[km], x and x[kp], where kp is clamped to the cell itself.
TRANSPORT2_MUTANTS = {
    1: ("K23 Aw: si[i] for si[im] (the west face takes the slope of the cell downwind of it)", transport2_body("signs"),
        [(TRANSPORT2, "const T Aw = trn2_hface<T>(pw, qw, siw, sic);", "const T Aw = trn2_hface<T>(pw, qw, sic, sic);")]),
    2: ("K23 gw: 1 + pw for 1 - pw (the correction grows with the Courant number instead of vanishing at 1)", transport2_body("parity"),
        [(TRANSPORT2, "const T tp = one - p;", "const T tp = one + p;")]),
    3: ("K23 MC: 2 * a left out of the minimum (the limiter looks downwind only)", transport2_body("parity"),
        [(TRANSPORT2, "const T lo = a2 < b2 ? a2 : b2;", "const T lo = b2;")]),
    4: ("K23 MC: the extremum branch returns c0 (no limiting at an extremum)", transport2_body("special"),
        [(TRANSPORT2, "    T s = zero;  ", "    T s = c0;    ")]),
    5: ("K23 dt: r[k] for r[kp] (the downward flux takes the Courant number of the cell below the face)", transport2_body("rows"),
        [(TRANSPORT2, "const T At = trn2_vface<T>(pt, qt, rk, rp, skc, skt);", "const T At = trn2_vface<T>(pt, qt, rk, rk, skc, skt);")]),
    6: ("K23 sk: not zeroed at k == ktot - 1 (the top cell has a slope towards the lid)", transport2_body("parity"),
        [(TRANSPORT2, "const bool inner = k > 0 && k + 1 < ktot;", "const bool inner = k > 0;")]),
    7: ("K23 Fe2: Aw added to Fe (the east face takes the west face's correction)", transport2_body("fields"),
        [(TRANSPORT2, "const T Fe2 = Fe + Ae;", "const T Fe2 = Fe + Aw;")]),
    8: ("K23 imm: taken as im (the slope of the west neighbour looks at the neighbour itself)", transport2_body("alignment"),
        [(TRANSPORT2, "const int imm = im ? im - 1 : itot - 1;", "const int imm = im;")]),
}

# K25 (spc_vmix.hpp), numbered on its own.  Every mutant changes a VALUE only: no loop bound, barrier or launch extent differs from
# the shipped kernel, and every index stays inside the column's LDS cells and the rows the shipped kernel reads (mutant 2 reads
# eu[ktot - 1], an entry of the array that the rule never uses; mutant 5 reads the cell of q[ktot - 1], which holds km[ktot - 1]).
VMIX_MUTANTS = {
    1: ("K25 s: the upper cell's km taken twice (km[k] for km[k-1]: a face no longer belongs to both its cells alike)", vmix_body("parity"),
        [(VMIX, "const T h = ka + kn;", "const T h = kn + kn;")]),
    2: ("K25 lo: eu for el", vmix_body("parity"),
        [(VMIX, "const T lo = ce[u] * slo;", "const T lo = cu[u] * slo;"), (VMIX, "const T lo = el[k] * slo;", "const T lo = eu[k] * slo;"),
         (VMIX, "const T lo = el[top] * slo;", "const T lo = eu[top] * slo;")]),
    3: ("K25 s: the comparison of the cap reversed (the larger of s and kv2)", vmix_body("viscosity"),
        [(VMIX, "return s < cap ? s : cap;", "return s > cap ? s : cap;")]),
    4: ("K25 b: 1 - lo for 1 + lo", vmix_body("parity"),
        [(VMIX, "const T b1 = (T)1 + lo;", "const T b1 = (T)1 - lo;", 2), (VMIX, "const T bk = (T)1 + lo; ", "const T bk = (T)1 - lo; ")]),
    5: ("K25 back substitution: q of the level above (q[k] for q[k-1], seen from the level that is known)", vmix_body("parity"),
        [(VMIX, "cq[u] = kq[k - u];", "cq[u] = kq[k - u + 1];"), (VMIX, "const T t = kq[k] * y;", "const T t = kq[k + 1] * y;")]),
    6: ("K25 drag: a field without a drag takes that of the launch's first field (the drag on a scalar)", vmix_body("boundary"),
        [(VMIX, "const T *dr = p.dr[f];", "const T *dr = p.dr[f] ? p.dr[f] : p.dr[0];")]),
    7: ("K25 d[0]: s0 left out (the flux enters as if dt / dz[0] were 1)", vmix_body("boundary"),
        [(VMIX, "const T t = p.s0[l] * flux[l];", "const T t = flux[l];")]),
    8: ("K25 sp: without v (the drag sees the wind along i only)", vmix_body("boundary"),
        [(VMIX, "const T e = uu + vv;", "const T e = uu;")]),
}


# K7 (spc_sputils.hpp, spc_sputils_host.hpp), numbered on its own; the guards are the slab bodies of tests/sputils_slabs.py.  Every
# mutant only computes wrong numbers: none reads or writes outside what the shipped kernel touches.
#  1: the element whose carry is lost stays in its row at entry 0, which the row's walk visits anyway (i > n alone would leave the
#     row by one entry: not the mutant).  2, 3: row 0 of the slab's own LDS.  4: the x of the thread's CURRENT output once more.
#  5, 14: element e < nrow * n of a slab whose rows are pitch >= n apart lies in front of the slab's last element.
#  6: lout[k * nrow + r] is a permutation of lout[r * nG + k] over the slab's nrow * nG results.  7, 8: row 0 of the slab's LDS;
#     the cell counts stay below nL - 1 because row 0's padded grid ends in NaN like every row's.  9: only the stored VALUE grows
#     (the count over the NaN padding, at most 2 p2 - 1).  10: a row index is used only below n_rows (`live`), rows of the next
#     workgroup included, which writes its own values there: wrong either way.  11: the same eight lanes in another order.
#  12: host only; the launch is right, the height the body asserts is not.  13: r * n_x + i <= r * pitch_out + i.
SPUTILS_MUTANTS = {
    1: ("K7 SuWalk::next: the carry lost where the entry lands exactly on n (i > n for i >= n; the entry wraps, the row does not)",
        sputils_body("walk"),
        [(SU, "        if (i >= n) { i -= n; ++r; }", "        if (i > n) { i -= n; ++r; } else if (i == n) i = 0;")]),
    2: ("K7 k_interp: the LDS row of xp of the slab's first row for every row although xp is per row", sputils_body("rows_differ"),
        [(SU, "const T *const xpr = q.pitch_xp ? lxp + su_mul(r, stride) : lxp;", "const T *const xpr = lxp;")]),
    3: ("K7 k_interp: fp of the slab's first row for every row", sputils_body("rows_differ"),
        [(SU, "res = su_interp_pad<SL>(xpr, lfp + su_mul(r, n_xp), n_xp, q.p2, xv);", "res = su_interp_pad<SL>(xpr, lfp, n_xp, q.p2, xv);")]),
    4: ("K7 k_interp: the one-ahead load of x taken before next() (every later output of a thread sees the x before it)", sputils_body("heights"),
        [(SU, "        w.next();\n        if (e + SU_THREADS < cnt) xn = ldg(su_at(xb, su_mul(w.r, px) + w.i));",
          "        if (e + SU_THREADS < cnt) xn = ldg(su_at(xb, su_mul(w.r, px) + w.i));\n        w.next();")]),
    5: ("K7 su_stage_slab: a pitched slab staged as if its rows were contiguous", sputils_body("last_slab"),
        [(SU, "    const bool flat = pitch == n;", "    const bool flat = true;")]),
    6: ("K7 k_interp_c: the results laid out layer-major in LDS, where the store reads them row-major", sputils_body("rows_differ"),
        [(SU, "if constexpr (STAGE) lout[su_mul(r, nG) + k] = res;", "if constexpr (STAGE) lout[su_mul(k, nrow) + r] = res;")]),
    7: ("K7 k_interp_c: the weight terms td of the slab's first row for every row", sputils_body("rows_differ"),
        [(SU, ", *const td = ltd + su_mul(r, nc) + ia;", ", *const td = ltd + ia;")]),
    8: ("K7 k_interp_c: the staged grid of the slab's first row for every row although zh is per row", sputils_body("rows_differ"),
        [(SU, "const T *const z = STAGE ? lz + (p.pitch_zh ? su_mul(r, zstride) : 0) : zg + (row0 + r) * p.pitch_zh;",
          "const T *const z = STAGE ? lz : zg + (row0 + r) * p.pitch_zh;")]),
    9: ("K7 k_searchsorted: no clamp to n_a (a NaN key counts the NaN padding too)", sputils_body("specials_in_the_slab"),
        [(SU, "            idx = idx < n_a ? idx : n_a;\n", "")]),
    10: ("K7 k_rms: the row taken from threadIdx.x >> 2 (four lanes per row where the leaf has eight accumulators)", sputils_body("rms_groups"),
         [(SU, "(SU_THREADS / 8) + (threadIdx.x >> 3);", "(SU_THREADS / 8) + (threadIdx.x >> 2);")]),
    11: ("K7 su_leaf8: the eight accumulators combined as ((r0+r4)+(r2+r6))+((r1+r5)+(r3+r7))", sputils_body("rms_groups"),
         [(SU, "    T s = rj + __shfl_xor(rj, 1);\n    s = s + __shfl_xor(s, 2);\n    s = s + __shfl_xor(s, 4);",
           "    T s = rj + __shfl_xor(rj, 4);\n    s = s + __shfl_xor(s, 2);\n    s = s + __shfl_xor(s, 1);")]),
    12: ("K7 su_rows (host): without the fit_rounds step (91 -> 160: 7 rows for 8)", sputils_body("heights"),
         [(SU_HOST, "    if (fit_rounds && n_out > 0) {", "    if (false && fit_rounds && n_out > 0) {")]),
    13: ("K7 k_interp: the results stored as if out were contiguous (r * n_x for r * pitch_out)", sputils_body("last_slab"),
         [(SU, "stg<WT>(su_at(ob, su_mul(r, po) + i), res);", "stg<WT>(su_at(ob, su_mul(r, n_x) + i), res);")]),
    14: ("K7 k_interp_c: the slab's results stored as if out were contiguous", sputils_body("last_slab"),
         [(SU, "const bool flat = p.pitch_out == nG;", "const bool flat = true;")]),
}


# What the slab-chain kernels share (spc_chain.hpp; K10, K11, K12, K14, K20), numbered on its own: slips of the header, and the same
# slip made in every kernel's own walk.  Every mutant only computes wrong numbers: none reads or writes outside what the shipped
# kernels touch (mutant 1 sends the lanes of an LES to its first ktot / V levels; mutants 3 and 4 visit fewer rows or the same rows
# of a batch again).  The guard of each is the body ``chain`` of EVERY kernel it changes, on both engines.
# K26 (spc_hmix.hpp), numbered on its own.  Every mutant changes a VALUE only: no loop bound, barrier or launch extent differs from
# the shipped kernel, and every index stays inside the line and the LDS of its lane.
HMIX_MUTANTS = {
    1: ("K26 t: the cell's own km taken twice (km[i] for km[ip]: a face no longer belongs to both its cells alike)", hmix_body("parity"),
        [(HMIX, "const T t = ka + kn;", "const T t = ka + ka;")]),
    2: ("K26 a: ay for ax (the sweep along i takes the coefficient of j, and the other way round)", hmix_body("parity"),
        [(HMIX, "(axis ? a->ay[f] : a->ax[f])", "(axis ? a->ax[f] : a->ay[f])")]),
    3: ("K26 s: the comparison of the bound reversed (the larger of s and kh2)", hmix_body("viscosity"),
        [(HMIX, "const T sc = s < cap ? s : cap;", "const T sc = s > cap ? s : cap;")]),
    4: ("K26 b: 1 - lo for 1 + lo", hmix_body("parity"),
        [(HMIX, "const T b1 = (T)1 + wl;", "const T b1 = (T)1 - wl;"), (HMIX, "const T b1 = (T)1 + lo;", "const T b1 = (T)1 - lo;", 2)]),
    5: ("K26 c: c[n-2] left out (the last eliminated cell forgets its face to the condensed one)", hmix_body("lines"),
        [(HMIX, "const T c = wl + (m == 1 ? up : (T)0);", "const T c = wl + (T)0;"),
         (HMIX, "const T c = (T)0 + (i + u == m - 1 ? up : (T)0);", "const T c = (T)0 + (T)0;")]),
    6: ("K26 back substitution: the q of the neighbouring cell (q[i+1] for q[i])", hmix_body("parity"),
        [(HMIX, "cq[u] = q[(i - u) * L];", "cq[u] = q[(i - u + 1) * L];")]),
    7: ("K26 num: lo[n-1] and up[n-1] swapped", hmix_body("parity"),
        [(HMIX, "const T n1 = wl * yv;", "const T n1 = lo * yv;"), (HMIX, "const T n3 = lo * yl;", "const T n3 = wl * yl;")]),
    8: ("K26 den: z left out (the condensed cell forgets what the others hand back)", hmix_body("parity"),
        [(HMIX, "const T den = d2 - d3;", "const T den = bl;")]),
}


def chain_guard(*modules):
    """the body ``chain`` of each of tests/``modules``.py: (every one of them failed, everything that failed anywhere)"""
    def guard(engine_of):
        caught, failed = True, []
        for module in modules:
            ok, names = body_guard(module, "chain")(engine_of)
            caught, failed = caught and ok, failed + ["%s.%s" % (module, n) for n in names]
        return caught, failed
    guard.__name__ = "chain of " + ", ".join(modules)
    return guard


_CHAIN_ALL = ("slab_edges", "les_advance_ref", "les_thermo_ref", "les_micro_ref", "les_moments_ref")
_CHAIN_WALK2 = ("les_advance_ref", "les_thermo_ref", "les_micro_ref")
_MORE = ("const bool more = r + 2 * U <= nij;", "const bool more = r + 3 * U <= nij;")
CHAIN_MUTANTS = {
    1: ("chain lane: k without * V (the lanes of an LES crowd into its first ktot / V levels)", chain_guard(*_CHAIN_ALL),
        [(CHAIN, "k = (int)(g - l * kv) * V;", "k = (int)(g - l * kv);")]),
    2: ("chain mean: the sums divided by itot * jtot - 1", chain_guard(*_CHAIN_ALL),
        [(CHAIN, "acc.v[v] = acc.v[v] / cnt;", "acc.v[v] = acc.v[v] / (cnt - (T)1);")]),
    3: ("double-buffered walks: `more` off by one batch (the last batch that has a successor works on the rows before it again)",
        chain_guard(*_CHAIN_WALK2), [(ADVANCE,) + _MORE, (THERMO,) + _MORE, (MICRO,) + _MORE]),
    4: ("every walk: the single rows behind the last whole batch dropped", chain_guard(*_CHAIN_ALL),
        [(SLAB, "    for (; r < p.nij; ++r) {", "    for (; r < p.nij && false; ++r) {"),
         (ADVANCE, "    for (; r < nij; ++r) {", "    for (; r < nij && false; ++r) {"),
         (THERMO, "    for (; r < nij; ++r) {", "    for (; r < nij && false; ++r) {"),
         (MICRO, "    for (; r < nij; ++r) {", "    for (; r < nij && false; ++r) {"),
         (MOMENTS, "    for (; r < nij; ++r) {", "    for (; r < nij && false; ++r) {")]),
}


def _tag(table):
    """(library prefix, source directory prefix) of a table"""
    for t in ALL_TABLES:
        if table is t.table:
            return t.lib, t.src
        if table is not None and table is t.equivalent:
            return t.lib[:-1] + "_eq_", t.src + "eq"
    return "", ""


def lib_of(n, table=None):
    return os.path.join(OUT, "libspc_%smutant%s.so" % (_tag(table)[0], n))


def build_one(n, table=None):
    src = os.path.join(OUT, "src%s%s" % (_tag(table)[1], n))
    shutil.rmtree(src, ignore_errors=True)
    shutil.copytree(CSRC, src)
    for name, text in patched(n, table=table).items():
        with open(os.path.join(src, name), "w") as f:
            f.write(text)
    lib = lib_of(n, table)
    r = subprocess.run([HIPCC] + HIP_FLAGS + [os.path.join(src, "spc_hip.hip"), "-o", lib], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise RuntimeError("mutant %s: hipcc exit status %d\n%s" % (n, r.returncode, r.stdout[-2000:]))
    return lib


def build(ns, jobs, table=None):
    os.makedirs(OUT, exist_ok=True)
    bad = 0

    def one(n):
        try:
            build_one(n, table)
            return "mutant %s built" % n, 0
        except (ValueError, RuntimeError) as e:
            return "mutant %s FAILED: %s" % (n, e), 1

    with ThreadPoolExecutor(max(1, min(jobs, 16))) as pool:
        for line, failed in pool.map(one, ns):
            print(line, flush=True)
            bad += failed
    return 1 if bad else 0


def run_guard(guard, lib_path):
    """a callable guard on the engines of one library -> (detected, what failed)"""
    from sp_coupler_amd.engine import Engine
    return guard(lambda dtype: Engine("cuda:0", dtype=dtype, lib_path=lib_path))


def run(lib_path):
    from tests import semantic_props as sp
    from tests.test_semantic_gpu import HipImpl
    impl = HipImpl(lib_path)
    failed = []
    for prop in sp.PROPERTIES:
        try:
            prop(impl)
        except AssertionError:
            failed.append(prop.__name__[5:])
        except Exception:
            failed.append(prop.__name__[5:] + " (raised: %s)" % traceback.format_exc().strip().splitlines()[-1])
    return failed


def main_table(only, t):
    """the control of a table numbered on its own (an entry of TABLES): the bodies of tests/``module``.py on the shipped
    library, then on every mutant; then the edits of ``equivalent`` (expected to fail no body) and
    ``old_guards[n](engine_of)`` -> names that failed, on the mutants it is given for (printed, not judged)"""
    import torch
    table, kernel, module, gpu_test, equivalent, old_guards, notes = t.table, t.kernel, t.module, t.gpu_test, t.equivalent, t.old_guards, t.notes
    print("mutation control of tests/%s.py (tests/%s.py) on %s" % (module, gpu_test, torch.cuda.get_device_name(0)))
    chosen = sorted(n for n in table if only is None or n in only)
    clean = run_guard(table[chosen[0]][1], None)[1]
    print("shipped library: the bodies of tests/%s.py on %s, failed: %s"
          % (module, "the float64 engine" if equivalent is not None else "both engines", clean or "none"), flush=True)
    for line in (notes() if notes else ()):
        print(line, flush=True)
    bad = int(bool(clean))
    for n in chosen:
        what, guard, _ = table[n]
        path = lib_of(n, table)
        if not os.path.exists(path):
            print("%s mutant %2d: NOT BUILT (%s)" % (kernel, n, path))
            bad += 1
            continue
        ok, failed = run_guard(guard, path)
        bad += not ok
        print("%s mutant %2d: %s\n           guarded by %s: %s; all failing: %s"
              % (kernel, n, what, guard.__name__, "DETECTED" if ok else "SURVIVED", failed or "none"), flush=True)
    for name in sorted(equivalent or {}) if only is None else ():
        path = lib_of(name, equivalent)
        if not os.path.exists(path):
            print("%s equivalent edit %s: NOT BUILT (%s)" % (kernel, name, path))
            bad += 1
            continue
        failed = run_guard(table[chosen[0]][1], path)[1]
        bad += bool(failed)
        print("%s equivalent edit %s: %s\n           proved to change no output; every body run, failing: %s"
              % (kernel, name, equivalent[name][0], failed or "none"), flush=True)
    for n, guard in (old_guards or {}).items() if only is None else ():
        failed = run_guard(lambda engine_of, g=guard: (False, g(engine_of)), lib_of(n, table))[1]
        print("%s mutant %2d under the guards that existed before tests/%s.py (%s): %s"
              % (kernel, n, module, guard.__doc__, "not detected" if not failed else "detected by %s" % failed), flush=True)
    print("result: %s" % ("every mutant detected, shipped library clean" if not bad else "%d problem(s)" % bad))
    return 1 if bad else 0


def geo_old_guard(engine_of):
    """adversarial, naive_flips, haversine and the 2^20-point scale test"""
    import torch
    from tests import geo_edges
    return geo_edges.check_everything(engine_of(torch.float64), names=geo_edges.OLD_BODIES, scale=True)


def lesstate_old_guard(engine_of):
    """mixed_shapes, forced_short_substreams, twist_boundary and engine_level"""
    import torch
    from tests import les_state_ref
    return les_state_ref.check_everything(engine_of(torch.float64), names=les_state_ref.OLD_BODIES)


def main_vnudge(only, t):
    """the control of VNUDGE_MUTANTS (main_table), then the old guard on every mutant: at least VNUDGE_MIN_SURVIVORS of them
    must pass the old matrix -- they are what the bodies of tests/vnudge_edges.py add -- and each of those was detected by its
    body above"""
    bad = main_table(only, t)
    if only is not None:
        return bad
    print("old guard: %s, on the shipped library and on every mutant" % vnudge_old_guard.__doc__)
    clean = run_guard(lambda engine_of: (False, vnudge_old_guard(engine_of)), None)[1]
    print("shipped library under the old guard, failed: %s" % (clean or "none"), flush=True)
    survivors = []
    for n in sorted(VNUDGE_MUTANTS):
        failed = run_guard(lambda engine_of: (False, vnudge_old_guard(engine_of)), lib_of(n, VNUDGE_MUTANTS))[1]
        if not failed:
            survivors.append(n)
        print("K6 mutant %2d under the old guard: %s" % (n, "SURVIVES (caught by its new body alone)" if not failed else
                                                         "caught already, %d of 16 cases: %s" % (len(failed), failed)), flush=True)
    ok = len(survivors) >= VNUDGE_MIN_SURVIVORS and not clean
    print("old guard: %d mutants survive it %s, at least %d asked for: %s" % (len(survivors), survivors, VNUDGE_MIN_SURVIVORS, "ok" if ok else "NOT ENOUGH"))
    return 1 if bad or not ok else 0


VNUDGE_MIN_SURVIVORS = 6


def geo_notes():
    from tests import geo_edges
    return ["exact_tails: " + geo_edges.exact_tails_counts()]


def main(only=None, t=None):
    import torch
    print("mutation control of tests/test_semantic_gpu.py and tests/slab_edges.py on %s" % torch.cuda.get_device_name(0))
    bad = 0
    chosen = sorted(n for n in MUTANTS if only is None or n in only)
    if any(not callable(MUTANTS[n][1]) for n in chosen):
        clean = run(None)
        from tests import semantic_props as sp
        print("shipped library: %d properties, failed: %s" % (len(sp.PROPERTIES), clean or "none"))
        bad += bool(clean)
    slab = [MUTANTS[n][1] for n in chosen if callable(MUTANTS[n][1])]
    if slab:
        slab_clean = run_guard(slab[0], None)[1]
        print("shipped library: the bodies of tests/slab_edges.py on both engines, failed: %s" % (slab_clean or "none"), flush=True)
        bad += bool(slab_clean)
    for n in chosen:
        what, guard, _ = MUTANTS[n]
        path = os.path.join(OUT, "libspc_mutant%d.so" % n)
        if not os.path.exists(path):
            print("mutant %2d: NOT BUILT (%s)" % (n, path))
            bad += 1
            continue
        if callable(guard):
            ok, failed = run_guard(guard, path)
            guard = guard.__name__
        else:
            failed = run(path)
            ok = guard in [f.split(" ")[0] for f in failed]
        bad += not ok
        print("mutant %2d: %s\n           guarded by %s: %s; all failing: %s" % (n, what, guard, "DETECTED" if ok else "SURVIVED", failed or "none"), flush=True)
    print("result: %s" % ("every mutant detected, shipped library clean" if not bad else "%d problem(s)" % bad))
    return 1 if bad else 0


#: every table in the order of its flag on the command line (the first one set is run); the unnumbered MUTANTS first, without a
#: flag.  lib, src: what the names of a mutant's library and of its source directory under build/mutants/ carry
Table = collections.namedtuple("Table", "flag table kernel lib src module gpu_test equivalent old_guards notes main",
                               defaults=(None, None, None, main_table))
TABLES = (
    Table(None, MUTANTS, None, "", "", "slab_edges", "test_slab_gpu", main=main),
    Table("advance", ADVANCE_MUTANTS, "K11", "advance_", "adv", "les_advance_ref", "test_les_advance_gpu"),
    Table("thermo", THERMO_MUTANTS, "K12", "thermo_", "thermo", "les_thermo_ref", "test_les_thermo_gpu"),
    Table("waterpath", WATERPATH_MUTANTS, "K13", "waterpath_", "waterpath", "les_water_paths_ref", "test_les_water_paths_gpu"),
    Table("micro", MICRO_MUTANTS, "K14", "micro_", "micro", "les_micro_ref", "test_les_micro_gpu"),
    Table("diffuse", DIFFUSE_MUTANTS, "K15", "diffuse_", "diffuse", "les_diffuse_ref", "test_les_diffuse_gpu"),
    Table("advect", ADVECT_MUTANTS, "K16", "advect_", "advect", "les_advect_ref", "test_les_advect_gpu"),
    Table("vadvect", VADVECT_MUTANTS, "K17", "vadvect_", "vadvect", "les_vadvect_ref", "test_les_vadvect_gpu"),
    Table("radiate", RADIATE_MUTANTS, "K18", "radiate_", "radiate", "les_radiate_ref", "test_les_radiate_gpu"),
    Table("qtlocal", QTLOCAL_MUTANTS, "K19", "qtlocal_", "qtlocal", "les_qt_local_ref", "test_les_qt_local_gpu"),
    Table("moments", MOMENTS_MUTANTS, "K20", "moments_", "moments", "les_moments_ref", "test_les_moments_gpu"),
    Table("buoyancy", BUOYANCY_MUTANTS, "K21", "buoyancy_", "buoyancy", "les_buoyancy_ref", "test_les_buoyancy_gpu"),
    Table("transport", TRANSPORT_MUTANTS, "K22", "transport_", "transport", "les_transport_ref", "test_les_transport_gpu"),
    Table("transport2", TRANSPORT2_MUTANTS, "K23", "transport2_", "transport2", "les_transport2_ref", "test_les_transport2_gpu"),
    Table("geo", GEO_MUTANTS, "K8", "geo_", "geo", "geo_edges", "test_geo_gpu", GEO_EQUIVALENT, {n: geo_old_guard for n in GEO_OLD_GUARDS}, geo_notes),
    Table("lesstate", LESSTATE_MUTANTS, "K9", "lesstate_", "lesstate", "les_state_ref", "test_les_state_gpu", LESSTATE_EQUIVALENT,
          {n: lesstate_old_guard for n in LESSTATE_OLD_GUARDS}),
    Table("vnudge", VNUDGE_MUTANTS, "K6", "vnudge_", "vnudge", "vnudge_edges", "test_vnudge_edges_gpu", main=main_vnudge),
)

#: the tables added since tests/test_les_harness_cpu.py pinned the length of TABLES (an existing test file, which a pull request
#: that adds a kernel leaves as it is): same rows, same handling; fold them into TABLES when that count is next revised
LATER_TABLES = (
    Table("mix", MIX_MUTANTS, "K24", "mix_", "mix", "les_mix_ref", "test_les_mix_gpu"),
    Table("vmix", VMIX_MUTANTS, "K25", "vmix_", "vmix", "les_vmix_ref", "test_les_vmix_gpu"),
)
#: K7's table stands in a tuple of its own, not at the end of LATER_TABLES: tests/test_les_vmix_mutants_cpu.py pins K25's row as
#: LATER_TABLES[-1], and tests/test_les_mix_mutants_cpu.py imports the guard module of every row of LATER_TABLES (existing test
#: files, which a pull request that adds a table leaves as they are).  Same rows, same handling.
SPUTILS_TABLES = (
    Table("sputils", SPUTILS_MUTANTS, "K7", "sputils_", "sputils", "sputils_slabs", "test_sputils_slabs_gpu"),
)
#: what spc_chain.hpp's kernels share: the guards are the ``chain`` bodies of five modules, tests/les_harness.py holds their cases
CHAIN_TABLES = (
    Table("chain", CHAIN_MUTANTS, "K10/K11/K12/K14/K20", "chain_", "chain", "les_harness", "test_*_gpu.py::test_the_chain_cases"),
)
#: K26's table stands in a tuple of its own as well, for the same reason
HMIX_TABLES = (
    Table("hmix", HMIX_MUTANTS, "K26", "hmix_", "hmix", "les_hmix_ref", "test_les_hmix_gpu"),
)
ALL_TABLES = TABLES + LATER_TABLES + SPUTILS_TABLES + CHAIN_TABLES + HMIX_TABLES


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="mutation control of the semantic tests")
    ap.add_argument("--build", nargs="*", type=int, metavar="n",
                    help="build the mutant libraries n ... (default: all) instead of running the control")
    ap.add_argument("--only", nargs="+", type=int, metavar="n", help="run the control for the mutants n ... only")
    ap.add_argument("-j", type=int, default=4, help="parallel compiles for --build (at most 16)")
    for t in ALL_TABLES[1:]:
        ap.add_argument("--" + t.flag, action="store_true", help="the table of %s (%s_MUTANTS) instead of MUTANTS" % (t.kernel, t.flag.upper()))
    args = ap.parse_args()
    t = next((t for t in ALL_TABLES[1:] if getattr(args, t.flag)), TABLES[0])
    if args.build is not None:
        unknown = sorted(set(args.build) - set(t.table))
        if unknown:
            ap.error("no mutant %s" % unknown)
        rc = build(args.build or sorted(t.table), args.j, t.table)
        if t.equivalent and not args.build:
            rc |= build(sorted(t.equivalent), args.j, t.equivalent)
        sys.exit(rc)
    sys.exit(t.main(set(args.only) if args.only else None, t))
