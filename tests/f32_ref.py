"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the reference coupling lines in a chosen floating type (not collected).

The float32 twin of oracle/spcpl_oracle.py, and the second restatement next to the C oracle's oracle_*_f32 entries
(oracle/spc_oracle.c states the contract both follow).  Every function computes in the dtype of its inputs, so that

* with float32 inputs it is the reference's lines evaluated by NumPy 2 on float32 arrays: constants are Python floats, i.e.
  NEP 50 weak scalars rounded to float32 once (``rv / rd - 1`` included); sums are NumPy's pairwise tree with float32 adds
  (``npsum32_restated``); the power is spc_powf (``tests/oracle_c.powf``, pinned by tests/test_pow_accuracy.py).  Two
  documented exceptions stay in float32 where NumPy would go through float64: ``numpy.interp`` (restated here as
  ``interp``, arr_interp with every operation in float32) and the ``numpy.zeros`` buffers of ``interp_c`` / ``interp_rho``;
* with float64 inputs it reproduces oracle/spcpl_oracle.py bit for bit (tests/test_f32_oracle_cpu.py), which proves it
  restates the same lines in the same order.

Citations are ``file:line`` relative to the reference root.
"""
import numpy

from tests import oracle_c
from tests.vnudge_f32_ref import npsum32_restated

F32, F64 = numpy.float32, numpy.float64
# splib/sputils.py:14-20 -- Python floats: weak scalars, rounded to the array's type where they meet it
pref0, rd, rv, cp, rlv, grav = 1e5, 287.04, 461.5, 1004., 2.53e6, 9.81
gcm_vars = ["U", "V", "T", "SH", "QL", "QI", "Pfull", "Phalf", "A", "Zgfull", "Zghalf"]


def power(x, y):
    """x ** y: spc_powf on float32 (the exponent a weak scalar rounded to float32), NumPy's ** on float64"""
    x = numpy.asarray(x)
    if x.dtype == F32:
        return oracle_c.powf(x, F32(y)).reshape(x.shape)[()]
    return x ** y


def rsum(a):
    """ndarray.sum() of a contiguous array: the pairwise tree, in float32 adds for float32"""
    return npsum32_restated(a) if a.dtype == F32 else a.sum()


def rms(a):
    """splib/sputils.py:23-24, NumPy's own lines"""
    return numpy.sqrt(numpy.mean(a ** 2))


def exner(p):
    """splib/sputils.py:28-29"""
    return power(p / pref0, rd / cp)


def iexner(p):
    """splib/sputils.py:33-34"""
    return power(p / pref0, -rd / cp)


def interp(x, xp, fp):
    """numpy.interp (sputils.py:86) as arr_interp computes it (numpy/_core/src/multiarray/compiled_base.c), every operation
    in the type of xp: left = fp[0], right = fp[-1], the exact-hit and NaN-fallback branches.  Vectorised over x."""
    xp, fp = numpy.asarray(xp), numpy.asarray(fp)
    R = xp.dtype
    x = numpy.asarray(x, dtype=R)
    n = len(xp)
    if n == 1:
        return numpy.full(x.shape, fp[0], dtype=R)
    lo, hi = numpy.zeros(x.shape, numpy.int64), numpy.full(x.shape, n, numpy.int64)
    while (lo < hi).any():                        # upper_bound: the binary search of the C oracle, lane by lane
        act = lo < hi
        mid = lo + ((hi - lo) >> 1)
        ge = x >= xp[numpy.minimum(mid, n - 1)]
        lo = numpy.where(act & ge, mid + 1, lo)
        hi = numpy.where(act & ~ge, mid, hi)
    j = lo - 1
    jc = numpy.clip(j, 0, n - 2)
    x0, x1, f0, f1 = xp[jc], xp[jc + 1], fp[jc], fp[jc + 1]
    with numpy.errstate(all="ignore"):
        slope = (f1 - f0) / (x1 - x0)
        r = slope * (x - x0) + f0
        r2 = slope * (x - x1) + f1
        r2 = numpy.where(numpy.isnan(r2) & (f0 == f1), f0, r2)
        r = numpy.where(numpy.isnan(r), r2, r)
    r = numpy.where(x0 == x, f0, r)
    r = numpy.where(j >= n - 1, fp[n - 1], r)
    r = numpy.where(x < xp[0], fp[0], r)
    r = numpy.where(x > xp[n - 1], fp[n - 1], r)
    return numpy.where(numpy.isnan(x), x, r).astype(R)


def searchsorted(a, v, **kwargs):
    """splib/sputils.py:88-91: numpy.searchsorted compares in the arrays' own type"""
    return numpy.searchsorted(a, v, **kwargs)


def integral(a, b, z, q, w=None):
    """splib/sputils.py:94-161"""
    if a < z[0] or a > z[-1] or b < z[0] or b > z[-1]:
        return None
    sign = 1
    if a > b:
        sign = -1
        a, b = b, a
    ia = 0
    while z[ia + 1] < a:
        ia += 1
    ib = ia
    while z[ib + 1] < b:
        ib += 1
    if w is None:
        S = rsum(q[ia:ib + 1] * (z[ia + 1:ib + 2] - z[ia:ib + 1]))
        Sa = q[ia] * (a - z[ia])
        Sb = q[ib] * (z[ib + 1] - b)
        return (S - Sa - Sb) * sign
    S = rsum(w[ia:ib + 1] * q[ia:ib + 1] * (z[ia + 1:ib + 2] - z[ia:ib + 1]))
    Sa = w[ia] * q[ia] * (a - z[ia])
    Sb = w[ib] * q[ib] * (z[ib + 1] - b)
    Sw = rsum(w[ia:ib + 1] * (z[ia + 1:ib + 2] - z[ia:ib + 1]))
    Swa = w[ia] * (a - z[ia])
    Swb = w[ib] * (z[ib + 1] - b)
    return (S - Sa - Sb) / (Sw - Swa - Swb) * sign


def interp_c(Zh, zh, q, rho):
    """splib/sputils.py:173-189, the Q buffer in the inputs' type (the reference's numpy.zeros is float64: exception).
    A None from integral becomes NaN, as in the C oracle."""
    Q = numpy.zeros(len(Zh) - 1, dtype=Zh.dtype)
    for i in range(len(Q)):
        if Zh[i] < zh[-1]:
            v = integral(Zh[i + 1], Zh[i], zh, q, rho)
            Q[i] = numpy.nan if v is None else v
    return Q


def interp_rho(Zh, zh, rho):
    """splib/sputils.py:191-197, the RHO buffer in the inputs' type (exception as interp_c)"""
    RHO = numpy.zeros(len(Zh) - 1, dtype=Zh.dtype)
    for i in range(len(RHO)):
        if Zh[i] < zh[-1]:
            v = integral(Zh[i + 1], Zh[i], zh, rho)
            RHO[i] = numpy.nan if v is None else v / (Zh[i] - Zh[i + 1])
    return RHO


def convert_surface_fluxes(Ph_s, T_s, QLflux, QIflux, SHflux, TSflux):
    """splib/spcpl.py:136-167 (vectorised over columns: every operation is elementwise)"""
    rho = Ph_s / (rd * T_s)                                                  # spcpl.py:153
    wqt = - (QLflux + QIflux + SHflux) / rho                                 # spcpl.py:159
    wthl = - TSflux * iexner(Ph_s) / (cp * rho)                              # spcpl.py:161
    return wthl, wqt


def convert_profiles(col, zf):
    """splib/spcpl.py:171-246"""
    U, V, T, SH, QL, QI, Pf, Ph, A, Zgfull, Zghalf = (col[v] for v in gcm_vars)
    c = rv / rd - 1                                                          # spcpl.py:175 (a Python float)
    Tv = T * (1 + c * SH - (QL + QI))                                        # spcpl.py:176
    Zh = (Zghalf - Zghalf[-1]) / grav                                        # spcpl.py:197
    Zf = (Zgfull - Zghalf[-1]) / grav                                        # spcpl.py:198
    thl_ = (T - (rlv * (QL + QI)) / cp) * iexner(Pf)                         # spcpl.py:214
    qt_ = SH + QL + QI                                                       # spcpl.py:215
    h = zf
    thl = interp(h, Zf[::-1], thl_[::-1])                                    # spcpl.py:224
    qt = interp(h, Zf[::-1], qt_[::-1])                                      # spcpl.py:225
    ql = interp(h, Zf[::-1], QL[::-1])                                       # spcpl.py:226
    u = interp(h, Zf[::-1], U[::-1])                                         # spcpl.py:227
    v = interp(h, Zf[::-1], V[::-1])                                         # spcpl.py:228
    return dict(u=u, v=v, thl=thl, qt=qt, ps=Ph[-1], ql=ql, Zf=Zf, Zh=Zh, Tv=Tv, THL=thl_, QT=qt_)


def _grid(z, i):
    return z if z.ndim == 1 else z[i]


def forward(gcm, zf, zh, prof, factor, dt, couple_surface=True):
    """K1 in full (splib/spcpl.py:171-246, 299-385, 136-167, 764) for every column: the outputs of tests/oracle_c.forward"""
    n = gcm["T"].shape[0]
    rows = []
    with numpy.errstate(all="ignore"):
        for i in range(n):
            col = {k: gcm[k][i] for k in gcm_vars if k in gcm}
            c = convert_profiles(col, _grid(zf, i))
            r = {k: c[k] for k in ("u", "v", "thl", "qt", "ps", "Zf", "Zh")}
            r["ql_ref"] = c["ql"]                                            # spcpl.py:347
            r["f_u"] = factor * (c["u"] - prof["U"][i]) / dt                 # spcpl.py:328
            r["f_v"] = factor * (c["v"] - prof["V"][i]) / dt                 # spcpl.py:329
            r["f_thl"] = factor * (c["thl"] - prof["THL"][i]) / dt           # spcpl.py:330
            r["f_qt"] = factor * (c["qt"] - prof["QT"][i]) / dt              # spcpl.py:331
            r["f_ps"] = factor * (c["ps"] - prof["PS"][i]) / dt              # spcpl.py:332
            r["f_ql"] = factor * (c["ql"] - prof["QL"][i]) / dt              # spcpl.py:333
            if "Rain" in prof and "rain_last" in prof:
                r["rainrate"] = (prof["Rain"][i] - prof["rain_last"][i]) / dt   # spcpl.py:325
            r["idx"] = searchsorted(_grid(zh, i), c["Zh"], side="right")[:-1][::-1].astype(numpy.int32)   # spcpl.py:764
            rows.append(r)
        out = {k: numpy.stack([numpy.asarray(r[k]) for r in rows]) for k in rows[0]}
        if couple_surface:
            out["wthl"], out["wqt"] = convert_surface_fluxes(gcm["Phalf"][:, -1], gcm["T"][:, -1], gcm["QLflux"],
                                                             gcm["QIflux"], gcm["SHflux"], gcm["TSflux"])
            out["z0m"], out["z0h"] = gcm["Z0M"].copy(), gcm["Z0H"].copy()
    return out


def cloud_indices(zh, Zh):
    """K2: splib/spcpl.py:26 / 764 for every column of Zh [n x nG+1]"""
    return numpy.stack([searchsorted(_grid(zh, i), Zh[i], side="right")[:-1][::-1] for i in range(Zh.shape[0])]).astype(numpy.int32)


def backward(gcm, Zf, zf, prof, factor, dt, conservative=False, zh=None, Zh=None):
    """K3 / K4: splib/spcpl.py:388-555 (468-478 or 479-489, 498, 518-533) for every column; Zf / Zh None: from the
    geopotential (spcpl.py:197-198).  The outputs of tests/oracle_c.backward."""
    n = gcm["T"].shape[0]
    rows = []
    with numpy.errstate(all="ignore"):
        for i in range(n):
            U, V, T, SH, QL, QI = (gcm[k][i] for k in ("U", "V", "T", "SH", "QL", "QI"))
            A = gcm["A"][i]
            zs = gcm["Zghalf"][i][-1]
            Zf_ = Zf[i] if Zf is not None else (gcm["Zgfull"][i] - zs) / grav    # spcpl.py:198
            h = _grid(zf, i)
            t_d, qt_d, ql_d, ql_ice_d, u_d, v_d = (prof[k][i] for k in ("T", "QT", "QL", "QL_ice", "U", "V"))
            ql_water_d = ql_d - ql_ice_d                                     # spcpl.py:402
            A_d = prof["A"][i][::-1]                                         # spcpl.py:404
            if not conservative:
                t_d = interp(Zf_, h, t_d)                                    # spcpl.py:471
                qt_d = interp(Zf_, h, qt_d)                                  # spcpl.py:472
                ql_d = interp(Zf_, h, ql_d)                                  # spcpl.py:473
                ql_water_d = interp(Zf_, h, ql_water_d)                      # spcpl.py:474
                ql_ice_d = interp(Zf_, h, ql_ice_d)                          # spcpl.py:475
                u_d = interp(Zf_, h, u_d)                                    # spcpl.py:476
                v_d = interp(Zf_, h, v_d)                                    # spcpl.py:477
            else:
                Zh_ = Zh[i] if Zh is not None else (gcm["Zghalf"][i] - zs) / grav   # spcpl.py:197
                zh_, rho = _grid(zh, i), prof["Rhobf"][i]
                t_d = interp_c(Zh_, zh_, t_d, rho)                           # spcpl.py:482
                qt_d = interp_c(Zh_, zh_, qt_d, rho)                         # spcpl.py:483
                ql_d = interp_c(Zh_, zh_, ql_d, rho)                         # spcpl.py:484
                ql_water_d = interp_c(Zh_, zh_, ql_water_d, rho)             # spcpl.py:485
                ql_ice_d = interp_c(Zh_, zh_, ql_ice_d, rho)                 # spcpl.py:486
                u_d = interp_c(Zh_, zh_, u_d, rho)                           # spcpl.py:487
                v_d = interp_c(Zh_, zh_, v_d, rho)                           # spcpl.py:488
            start_index = int(searchsorted(-Zf_, -h[-1]))                    # spcpl.py:498
            r = dict(f_T=factor * (t_d - T) / dt,                            # spcpl.py:518
                     f_SH=factor * ((qt_d - ql_d) - SH) / dt,                # spcpl.py:519
                     f_QL=factor * (ql_water_d - QL) / dt,                   # spcpl.py:520
                     f_QI=factor * (ql_ice_d - QI) / dt,                     # spcpl.py:521
                     f_U=factor * (u_d - U) / dt,                            # spcpl.py:524
                     f_V=factor * (v_d - V) / dt,                            # spcpl.py:525
                     f_A=factor * (A_d - A) / dt)                            # spcpl.py:526
            for f in r.values():                                             # spcpl.py:527-533
                f[0:start_index] *= 0
            r["start_index"] = numpy.int32(start_index)
            rows.append(r)
    return {k: numpy.stack([numpy.asarray(r[k]) for r in rows]) for k in rows[0]}


def diagnostics(gcm, zf=None, prof=None):
    """K5, the spifs diagnostics: splib/spcpl.py:176, 197-198, 214-215 and, with zf / prof, 402, 408-409"""
    n = gcm["T"].shape[0]
    rows = []
    with numpy.errstate(all="ignore"):
        for i in range(n):
            col = {k: gcm[k][i] for k in gcm_vars if k in gcm}
            T, SH, QL, QI, Pf = (col[k] for k in ("T", "SH", "QL", "QI", "Pfull"))
            zs = col["Zghalf"][-1]
            Zf = (col["Zgfull"] - zs) / grav                                 # spcpl.py:198
            r = dict(Tv=T * (1 + (rv / rd - 1) * SH - (QL + QI)),           # spcpl.py:175-176
                     THL=(T - (rlv * (QL + QI)) / cp) * iexner(Pf),          # spcpl.py:214
                     QT=SH + QL + QI, Zf=Zf,                                 # spcpl.py:215
                     Zh=(col["Zghalf"] - zs) / grav)                         # spcpl.py:197
            if zf is not None and prof is not None:
                pf = interp(_grid(zf, i), Zf[::-1], Pf[::-1])                # spcpl.py:408
                r["pf"] = pf
                r["t"] = prof["THL"][i] * exner(pf) + rlv * prof["QL"][i] / cp   # spcpl.py:409
                r["ql_water"] = prof["QL"][i] - prof["QL_ice"][i]            # spcpl.py:402
            rows.append(r)
    return {k: numpy.stack([numpy.asarray(r[k]) for r in rows]) for k in rows[0]}
