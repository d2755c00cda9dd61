"""float32 restatement of ``spcpl.variability_nudge`` (splib/spcpl.py:613-744): the reference's own lines, evaluated by
NumPy on float32 arrays (NumPy 2 promotion rules, NEP 50: Python scalars are "weak" and take the array's type, NumPy
scalars and arrays are "strong"), with scipy's brentq.  This is the contract of ``spc_variability_nudge_f32`` (include/spc.h,
INTEGRATION.md "float32"); tests/test_vnudge_f32_gpu.py compares the kernel with it.  A helper module, not collected.

Inputs are rounded to float32 once (the float32 engine does that on upload); R is float64, drawn as the reference draws it
(oracle/vnudge_oracle.py: make_R).  Without AMUSE units, as oracle/vnudge_oracle.py (SI-coherent, factor 1).

Also here: ``npsum32_restated`` (``ndarray.sum()`` of a contiguous float32 array, scalar by scalar: the pairwise tree of
oracle/vnudge_oracle.py's npsum_restated with float32 adds) and ``std32_restated`` (``qt.std(axis=(0, 1))`` of a float32 field:
sequential float32 sums), the orders the kernel reproduces; tests/test_vnudge_f32_cpu.py checks both against NumPy.
"""
import numpy
from scipy.optimize import brentq

F32 = numpy.float32
rlv, cp, rd, pref0 = 2.53e6, 1004., 287.04, 1e5          # splib/sputils.py:14-20, `.number`: Python floats (weak)


def exner(p):                                             # splib/sputils.py:28-29 on a numpy.float32: float32 quotient, powf
    return (p / pref0) ** (rd / cp)


def variability_nudge(qt, qsat, ql_av, qt_av, presf, ql_ref, R, DT, constantT=False, thl=None, ql=None, types=None):
    """One LES, as oracle/vnudge_oracle.variability_nudge but on float32 fields and profiles.  Returns dict(qt, thl, beta,
    alpha, qt_std, a, status, error): qt, thl, qt_std float32; beta, alpha, a float64.  ``types`` (a dict), when given,
    receives the dtype of every intermediate of the contract table (tests/test_vnudge_f32_cpu.py)."""
    qt = numpy.array(qt, dtype=F32)
    qsat = numpy.asarray(qsat, dtype=F32)
    ql_av, qt_av, ql_ref = (numpy.asarray(v, dtype=F32) for v in (ql_av, qt_av, ql_ref))
    p = numpy.asarray(presf, dtype=F32)
    R = numpy.asarray(R, dtype=numpy.float64)
    thl = None if thl is None else numpy.array(thl, dtype=F32)
    ql = None if ql is None else numpy.asarray(ql, dtype=F32)
    types = {} if types is None else types
    itot, jtot, kmax = qt.shape
    beta_min, beta_max = 0, 5                                                   # spcpl.py:659-660
    beta = numpy.ones(kmax)                                                     # spcpl.py:662 (float64)
    a_used = numpy.zeros(kmax)
    status = numpy.zeros(kmax, dtype=numpy.int32)
    error = None
    for k in range(kmax):                                                       # spcpl.py:663
        def get_ql_diff(b):                                                     # spcpl.py:646-648: b weak -> float32
            r = numpy.maximum((b * (qt[:, :, k] - qt_av[k]) + qt_av[k] - qsat[:, :, k]), 0).sum() / (itot * jtot) - ql_ref[k]
            types["get_ql_diff"] = r.dtype
            return r

        def get_ql_diff_additive(a):                                            # spcpl.py:653-656: a * R is float64
            r = numpy.maximum((qt[:, :, k] + (a * R[:, :]) - qsat[:, :, k]), 0).sum() / (itot * jtot) - ql_ref[k]
            types["get_ql_diff_additive"] = r.dtype
            return r

        if ql_ref[k] > 1e-9:                                                    # spcpl.py:665
            q_min, q_max = get_ql_diff(beta_min), get_ql_diff(beta_max)
            if q_min > 0 or q_max < 0:                                          # spcpl.py:669
                beta[k] = beta_max                                              # spcpl.py:673
                status[k] = 16
            else:
                try:
                    beta[k] = brentq(get_ql_diff, beta_min, beta_max)           # spcpl.py:676
                    status[k] = 1
                except (ValueError, RuntimeError) as e:
                    error = e
                    status[k] = 1 | (256 if isinstance(e, ValueError) else 512)
                    continue
        elif ql_av[k] > ql_ref[k]:                                              # spcpl.py:679
            i, j = numpy.unravel_index(numpy.argmax(qt[:, :, k] - qsat[:, :, k]), qt[:, :, k].shape)
            with numpy.errstate(divide="ignore", invalid="ignore"):
                q = (qsat[i, j, k] - qt_av[k]) / (qt[i, j, k] - qt_av[k])      # spcpl.py:683: numpy.float32 scalars
            types["barely_unsaturated"] = q.dtype
            beta[k] = q
            if beta[k] < 0:                                                     # spcpl.py:692-695
                beta[k] = 1
            status[k] = 2
        else:
            continue                                                            # spcpl.py:697
        if beta[k] >= beta_max:                                                 # spcpl.py:703
            if ql_ref[k] > ql_av[k]:                                            # spcpl.py:712
                try:
                    a = brentq(get_ql_diff_additive, 0, 5)                      # spcpl.py:713
                except (ValueError, RuntimeError) as e:
                    error = e
                    status[k] |= 4 | (256 if isinstance(e, ValueError) else 512)
                    beta[k] = 1
                    continue
                a_used[k] = a
                status[k] |= 4
                dQT = a * R                                                     # spcpl.py:716: float64
                types["dQT_additive"] = dQT.dtype
                qt[:, :, k] += dQT                                              # spcpl.py:719: float64 sum, rounded to float32
            else:
                status[k] |= 8
            beta[k] = 1                                                         # spcpl.py:722
        else:
            dQT = (beta[k] - 1) * (qt[:, :, k] - qt_av[k])                      # spcpl.py:724: numpy.float64 scalar (strong)
            types["dQT_multiplicative"] = dQT.dtype
            qt[:, :, k] += dQT                                                  # spcpl.py:725
        if constantT:                                                           # spcpl.py:726-733
            ql_target = numpy.maximum((qt[:, :, k] - qsat[:, :, k]), 0)
            dQL = ql_target - ql[:, :, k]
            dTHL = - rlv / (cp * exner(p[k])) * dQL
            types["dTHL"] = dTHL.dtype
            thl[:, :, k] += dTHL
    alpha = numpy.log(beta) / DT                                                # spcpl.py:739
    qt_std = qt.std(axis=(0, 1))                                                # spcpl.py:743
    types["beta"], types["qt_std"], types["qt"] = beta.dtype, qt_std.dtype, qt.dtype
    return dict(qt=qt, thl=thl, beta=beta, alpha=alpha, qt_std=qt_std, a=a_used, status=status, error=error)


# ---- scalar restatements of the float32 reductions the kernel re-implements ---------------------------------------
def _leaf32(a, lo, n):
    if n < 8:
        res = F32(0)
        for i in range(n):
            res = F32(res + a[lo + i])
        return res
    r = [a[lo + j] for j in range(8)]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] = F32(r[j] + a[lo + i + j])
        i += 8
    res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
    while i < n:
        res = F32(res + a[lo + i])
        i += 1
    return res


def _pairwise32(a, lo, n):
    if n <= 128:
        return _leaf32(a, lo, n)
    n2 = n // 2
    n2 -= n2 % 8
    return F32(_pairwise32(a, lo, n2) + _pairwise32(a, lo + n2, n - n2))


def npsum32_restated(a):
    """ndarray.sum() of a contiguous float32 array, scalar by scalar (float32 adds, float32 total over 8192-element chunks)"""
    a = [F32(x) for x in numpy.asarray(a, dtype=F32).ravel()]
    res, lo = F32(0), 0
    while lo < len(a):
        c = min(8192, len(a) - lo)
        res = F32(res + _pairwise32(a, lo, c))
        lo += c
    return res


def std32_restated(plane):
    """numpy's float32 .std() of one [itot, jtot] level of a [itot, jtot, k] field reduced over axes (0, 1): a sequential float32
    sum in C order, the mean = float32(float64 sum / count) (true_divide by an intp), sequential float32 sum of the squared
    float32 deviations, the same quotient, a float32 sqrt"""
    x = [F32(v) for v in numpy.asarray(plane, dtype=F32).ravel()]
    s = F32(0)
    for v in x:
        s = F32(s + v)
    mean = F32(numpy.float64(s) / len(x))
    q = F32(0)
    for v in x:
        d = F32(v - mean)
        q = F32(q + F32(d * d))
    return numpy.sqrt(F32(numpy.float64(q) / len(x)))
