"""Test-side loader of the plain-C oracle (oracle/libspc_oracle.so). It takes the SAME ctypes
argument structs as the product ABI, but with HOST (NumPy) pointers.  Every wrapper computes in the dtype of its inputs:
float64 arrays go to the oracle_*_f64 entries, float32 arrays to the oracle_*_f32 ones (the float32 contract is stated in
oracle/spc_oracle.c); outputs come back in that dtype."""
import ctypes
import os
import subprocess

import numpy

from sp_coupler_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(ROOT, "oracle", "libspc_oracle.so")
        if not os.path.exists(path):
            subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
        _LIB = ctypes.CDLL(path)
        for t in ("f64", "f32"):
            getattr(_LIB, "oracle_forward_" + t).argtypes = [ctypes.POINTER(_abi.Dims), ctypes.POINTER(_abi.ForwardArgs)]
            getattr(_LIB, "oracle_backward_" + t).argtypes = [ctypes.POINTER(_abi.Dims), ctypes.POINTER(_abi.BackwardArgs)]
            getattr(_LIB, "oracle_cloud_indices_" + t).argtypes = [ctypes.POINTER(_abi.Dims)] + [ctypes.c_void_p] * 3
            getattr(_LIB, "oracle_diagnostics_" + t).argtypes = [ctypes.POINTER(_abi.Dims),
                                                                 ctypes.POINTER(_abi.DiagnosticsArgs)]
            getattr(_LIB, "oracle_surface_fluxes_" + t).argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 8
        _LIB.oracle_pairwise_sum_f32.argtypes = [ctypes.c_void_p, ctypes.c_int64]
        _LIB.oracle_pairwise_sum_f32.restype = ctypes.c_float
        _LIB.oracle_powf.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64]
    return _LIB


_SUFFIX = {numpy.dtype(numpy.float64): "f64", numpy.dtype(numpy.float32): "f32"}


def _fn(name, dtype):
    return getattr(lib(), "oracle_%s_%s" % (name, _SUFFIX[numpy.dtype(dtype)]))


def _p0(a, dtype=None):
    assert a.flags.c_contiguous and a.dtype in (numpy.float64, numpy.float32, numpy.int32)
    assert dtype is None or a.dtype == dtype, (a.dtype, dtype)
    return a.ctypes.data


def forward(gcm, zf, zh, prof, factor, dt, couple_surface=True):
    n, nG = gcm["T"].shape
    nL = prof["U"].shape[1]
    dt_ = gcm["T"].dtype
    _p = lambda x: _p0(x, dt_ if x.dtype != numpy.int32 else None)      # noqa: E731
    a = _abi.ForwardArgs()
    for k, f in (("U", "U"), ("V", "V"), ("T", "T"), ("SH", "SH"), ("QL", "QL"), ("QI", "QI"), ("Pfull", "Pf"),
                 ("Phalf", "Ph"), ("Zgfull", "Zgfull"), ("Zghalf", "Zghalf")):
        setattr(a, f, _p(gcm[k]))
    for k, f in (("U", "u_d"), ("V", "v_d"), ("THL", "thl_d"), ("QT", "qt_d"), ("QL", "ql_d"), ("PS", "ps_d"),
                 ("Rain", "rain"), ("rain_last", "rain_last")):
        setattr(a, f, _p(prof[k]))
    a.zf, a.zh = _p(zf), _p(zh)
    out = {k: numpy.empty((n, nL), dt_) for k in ("f_u", "f_v", "f_thl", "f_qt", "f_ql", "ql_ref", "u", "v", "thl", "qt")}
    out.update({k: numpy.empty(n, dt_) for k in ("f_ps", "ps", "rainrate")})
    out["Zf"], out["Zh"] = numpy.empty((n, nG), dt_), numpy.empty((n, nG + 1), dt_)
    out["idx"] = numpy.empty((n, nG), dtype=numpy.int32)
    if couple_surface:
        for k in ("Z0M", "Z0H", "QLflux", "QIflux", "SHflux", "TSflux"):
            setattr(a, k, _p(gcm[k]))
        out.update({k: numpy.empty(n, dt_) for k in ("z0m", "z0h", "wthl", "wqt")})
    for k, v in out.items():
        setattr(a, k, _p(v))
    a.factor, a.dt = factor, dt
    d = _abi.Dims(n, nG, nL, nG, nG + 1, nL, 1 if zf.ndim == 1 else 0, 0)
    rc = _fn("forward", dt_)(ctypes.byref(d), ctypes.byref(a))
    assert rc == 0, rc
    return out


def backward(gcm, Zf, zf, prof, factor, dt, conservative=False, zh=None, Zh=None):
    n, nG = gcm["T"].shape
    dt_ = gcm["T"].dtype
    _p = lambda x: _p0(x, dt_ if x.dtype != numpy.int32 else None)      # noqa: E731
    a = _abi.BackwardArgs()
    if conservative:
        a.conservative = 1
        a.zh, a.rhobf_d = _p(zh), _p(prof["Rhobf"])
        if Zh is not None:
            a.Zh = _p(Zh)
        else:
            a.Zghalf = _p(gcm["Zghalf"])
    for k in ("T", "SH", "QL", "QI", "U", "V", "A"):
        setattr(a, k, _p(gcm[k]))
    if Zf is not None:
        a.Zf = _p(Zf)
    else:
        a.Zgfull, a.Zghalf = _p(gcm["Zgfull"]), _p(gcm["Zghalf"])
    for k, f in (("T", "t_d"), ("QT", "qt_d"), ("QL", "ql_d"), ("QL_ice", "ql_ice_d"), ("U", "u_d"), ("V", "v_d"),
                 ("A", "A_prof")):
        setattr(a, f, _p(prof[k]))
    a.zf = _p(zf)
    out = {k: numpy.empty((n, nG), dt_) for k in ("f_T", "f_SH", "f_QL", "f_QI", "f_U", "f_V", "f_A")}
    out["start_index"] = numpy.empty(n, dtype=numpy.int32)
    for k, v in out.items():
        setattr(a, k, _p(v))
    a.factor, a.dt = factor, dt
    nL = prof["T"].shape[1]
    d = _abi.Dims(n, nG, nL, nG, nG + 1, nL, 1 if zf.ndim == 1 else 0, 0)
    rc = _fn("backward", dt_)(ctypes.byref(d), ctypes.byref(a))
    assert rc == 0, rc
    return out


def cloud_indices(zh, Zh):
    n, nG1 = Zh.shape
    nL = zh.shape[-1]
    idx = numpy.empty((n, nG1 - 1), dtype=numpy.int32)
    d = _abi.Dims(n, nG1 - 1, nL, nG1 - 1, nG1, nL, 1 if zh.ndim == 1 else 0, 0)
    _p = _p0
    rc = _fn("cloud_indices", Zh.dtype)(ctypes.byref(d), _p(zh, Zh.dtype), _p(Zh), _p(idx))
    assert rc == 0, rc
    return idx


def diagnostics(gcm, zf=None, prof=None):
    """spifs diagnostics (oracle_diagnostics_*): Tv THL QT Zf [n x nG], Zh [n x nG+1] and, with zf / prof (THL, QL,
    QL_ice [n x nL]), pf t ql_water [n x nL]"""
    n, nG = gcm["T"].shape
    dt_ = gcm["T"].dtype
    _p = lambda x: _p0(x, dt_)      # noqa: E731
    a = _abi.DiagnosticsArgs()
    for k, f in (("T", "T"), ("SH", "SH"), ("QL", "QL"), ("QI", "QI"), ("Pfull", "Pf"), ("Zgfull", "Zgfull"),
                 ("Zghalf", "Zghalf")):
        setattr(a, f, _p(gcm[k]))
    out = {k: numpy.empty((n, nG), dt_) for k in ("Tv", "THL", "QT", "Zf")}
    out["Zh"] = numpy.empty((n, nG + 1), dt_)
    nL, shared = 1, 1
    if zf is not None and prof is not None:
        nL, shared = prof["THL"].shape[1], 1 if zf.ndim == 1 else 0
        a.zf = _p(zf)
        for k, f in (("THL", "thl_d"), ("QL", "ql_d"), ("QL_ice", "ql_ice_d")):
            setattr(a, f, _p(prof[k]))
        out.update({k: numpy.empty((n, nL), dt_) for k in ("pf", "t", "ql_water")})
    for k, v in out.items():
        setattr(a, k, _p(v))
    d = _abi.Dims(n, nG, nL, nG, nG + 1, nL, shared, 0)
    rc = _fn("diagnostics", dt_)(ctypes.byref(d), ctypes.byref(a))
    assert rc == 0, rc
    return out


def surface_fluxes(Ph_s, T_s, QLflux, QIflux, SHflux, TSflux):
    """(wthl, wqt) of spcpl.convert_surface_fluxes for [n] scalars (oracle_surface_fluxes_*)"""
    dt_ = Ph_s.dtype
    n = Ph_s.shape[0]
    wthl, wqt = numpy.empty(n, dt_), numpy.empty(n, dt_)
    keep = [numpy.ascontiguousarray(x) for x in (Ph_s, T_s, QLflux, QIflux, SHflux, TSflux)] + [wthl, wqt]
    assert _fn("surface_fluxes", dt_)(n, *[_p0(x, dt_) for x in keep]) == 0
    return wthl, wqt


def pairwise_sum32(a):
    """numpy's float32 pairwise sum of a contiguous float32 array (oracle_pairwise_sum_f32)"""
    a = numpy.ascontiguousarray(a, dtype=numpy.float32)
    return numpy.float32(lib().oracle_pairwise_sum_f32(a.ctypes.data, a.size))


def powf(x, y):
    """x ** y of the float32 contract: spc_powf.h with C99 pow()'s special values (oracle_powf)"""
    x = numpy.ascontiguousarray(x, dtype=numpy.float32)
    out = numpy.empty_like(x)
    lib().oracle_powf(x.ctypes.data, numpy.float32(y), out.ctypes.data, x.size)
    return out
