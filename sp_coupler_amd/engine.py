"""Host launcher for the HIP coupling kernels: torch tensors in HBM -> C ABI (include/spc.h).

PyTorch is plumbing here (device memory, streams); every number is produced by the hand-written
kernels of csrc/ (one translation unit, spc_hip.hip).  There is no CPU fallback: constructing an ``Engine`` without the built
extension or without a GPU raises.

A *plan* (``ForwardPlan`` / ``BackwardPlan``) validates shapes once, freezes the ctypes argument block
and can then be launched repeatedly with one foreign call -- what the per-step driver and ``bench.py``
use, so host overhead per step stays at two launches.
"""
import contextlib
import ctypes

import torch

from . import _abi

SURF_IN = ("Z0M", "Z0H", "QLflux", "QIflux", "SHflux", "TSflux")      # [n]        (spcpl.py:33,138)
FWD_LES = ("U", "V", "THL", "QT", "QL")                               # profile[...] spcpl.py:310-314
BWD_LES = ("T", "QT", "QL", "QL_ice", "U", "V")                       # profile[...] spcpl.py:393-411

_DTYPES = {torch.float64: "f64", torch.float32: "f32"}
LES_STATE_FIELDS = ("U", "V", "THL", "QT")                            # the order set_les_state draws them (spcpl.py:288-291)
LES_STATE_AMPS = (0.5, 0.5, 0.1, 2.5e-5)                              # vabsmax, vabsmax, thlabsmax, qabsmax (spcpl.py:285-287)


def _stream_ptr(stream, device=None):
    """hipStream_t of ``stream`` (default: torch's current stream ON ``device``, not on whatever device
    happens to be current) as a ctypes handle; a stream of another device is rejected."""
    if stream is None:
        stream = torch.cuda.current_stream(device)
    elif device is not None and stream.device != device:
        raise ValueError("stream is on %s, engine is on %s" % (stream.device, device))
    return ctypes.c_void_p(stream.cuda_stream)


def _on_engine_stream(fn):
    """run an Engine method with torch's current stream set to the stream its kernels launch on (``stream=`` argument, else
    the engine's own): tensors it allocates belong to that stream, torch ops it issues (``.contiguous()``) are ordered
    with the launch.  Nothing changes for an engine without a stream called without one."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *a, **kw):
        st = kw.get("stream")
        if st is None:
            st = self.stream
        if st is None:
            return fn(self, *a, **kw)
        with torch.cuda.stream(st):
            return fn(self, *a, **kw)
    return wrapper


class _Checker:
    """Shape / layout validation done on the host BEFORE any launch (a kernel never sees a tensor
    whose extent differs from what its grid assumes)."""

    def __init__(self, device, dtype):
        self.device, self.dtype = device, dtype
        self.keep = []

    def mat(self, name, t, n, m, pitch=None, dtype=None):
        """``dtype``: an argument whose type is fixed whatever the engine's (the float64 R of the nudge)"""
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if t.device != self.device:
            raise ValueError("%s is on %s, engine is on %s" % (name, t.device, self.device))
        if dtype is not None and t.dtype != dtype:
            raise ValueError("%s has dtype %s, must be %s" % (name, t.dtype, dtype))
        if dtype is None and t.dtype != self.dtype:
            raise ValueError("%s has dtype %s, engine computes in %s" % (name, t.dtype, self.dtype))
        if t.dim() != 2 or t.shape[0] != n or t.shape[1] != m:
            raise ValueError("%s must have shape [%d x %d], got %s" % (name, n, m, tuple(t.shape)))
        if m > 1 and t.stride(1) != 1:
            raise ValueError("%s must be contiguous along levels (stride %s)" % (name, t.stride()))
        p = t.stride(0) if n > 1 else (pitch if pitch is not None else max(m, t.stride(0)))
        if pitch is not None and n > 1 and p != pitch:
            raise ValueError("%s has column pitch %d, batch uses %d" % (name, p, pitch))
        if p < m:
            raise ValueError("%s has column pitch %d < %d levels" % (name, p, m))
        self.keep.append(t)
        return t.data_ptr(), p

    def vec(self, name, t, n, dtype=None):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if t.device != self.device or t.dtype != (dtype or self.dtype):
            raise ValueError("%s must be %s on %s" % (name, dtype or self.dtype, self.device))
        if t.dim() != 1 or t.shape[0] != n or (n > 1 and t.stride(0) != 1):
            raise ValueError("%s must be a contiguous vector of %d, got %s" % (name, n, tuple(t.shape)))
        self.keep.append(t)
        return t.data_ptr()


class _Plan:
    """A validated, frozen launch: shapes checked once, ctypes argument block built once, tensors kept alive; ``launch``
    is then ONE foreign call.  ``fn(*call_args, stream)`` is the C-ABI entry point."""

    def __init__(self, engine, fn, call_args, keep, outputs, dims=None, args=None):
        self.engine, self._fn, self._call, self._keep, self.outputs = engine, fn, tuple(call_args), keep, outputs
        self.dims, self.args = dims, args

    def set_scalars(self, factor, dt):
        """forcing factor and time step of the next launches (they change between spin-up and coupled steps)"""
        self.args.factor, self.args.dt = float(factor), float(dt)

    def launch(self, stream=None):
        """Enqueue the kernel on ``stream`` (default: the engine's own stream if it has one, else torch's current
        stream of the engine's device). Returns outputs dict."""
        eng = self.engine
        if stream is None:
            stream = eng.stream
        with torch.cuda.device(eng.device):          # occupancy queries + launch on the engine's device
            rc = self._fn(*self._call, _stream_ptr(stream, eng.device))
        if rc:
            _abi.check(eng.lib, rc)
        return self.outputs

    def launch_raw(self, stream_ptr):
        """Same with a pre-fetched ``ctypes.c_void_p`` stream handle (hot loops). The caller guarantees that the
        handle belongs to the engine's device and that this device is current (``torch.cuda.set_device``)."""
        rc = self._fn(*self._call, stream_ptr)
        if rc:
            _abi.check(self.engine.lib, rc)

    def describe(self):
        """which kernel instantiation / slab size / grid the library picks for this plan (spc_describe_launch)"""
        return _abi.describe_launch(self.engine.lib, self.dims, self._pass, self._flags(), 8 if self.engine.dtype == torch.float64 else 4)


class ForwardPlan(_Plan):
    _pass = 0

    def _flags(self):
        a = self.args
        full = any(getattr(a, f) for f in ("u", "v", "thl", "qt", "ps", "Zf", "Zh", "rainrate", "wthl"))
        return (1 if a.idx else 0) | (2 if full else 0)


class BackwardPlan(_Plan):
    @property
    def _pass(self):
        return 4 if self.args.conservative else 1

    def _flags(self):
        return 0


class DiagnosticsPlan(_Plan):
    _pass = 3

    def _flags(self):
        return 0


class CloudIndexPlan(_Plan):
    _pass = 2

    def _flags(self):
        return 0


class SurfacePlan(_Plan):
    def describe(self):
        return "k_surface"


class OperatorPlan(_Plan):
    """a K7 operator (exner / interp / searchsorted / interp_c / rms) with its arguments frozen: ``run()`` launches and
    returns the result tensor (the caller's ``out=`` or the one allocated when the plan was made)"""

    def __init__(self, engine, fn, call_args, keep, outputs, result, refresh=()):
        super().__init__(engine, fn, call_args, keep, outputs)
        self.result = result
        # (private contiguous copy, the caller's tensor) of every argument whose layout the kernels cannot read in place: the
        # copy is REDONE in front of every launch, so a plan never computes from a stale snapshot of a tensor the caller
        # has updated since (round-4 advisor).  Empty for row-contiguous arguments: run() is then one foreign call.
        self._refresh = tuple(refresh)

    def run(self, stream=None):
        if self._refresh:
            eng = self.engine
            st = stream if stream is not None else eng.stream
            with (torch.cuda.stream(st) if st is not None else contextlib.nullcontext()):
                for snap, src in self._refresh:
                    snap.copy_(src if src.shape == snap.shape else src.expand_as(snap))
        self.launch(stream)
        return self.result

    def launch_raw(self, stream_ptr):
        """the bare foreign call (hot loops) -- only for plans that read every argument in place: a plan holding private
        packed copies must go through run(), which refreshes them, and says so instead of serving a stale snapshot"""
        if self._refresh:
            raise RuntimeError("this plan reads %d argument(s) through private packed copies (non-contiguous or spread inputs): "
                               "use run(), which refreshes them before the launch" % len(self._refresh))
        super().launch_raw(stream_ptr)

    def describe(self):
        return getattr(self._fn, "__name__", "operator")


class Engine:
    """One engine per (device, dtype). ``dtype`` is the arithmetic type of the path: float64 as in
    the reference (AMUSE quantities wrap float64 arrays), float32 for the tolerance sweep."""

    def __init__(self, device=None, dtype=torch.float64, stream=None, lib_path=None):
        """``stream``: a ``torch.cuda.Stream`` every plan and every K7 operator of this engine launches on (None: torch's
        current stream of the device at launch time).  The engine's transfer buffers (``arena``) order their copies
        against the same stream, and the tensors the engine allocates are allocated under it (``on_stream``), so an
        engine with a stream of its own never depends on what stream is current in the caller.  Several such engines on
        ONE device run the row blocks of a ``multi.MultiDeviceEngine`` batch concurrently."""
        self.stream = stream
        # ``lib_path``: another build of the SAME ABI (A/B runs, tools/mutation_control.py); default: the shipped library
        self.lib = _abi.load_library(lib_path)  # raises SpcLibraryError if the HIP extension is missing
        if dtype not in _DTYPES:
            raise ValueError("dtype must be torch.float64 or torch.float32")
        if not torch.cuda.is_available() or self.lib.spc_device_count() < 1:
            raise RuntimeError("sp_coupler_amd.Engine needs a HIP device (MI355X); there is no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        if self.device.type != "cuda":
            raise ValueError("Engine device must be a cuda/HIP device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.dtype = dtype
        sfx = _DTYPES[dtype]
        self._vn_work = None                    # variability_nudge's transposed-plane scratch, grown on demand
        self._exp_tab = None                    # les_radiate's table of exp(-x) on the device, uploaded on first use
        self._es_tab = None                     # les_thermo's saturation-pressure table on the device, uploaded on first use
        self._fwd = getattr(self.lib, "spc_forward_" + sfx)
        self._bwd = getattr(self.lib, "spc_backward_" + sfx)
        self._idx = getattr(self.lib, "spc_cloud_indices_" + sfx)
        self._diag = getattr(self.lib, "spc_diagnostics_" + sfx)

    # -- helpers ----------------------------------------------------------------------------
    def _grid(self, ck, name, z, n, nL, pitchL):
        """LES grid: [nL] shared by all columns or [n x nL]."""
        if z.dim() == 1:
            return ck.vec(name, z, nL), 1
        ptr, _ = ck.mat(name, z, n, nL, pitchL)
        return ptr, 0

    def empty(self, *shape, dtype=None):
        return torch.empty(*shape, device=self.device, dtype=dtype or self.dtype)

    def on_stream(self):
        """context in which torch's current stream IS this engine's stream (allocations, ``.to()`` / ``.cpu()`` copies and
        torch ops issued inside are then ordered with the engine's launches); a no-op for an engine without a stream"""
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def synchronize(self):
        (self.stream if self.stream is not None else torch.cuda.current_stream(self.device)).synchronize()

    # -- transfer plumbing shared with multi.MultiDeviceEngine (which shards the same things over several devices) ----
    def arena(self, specs, rows=None):
        """named arrays in ONE pinned host buffer mirrored by ONE device buffer (transfer.Arena)"""
        from .transfer import Arena
        return Arena(self.device, specs, stream=self.stream)

    def to_devices(self, host_array, rows=None, n_cols=None, dtype=None):
        """the host array on this engine's device, in the engine's dtype or ``dtype`` (variability_nudge's R: float64)"""
        import numpy
        with self.on_stream():
            return torch.from_numpy(numpy.ascontiguousarray(host_array)).to(self.device, dtype or self.dtype)

    # -- K1 (+K2) ---------------------------------------------------------------------------
    @_on_engine_stream
    def plan_forward(self, gcm, zf, prof, factor, dt, zh=None, *, want_profiles=False, want_heights=True,
                     want_idx=None, couple_surface=False, cols_per_block=0, out=None):
        """Arithmetic of convert_profiles + set_les_forcings (splib/spcpl.py:171-246, 299-385) for all
        columns. ``gcm``: dict of the gcm_vars tensors; ``prof``: dict U,V,THL,QT,QL [n x nL], PS [n]
        (+ Rain, rain_last [n]). Output tensors are allocated here (or taken from ``out``)."""
        T_ = gcm["T"]
        n, nG = int(T_.shape[0]), int(T_.shape[1])
        nL = int(prof["U"].shape[1])
        ck = _Checker(self.device, self.dtype)
        a = _abi.ForwardArgs()
        pitchG = pitchGh = pitchL = None
        for key, field in (("U", "U"), ("V", "V"), ("T", "T"), ("SH", "SH"), ("QL", "QL"), ("QI", "QI"),
                           ("Pfull", "Pf"), ("Zgfull", "Zgfull")):
            ptr, pitchG = ck.mat("gcm[%s]" % key, gcm[key], n, nG, pitchG)
            setattr(a, field, ptr)
        for key, field in (("Phalf", "Ph"), ("Zghalf", "Zghalf")):
            ptr, pitchGh = ck.mat("gcm[%s]" % key, gcm[key], n, nG + 1, pitchGh)
            setattr(a, field, ptr)
        for key, field in zip(FWD_LES, ("u_d", "v_d", "thl_d", "qt_d", "ql_d")):
            ptr, pitchL = ck.mat("prof[%s]" % key, prof[key], n, nL, pitchL)
            setattr(a, field, ptr)
        a.ps_d = ck.vec("prof[PS]", prof["PS"], n)
        a.zf, shared = self._grid(ck, "zf", zf, n, nL, pitchL)
        if want_idx is None:
            want_idx = zh is not None
        out = dict(out or {})
        res = {}

        def omat(name, m, pitch):
            t = out.get(name)
            if t is None:
                t = torch.empty(n, pitch or m, device=self.device, dtype=self.dtype)[:, :m]
            ptr, _ = ck.mat("out[%s]" % name, t, n, m, pitch)
            res[name] = t
            return ptr

        def ovec(name):
            t = out.get(name)
            if t is None:
                t = self.empty(n)
            res[name] = t
            return ck.vec("out[%s]" % name, t, n)

        for name in ("f_u", "f_v", "f_thl", "f_qt", "f_ql", "ql_ref"):
            setattr(a, name, omat(name, nL, pitchL))
        a.f_ps = ovec("f_ps")
        if want_profiles:
            for name in ("u", "v", "thl", "qt"):
                setattr(a, name, omat(name, nL, pitchL))
            a.ps = ovec("ps")
        if want_heights:
            a.Zf = omat("Zf", nG, pitchG)
            a.Zh = omat("Zh", nG + 1, pitchGh)
        if want_idx:
            if zh is None:
                raise ValueError("want_idx needs the LES half-level heights zh")
            a.zh, sh2 = self._grid(ck, "zh", zh, n, nL, pitchL)
            if sh2 != shared:
                raise ValueError("zf and zh must both be shared [nL] or both per column [n x nL]")
            idx = out.get("idx")
            if idx is None:  # idx shares the column pitch of the GCM full-level arrays
                idx = torch.empty(n, pitchG or nG, device=self.device, dtype=torch.int32)[:, :nG]
            if (idx.dtype != torch.int32 or idx.device != self.device or tuple(idx.shape) != (n, nG)
                    or (nG > 1 and idx.stride(1) != 1) or (n > 1 and idx.stride(0) != pitchG)):
                raise ValueError("out[idx] must be int32 [%d x %d] with column pitch %d" % (n, nG, pitchG))
            ck.keep.append(idx)
            a.idx = idx.data_ptr()
            res["idx"] = idx
        if "Rain" in prof and "rain_last" in prof:
            a.rain = ck.vec("prof[Rain]", prof["Rain"], n)
            a.rain_last = ck.vec("prof[rain_last]", prof["rain_last"], n)
            a.rainrate = ovec("rainrate")
        if couple_surface:
            for key in SURF_IN:
                setattr(a, key, ck.vec("gcm[%s]" % key, gcm[key], n))
            for name in ("z0m", "z0h", "wthl", "wqt"):
                setattr(a, name, ovec(name))
        a.factor, a.dt = float(factor), float(dt)
        dims = _abi.Dims(n, nG, nL, pitchG or nG, pitchGh or nG + 1, pitchL or nL, shared, int(cols_per_block))
        return ForwardPlan(self, self._fwd, (ctypes.byref(dims), ctypes.byref(a)), ck.keep, res, dims, a)

    @_on_engine_stream
    def forward(self, *args, stream=None, **kw):
        return self.plan_forward(*args, **kw).launch(stream)

    # -- K2 standalone ----------------------------------------------------------------------
    @_on_engine_stream
    def plan_cloud_indices(self, zh, Zh, out=None, cols_per_block=0):
        """searchsorted(zh, Zh, 'right')[:-1][::-1] per column (splib/spcpl.py:26, 764); ``out``: int32 [n x nG]."""
        n, nGp1 = int(Zh.shape[0]), int(Zh.shape[1])
        nG = nGp1 - 1
        nL = int(zh.shape[-1])
        ck = _Checker(self.device, self.dtype)
        Zh_ptr, pitchGh = ck.mat("Zh", Zh, n, nG + 1)
        zh_ptr, shared = self._grid(ck, "zh", zh, n, nL, None)
        pitchL = zh.stride(0) if (zh.dim() == 2 and n > 1) else nL
        idx = out if out is not None else self.empty(n, nG, dtype=torch.int32)
        if (idx.dtype != torch.int32 or idx.device != self.device or tuple(idx.shape) != (n, nG)
                or (nG > 1 and idx.stride(1) != 1)):
            raise ValueError("out must be int32 [%d x %d] on %s, contiguous along levels" % (n, nG, self.device))
        pitchI = idx.stride(0) if n > 1 else nG
        ck.keep.append(idx)
        dims = _abi.Dims(n, nG, nL, pitchI, pitchGh, pitchL, shared, int(cols_per_block))
        return CloudIndexPlan(self, self._idx, (ctypes.byref(dims), zh_ptr, Zh_ptr, idx.data_ptr()), ck.keep, {"idx": idx}, dims)

    @_on_engine_stream
    def cloud_indices(self, zh, Zh, stream=None, cols_per_block=0):
        return self.plan_cloud_indices(zh, Zh, cols_per_block=cols_per_block).launch(stream)["idx"]

    # -- K3 ---------------------------------------------------------------------------------
    @_on_engine_stream
    def plan_backward(self, gcm, zf, prof, factor, dt, Zf=None, *, want_start_index=True, conservative=False,
                      zh=None, Zh=None, cols_per_block=0, out=None):
        """Arithmetic of set_gcm_tendencies (splib/spcpl.py:388-555) for all columns. ``prof``: dict
        T,QT,QL,QL_ice,U,V [n x nL] and A [n x nG] (order of get_cloudfraction(indices))."""
        T_ = gcm["T"]
        n, nG = int(T_.shape[0]), int(T_.shape[1])
        nL = int(prof["T"].shape[1])
        ck = _Checker(self.device, self.dtype)
        a = _abi.BackwardArgs()
        pitchG = pitchGh = pitchL = None
        for key in ("T", "SH", "QL", "QI", "U", "V", "A"):
            ptr, pitchG = ck.mat("gcm[%s]" % key, gcm[key], n, nG, pitchG)
            setattr(a, key, ptr)
        if Zf is not None:
            a.Zf, pitchG = ck.mat("Zf", Zf, n, nG, pitchG)
        else:
            a.Zgfull, pitchG = ck.mat("gcm[Zgfull]", gcm["Zgfull"], n, nG, pitchG)
            a.Zghalf, pitchGh = ck.mat("gcm[Zghalf]", gcm["Zghalf"], n, nG + 1, pitchGh)
        for key, field in zip(BWD_LES, ("t_d", "qt_d", "ql_d", "ql_ice_d", "u_d", "v_d")):
            ptr, pitchL = ck.mat("prof[%s]" % key, prof[key], n, nL, pitchL)
            setattr(a, field, ptr)
        a.A_prof, pitchG = ck.mat("prof[A]", prof["A"], n, nG, pitchG)
        a.zf, shared = self._grid(ck, "zf", zf, n, nL, pitchL)
        a.conservative = 1 if conservative else 0
        if conservative:   # sputils.interp_c needs the half levels of both grids and the LES base density
            if zh is None:
                raise ValueError("conservative coarsening needs the LES half-level heights zh")
            a.zh, sh2 = self._grid(ck, "zh", zh, n, nL, pitchL)
            if sh2 != shared:
                raise ValueError("zf and zh must both be shared [nL] or both per column [n x nL]")
            a.rhobf_d, pitchL = ck.mat("prof[Rhobf]", prof["Rhobf"], n, nL, pitchL)
            if Zh is not None:
                a.Zh, pitchGh = ck.mat("Zh", Zh, n, nG + 1, pitchGh)
            else:
                a.Zghalf, pitchGh = ck.mat("gcm[Zghalf]", gcm["Zghalf"], n, nG + 1, pitchGh)
        a.factor, a.dt = float(factor), float(dt)
        out = dict(out or {})
        res = {}
        for name in ("f_T", "f_SH", "f_QL", "f_QI", "f_U", "f_V", "f_A"):
            t = out.get(name)
            if t is None:   # outputs share the column pitch of the GCM full-level inputs
                t = torch.empty(n, pitchG or nG, device=self.device, dtype=self.dtype)[:, :nG]
            ptr, pitchG = ck.mat("out[%s]" % name, t, n, nG, pitchG)
            setattr(a, name, ptr)
            res[name] = t
        if want_start_index:
            t = out.get("start_index")
            if t is None:
                t = self.empty(n, dtype=torch.int32)
            a.start_index = ck.vec("out[start_index]", t, n, dtype=torch.int32)
            res["start_index"] = t
        dims = _abi.Dims(n, nG, nL, pitchG or nG, pitchGh or nG + 1, pitchL or nL, shared, int(cols_per_block))
        return BackwardPlan(self, self._bwd, (ctypes.byref(dims), ctypes.byref(a)), ck.keep, res, dims, a)

    @_on_engine_stream
    def backward(self, *args, stream=None, **kw):
        return self.plan_backward(*args, **kw).launch(stream)

    # -- the hot-path pair: what a steady-state step launches, and what bench.py / tools time -------
    def plan_exchange(self, gcm, zf, zh, prof, factor_les, factor_gcm, dt, cols_per_block=0):
        """(ForwardPlan, BackwardPlan) of one column-exchange with ONLY the outputs SURVEY 8(d) counts: K1 writes
        the six setter arrays + f_ps + the fused index map (no optional profiles / heights / rain rate), K3
        recomputes Zf from the geopotential (no Zf round trip) and writes the seven tendencies."""
        lean = {k: v for k, v in prof.items() if k not in ("Rain", "rain_last")}
        fp = self.plan_forward(gcm, zf, lean, factor_les, dt, zh=zh, want_profiles=False, want_heights=False,
                               cols_per_block=cols_per_block)
        bp = self.plan_backward(gcm, zf, prof, factor_gcm, dt, Zf=None, want_start_index=False,
                                cols_per_block=cols_per_block)
        return fp, bp

    # -- K5 ---------------------------------------------------------------------------------
    @_on_engine_stream
    def plan_diagnostics(self, gcm, zf=None, prof=None, out=None, cols_per_block=0):
        """spifs.nc diagnostics: Tv, THL, QT, Zf, Zh (splib/spcpl.py:176,197-198,214-215) and, when
        ``zf``/``prof`` are given, pf, t, ql_water on LES levels (splib/spcpl.py:402,408-409).  Output tensors are
        taken from ``out`` where given (views of a transfer buffer), else allocated ONCE here."""
        T_ = gcm["T"]
        n, nG = int(T_.shape[0]), int(T_.shape[1])
        ck = _Checker(self.device, self.dtype)
        a = _abi.DiagnosticsArgs()
        out = dict(out or {})
        pitchG = pitchGh = pitchL = None
        for key, field in (("T", "T"), ("SH", "SH"), ("QL", "QL"), ("QI", "QI"), ("Pfull", "Pf"), ("Zgfull", "Zgfull")):
            ptr, pitchG = ck.mat("gcm[%s]" % key, gcm[key], n, nG, pitchG)
            setattr(a, field, ptr)
        a.Zghalf, pitchGh = ck.mat("gcm[Zghalf]", gcm["Zghalf"], n, nG + 1, pitchGh)
        res = {}
        for name in ("Tv", "THL", "QT", "Zf"):
            t = out.get(name)
            res[name] = t if t is not None else torch.empty(n, pitchG or nG, device=self.device, dtype=self.dtype)[:, :nG]
            ptr, pitchG = ck.mat(name, res[name], n, nG, pitchG)
            setattr(a, name, ptr)
        t = out.get("Zh")
        res["Zh"] = t if t is not None else torch.empty(n, pitchGh or nG + 1, device=self.device, dtype=self.dtype)[:, :nG + 1]
        a.Zh, pitchGh = ck.mat("Zh", res["Zh"], n, nG + 1, pitchGh)
        nL, shared = 1, 1
        if zf is not None and prof is not None:
            nL = int(prof["THL"].shape[1])
            for key, field in (("THL", "thl_d"), ("QL", "ql_d"), ("QL_ice", "ql_ice_d")):
                ptr, pitchL = ck.mat("prof[%s]" % key, prof[key], n, nL, pitchL)
                setattr(a, field, ptr)
            a.zf, shared = self._grid(ck, "zf", zf, n, nL, pitchL)
            for name in ("pf", "t", "ql_water"):
                t = out.get(name)
                res[name] = t if t is not None else torch.empty(n, pitchL or nL, device=self.device, dtype=self.dtype)[:, :nL]
                ptr, pitchL = ck.mat(name, res[name], n, nL, pitchL)
                setattr(a, name, ptr)
        dims = _abi.Dims(n, nG, nL, pitchG or nG, pitchGh or nG + 1, pitchL or nL, shared, int(cols_per_block))
        return DiagnosticsPlan(self, self._diag, (ctypes.byref(dims), ctypes.byref(a)), ck.keep, res, dims, a)

    @_on_engine_stream
    def diagnostics(self, gcm, zf=None, prof=None, stream=None, cols_per_block=0):
        return self.plan_diagnostics(gcm, zf, prof, cols_per_block=cols_per_block).launch(stream)

    # -- variability nudge (qt_forcing == 'variance') ------------------------------------------------
    @_on_engine_stream
    def variability_nudge(self, qt, qsat, R, ql_av, qt_av, ql_ref, presf=None, thl=None, ql=None, constantT=False,
                          stream=None):
        """spcpl.variability_nudge (splib/spcpl.py:613-744) for all columns: ``qt`` [n x itot x jtot x k] is updated
        IN PLACE (``thl`` too with ``constantT``); returns dict beta, a, qt_std [n x k] and status [n x k] int32.
        float64 engine: every tensor float64, bit-identical to NumPy / SciPy.  float32 engine: the fields (qt, qsat, thl,
        ql) and profiles (ql_av, qt_av, ql_ref, presf) float32, R float64; beta and a come back float64, qt_std float32 --
        the reference's lines evaluated by NumPy on float32 arrays (INTEGRATION.md "float32")."""
        f32 = self.dtype == torch.float32
        if self.dtype not in (torch.float64, torch.float32):
            raise ValueError("variability_nudge computes in float64 or float32, engine has %s" % self.dtype)
        if qt.dim() != 4:
            raise ValueError("qt must be [n x itot x jtot x ktot]")
        n, itot, jtot, ktot = (int(x) for x in qt.shape)
        ck = _Checker(self.device, self.dtype)
        fname = "float32" if f32 else "float64"

        def field(name, t):
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != self.dtype or \
                    tuple(t.shape) != (n, itot, jtot, ktot) or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s [%d x %d x %d x %d] tensor on %s" % (name, fname, n, itot, jtot, ktot, self.device))
            ck.keep.append(t)
            return t.data_ptr()
        a = _abi.VnudgeArgs()
        a.n_cols, a.itot, a.jtot, a.ktot, a.constantT = n, itot, jtot, ktot, 1 if constantT else 0
        a.qt, a.qsat = field("qt", qt), field("qsat", qsat)
        # the noise plane is float64 on either engine (spcpl.py:620-621 draws it in float64) and the kernels read it as
        # [n][itot*jtot] with that row pitch: a view of other strides is packed into a copy, which ck keeps alive until
        # the launch along with every other tensor whose pointer it hands out
        if not isinstance(R, torch.Tensor):
            raise TypeError("R must be a torch.Tensor, got %s" % type(R).__name__)
        a.R, _ = ck.mat("R", R.reshape(n, itot * jtot).contiguous(), n, itot * jtot, itot * jtot, dtype=torch.float64)
        for name, t in (("ql_av", ql_av), ("qt_av", qt_av), ("ql_ref", ql_ref)):
            ptr, _ = ck.mat(name, t, n, ktot, ktot)
            setattr(a, name, ptr)
        if constantT:
            a.thl, a.ql = field("thl", thl), field("ql", ql)
            a.presf, _ = ck.mat("presf", presf, n, ktot, ktot)
        res = {k: self.empty(n, ktot, dtype=torch.float64) for k in ("beta", "a")}
        res["qt_std"] = self.empty(n, ktot)
        res["status"] = self.empty(n, ktot, dtype=torch.int32)
        a.beta, a.a_add, a.qt_std, a.status = (res["beta"].data_ptr(), res["a"].data_ptr(), res["qt_std"].data_ptr(),
                                               res["status"].data_ptr())
        # scratch for the transposed qt / qsat planes (include/spc.h: spc_vnudge_args.work), kept between calls and sized
        # by the library
        need = int((self.lib.spc_vnudge_workspace_bytes_f32 if f32 else self.lib.spc_vnudge_workspace_bytes)(n, itot, jtot, ktot))
        if need < 0:
            _abi.check(self.lib, need)
        if self._vn_work is None or self._vn_work.numel() < need:
            self._vn_work = None
            self._vn_work = torch.empty(need, dtype=torch.uint8, device=self.device)
        a.work, a.work_bytes = self._vn_work.data_ptr(), self._vn_work.numel()
        self._call(self._sym("variability_nudge"), ctypes.byref(a), stream=stream)
        return res

    # -- K10: horizontal reductions of device-resident LES fields (les.get_profile_*, les.get_cloudfraction) ----------
    def _field4(self, name, t, shape=None):
        """a contiguous [n x itot x jtot x ktot] tensor of the engine's dtype on its device (as variability_nudge asks)"""
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if t.device != self.device or t.dtype != self.dtype or t.dim() != 4 or not t.is_contiguous() or \
                (shape is not None and tuple(t.shape) != tuple(shape)):
            raise ValueError("%s must be a contiguous %s [n x itot x jtot x ktot] tensor%s on %s, got %s %s on %s"
                             % (name, self.dtype, "" if shape is None else " of shape %s" % (tuple(shape),), self.device,
                                t.dtype, tuple(t.shape), t.device))
        return t

    # -- one copy of what the K10 - K23 methods below have in common ---------------------------------------------------------------
    @property
    def _esize(self):
        return 4 if self.dtype == torch.float32 else 8

    def _sym(self, name):
        """the library's entry point ``spc_<name>_f32`` / ``_f64`` of the engine's dtype"""
        return getattr(self.lib, "spc_%s_%s" % (name, _DTYPES[self.dtype]))

    def _geometry(self, name, *extents):
        """what the library's ``spc_les_<name>(extents ..., element size)`` says of a launch at these extents in the engine's dtype"""
        return int(getattr(self.lib, "spc_les_" + name)(*(int(x) for x in extents), self._esize))

    def _extents(self, what, name, t):
        """(n, itot, jtot, ktot) of the 4-D field ``t`` (``_field4``'s checks under ``name``); an empty plane or column is refused"""
        shape = tuple(int(x) for x in self._field4(name, t).shape)
        if min(shape[1:]) < 1:
            raise ValueError("%s: empty field shape %s" % (what, shape))
        return shape

    def _plane(self, name, t, shape, dtype=None):
        """``t``, a contiguous tensor of ``shape`` and ``dtype`` (default: the engine's) on the engine's device"""
        dtype = dtype or self.dtype
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), self.device))
        return t

    def _largest(self, ck, name, want, n):
        """the optional [n] output ``name``: a fresh tensor for True, the caller's (checked) tensor, None for False / None"""
        if want is None or want is False:
            return None
        res = torch.empty(n, dtype=self.dtype, device=self.device) if want is True else want
        ck.vec(name, res, n)
        return res

    @staticmethod
    def _no_alias(text, written, read, n=1):
        """refuse with ``text`` a written tensor that STARTS where a read tensor or another written one starts (None: not
        given); views that overlap in part are not detected, and with ``n == 0`` nothing is"""
        written = [t.data_ptr() for t in written if t is not None]
        if n and (len(set(written)) != len(written) or set(written) & set(t.data_ptr() for t in read if t is not None)):
            raise ValueError(text)

    @staticmethod
    def _same_pitch(what, p, pitch, n, others="the others"):
        """the row pitch ``p`` of the output ``what``, which is the pitch of those before it (``pitch``; None: it is the first)"""
        if pitch is not None and n > 1 and p != pitch:
            raise ValueError("%s has row pitch %d, %s %d" % (what, p, others, pitch))
        return p

    @_on_engine_stream
    def slab_means(self, fields, out=None, stream=None):
        """``{name: numpy.mean(field[l], axis=(0, 1)) for every LES l}`` of device fields [n x itot x jtot x ktot] of ONE
        shape, bit for bit, in ONE launch for all of them (at most ``_abi.SLAB_MAX_FIELDS``): dict name -> [n x ktot].
        ``out``: dict name -> [n x ktot] tensors to write into (rows may be pitched, all with one pitch)."""
        names = list(fields)
        if not 1 <= len(names) <= _abi.SLAB_MAX_FIELDS:
            raise ValueError("slab_means takes 1 ... %d fields per launch, got %d" % (_abi.SLAB_MAX_FIELDS, len(names)))
        shape = n, itot, jtot, ktot = self._extents("slab_means", names[0], fields[names[0]])
        a = _abi.SlabMeansArgs()
        a.n_les, a.itot, a.jtot, a.ktot, a.n_fields = n, itot, jtot, ktot, len(names)
        res, pitch = {}, None
        for f, name in enumerate(names):
            a.fields[f] = self._field4(name, fields[name], shape).data_ptr()
            o, p = self._out(None if out is None else out[name], n, ktot)
            pitch = self._same_pitch("slab_means: out[%s]" % name, p, pitch, n)
            a.out[f] = o.data_ptr()
            res[name] = o
        a.pitch_out = pitch
        self._call(self._sym("slab_means"), ctypes.byref(a), stream=stream)
        return res

    @_on_engine_stream
    def slab_cloud_fraction(self, ql, idx, out=None, stream=None):
        """les.get_cloudfraction(indices) (splib/spcpl.py:764-765) of every LES from its device-resident QL field
        [n x itot x jtot x ktot] and K2's index map ``idx`` [n x nG] int32 (``cloud_indices`` / the fused K1 output): the
        fraction of (i, j) columns with ql > 0 at some LES level of GCM layer r (include/spc.h), [n x nG], exact."""
        n, itot, jtot, ktot = self._extents("slab_cloud_fraction", "ql", ql)
        if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.shape[0] != n:
            raise ValueError("idx must be an [n x nG] tensor with n = %d" % n)
        nG = int(idx.shape[1])
        ck = _Checker(self.device, self.dtype)
        a = _abi.SlabCloudArgs()
        a.n_les, a.itot, a.jtot, a.ktot, a.nG = n, itot, jtot, ktot, nG
        a.idx, a.pitch_idx = ck.mat("idx", idx, n, nG, dtype=torch.int32)
        o, a.pitch_out = self._out(out, n, nG)
        a.ql, a.out = ql.data_ptr(), o.data_ptr()
        self._call(self._sym("slab_cloud_fraction"), ctypes.byref(a), stream=stream)
        return o

    # -- K11: one step of device-resident LES fields and the slab means of the stepped fields, one launch ---------------
    @_on_engine_stream
    def les_advance(self, fields, tend, dt, qsat=None, sat=None, ql=None, means=None, ql_mean=True, stream=None):
        """``field += (tend * dt)[:, None, None, :]`` IN PLACE for every name of ``fields`` (dict name -> contiguous
        [n x itot x jtot x ktot] tensor, at most ``_abi.ADVANCE_MAX_FIELDS`` of one shape) that ``tend`` (dict name ->
        [n x ktot], rows may be pitched, all with one pitch) holds; a field without a tendency keeps its bits.  With
        ``sat`` (the name of the QT field) and ``qsat``: ``q = max(fields[sat] - qsat, 0)`` of the UPDATED field (NaN stays
        NaN, -0.0 gives +0.0: include/spc.h), written to ``ql`` where given.  Returns the slab means of the new fields,
        dict name -> [n x ktot] (``Engine.slab_means``' rule, bit for bit), with ``"QL"`` = the mean of q when ``sat`` is
        given and ``ql_mean`` is true.  ``means``: dict name -> [n x ktot] tensors to write into (``"QL"`` included), pitched
        as in ``slab_means``.  One launch; a field of one level (ktot == 1) is refused (SPC_ERR_UNSUPPORTED)."""
        names = list(fields)
        if not 1 <= len(names) <= _abi.ADVANCE_MAX_FIELDS:
            raise ValueError("les_advance takes 1 ... %d fields per launch, got %d" % (_abi.ADVANCE_MAX_FIELDS, len(names)))
        unknown = [k for k in tend if k not in fields]
        if unknown:
            raise ValueError("les_advance: tendencies %s have no field" % unknown)
        if (sat is None) != (qsat is None):
            raise ValueError("les_advance: sat (the name of the QT field) and qsat come together")
        if sat is not None and sat not in fields:
            raise ValueError("les_advance: sat = %r is not one of the fields %s" % (sat, names))
        if sat is None and ql is not None:
            raise ValueError("les_advance: ql needs sat and qsat")
        if sat is not None and ql_mean and "QL" in fields:
            raise ValueError("les_advance: the mean of q is returned as 'QL', which is also the name of a field")
        shape = n, itot, jtot, ktot = self._extents("les_advance", names[0], fields[names[0]])
        ck = _Checker(self.device, self.dtype)
        a = _abi.LesAdvanceArgs()
        a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.dt = n, itot, jtot, ktot, len(names), float(dt)
        a.pitch_tend = a.pitch_mean = ktot
        res, pitch, pitch_t = {}, None, None

        def mean_of(name):
            nonlocal pitch
            o, p = self._out(None if means is None or name not in means else means[name], n, ktot)
            pitch = self._same_pitch("les_advance: means[%s]" % name, p, pitch, n)
            res[name] = o
            return o.data_ptr()
        for f, name in enumerate(names):
            a.fields[f] = self._field4(name, fields[name], shape).data_ptr()
            if name in tend:
                a.tend[f], pitch_t = ck.mat("tend[%s]" % name, tend[name], n, ktot, pitch=pitch_t)
            a.mean[f] = mean_of(name)
        a.sat_field = -1
        if sat is not None:
            a.sat_field = names.index(sat)
            a.qsat = self._field4("qsat", qsat, shape).data_ptr()
            if ql is not None:
                a.ql = self._field4("ql", ql, shape).data_ptr()
            if ql_mean:
                a.ql_mean = mean_of("QL")
        a.pitch_mean = pitch
        if pitch_t is not None:
            a.pitch_tend = pitch_t
        self._call(self._sym("les_advance"), ctypes.byref(a), stream=stream)
        return res

    # -- K12: saturation adjustment of device-resident LES fields and the slab means of QL and T, one launch -------------
    @_on_engine_stream
    def les_thermo(self, thl, qt, presf, ex, n_iter=None, qsat=None, ql=None, temp=None, means=True, stream=None, table_mode=0):
        """Qsat, QL (and T where ``temp`` is given) of every cell of the device fields ``thl`` and ``qt`` (contiguous
        [n x itot x jtot x ktot], read only) at the pressures ``presf`` [n x ktot] with the Exner factors ``ex`` [n x ktot]
        (``thermo.exner(presf)``; rows may be pitched, both with one pitch): ``n_iter`` Newton iterations (default
        ``thermo.DEFAULT_N_ITER``) over the saturation-pressure table of ``thermo.saturation_table`` (include/spc.h has the
        rule).  ``qsat`` and ``ql`` are written where given (else scratch tensors of the call receive them).  Returns
        ``{"QL": ..., "T": ...}``, the slab means [n x ktot] of QL and T (``Engine.slab_means``' rule, bit for bit);
        ``means``: True, a dict of tensors to write into (pitched as in ``slab_means``), or False (no means: {}).
        ``table_mode``: ``_abi.THERMO_TABLE_*`` (0: the library's choice).  One launch; ktot == 1 is refused
        (SPC_ERR_UNSUPPORTED)."""
        from . import thermo
        shape = n, itot, jtot, ktot = self._extents("les_thermo", "thl", thl)
        n_iter = thermo.DEFAULT_N_ITER if n_iter is None else int(n_iter)
        if n_iter < 0:
            raise ValueError("les_thermo: n_iter = %d < 0" % n_iter)
        if self._es_tab is None:
            self._es_tab = torch.from_numpy(thermo.saturation_table(self.dtype)).to(self.device)
        ck = _Checker(self.device, self.dtype)
        a = _abi.LesThermoArgs()
        a.n_les, a.itot, a.jtot, a.ktot, a.n_iter, a.table_mode = n, itot, jtot, ktot, n_iter, int(table_mode)
        a.thl, a.qt = thl.data_ptr(), self._field4("qt", qt, shape).data_ptr()
        a.presf, a.pitch_prof = ck.mat("presf", presf, n, ktot)
        a.ex, _ = ck.mat("ex", ex, n, ktot, pitch=a.pitch_prof)
        a.es_tab, a.n_tab, a.t_lo, a.inv_step = self._es_tab.data_ptr(), int(self._es_tab.numel()), thermo.T_LO, thermo.INV_STEP
        keep = [torch.empty_like(thl) if t is None else self._field4(name, t, shape) for name, t in (("qsat", qsat), ("ql", ql))]
        a.qsat, a.ql = keep[0].data_ptr(), keep[1].data_ptr()
        if temp is not None:
            a.temp = self._field4("temp", temp, shape).data_ptr()
        res, a.pitch_mean = {}, ktot
        if means is not False and means is not None:
            given = means if isinstance(means, dict) else {}
            unknown = [k for k in given if k not in ("QL", "T")]
            if unknown:
                raise ValueError("les_thermo: means of %s are not computed (QL and T are)" % unknown)
            res["QL"], pitch = self._out(given.get("QL"), n, ktot)
            res["T"], pitch_t = self._out(given.get("T"), n, ktot)
            self._same_pitch("les_thermo: means[T]", pitch_t, pitch, n, others="means[QL]")
            a.ql_mean, a.t_mean, a.pitch_mean = res["QL"].data_ptr(), res["T"].data_ptr(), pitch
        self._call(self._sym("les_thermo"), ctypes.byref(a), stream=stream)
        return res

    # -- K13: column water paths, cloud top and cloud cover of device-resident LES fields, one launch ---------------------
    @_on_engine_stream
    def les_water_paths(self, fields, w, cloud=None, out=None, top=False, cover=False, stream=None):
        """``{name: numpy.add.reduce(field * w[:, None, None, :], axis=3)}`` of device fields [n x itot x jtot x ktot] of ONE
        shape (at most ``_abi.WP_MAX_FIELDS``) and the weight profile ``w`` [n x ktot] (rows may be pitched), bit for bit
        (include/spc.h has the rule), in ONE launch for all of them: dict name -> [n x itot x jtot].  ``cloud``: the name of
        the field the cloud outputs are taken from; with it ``top`` adds ``"top"`` (int32 [n x itot x jtot]: the largest k
        with field > 0, else -1) and ``cover`` adds ``"cover"`` ([n]: the fraction of (i, j) with top >= 0, exact).  ``top``
        and ``cover`` are True or a tensor to write into; ``out``: dict name -> contiguous [n x itot x jtot] tensors to write
        into.  ktot > ``_abi.WP_MAX_KTOT`` is refused (SPC_ERR_UNSUPPORTED)."""
        names = list(fields)
        if not 1 <= len(names) <= _abi.WP_MAX_FIELDS:
            raise ValueError("les_water_paths takes 1 ... %d fields per launch, got %d" % (_abi.WP_MAX_FIELDS, len(names)))
        if any(k in ("top", "cover") for k in names):
            raise ValueError("les_water_paths: 'top' and 'cover' name the cloud outputs, not fields")
        wants = [k for k, v in (("top", top), ("cover", cover)) if v is not False and v is not None]
        if wants and cloud is None:
            raise ValueError("les_water_paths: %s need cloud (the name of a field)" % " and ".join(wants))
        if cloud is not None and cloud not in fields:
            raise ValueError("les_water_paths: cloud = %r is not one of the fields %s" % (cloud, names))
        shape = n, itot, jtot, ktot = self._extents("les_water_paths", names[0], fields[names[0]])
        ck = _Checker(self.device, self.dtype)
        a = _abi.WaterPathArgs()
        a.n_les, a.itot, a.jtot, a.ktot, a.n_fields = n, itot, jtot, ktot, len(names)
        a.w, a.pitch_w = ck.mat("w", w, n, ktot)

        def plane(name, t, dtype, shp):
            if t is None or t is True:
                return torch.empty(shp, dtype=dtype, device=self.device)
            return self._plane("les_water_paths: " + name, t, shp, dtype)
        res = {}
        for f, name in enumerate(names):
            a.fields[f] = self._field4(name, fields[name], shape).data_ptr()
            res[name] = plane("out[%s]" % name, None if out is None else out.get(name), self.dtype, (n, itot, jtot))
            a.out[f] = res[name].data_ptr()
        a.cloud_field = -1
        if wants:
            a.cloud_field = names.index(cloud)
            if "top" in wants:
                res["top"] = plane("top", top, torch.int32, (n, itot, jtot))
                a.top = res["top"].data_ptr()
            if "cover" in wants:
                res["cover"] = plane("cover", cover, self.dtype, (n,))
                a.cover = res["cover"].data_ptr()
        self._no_alias("les_water_paths: an output is an input or another output", [t for t in res.values() if t.numel()],
                       [fields[k] for k in names] + [w])
        self._call(self._sym("les_water_paths"), ctypes.byref(a), stream=stream)
        return res

    # -- K14: warm-rain microphysics of device-resident LES fields and the slab means of what it changes, one launch ------
    @_on_engine_stream
    def les_microphysics(self, qt, ql, qr, qr_new, sed_out, sed_in, lcpex, w, dt, thl=None, temp=None, rain=None, means=True,
                         qc0=None, k_auto=None, k_acc=None, t_up=None, t_dn=None, stream=None):
        """One step of the warm-rain microphysics (include/spc.h has the rule) on contiguous device fields
        [n x itot x jtot x ktot]: cloud water ``ql`` (read only) above ``qc0`` and next to rain turns into rain, the rain
        ``qr`` (read only) falls one upwind step; ``qt`` (and ``thl`` where given) are updated IN PLACE, the new rain is written
        to ``qr_new`` (another tensor than ``qr``), what leaves level 0 is added to ``rain`` [n x itot x jtot] where given.
        ``sed_out``, ``sed_in``, ``lcpex``, ``w`` [n x ktot] are ``microphysics.profiles`` in the engine's dtype (rows may be
        pitched, all with one pitch).  With ``temp`` (the cells' temperature, read only) the cloud ice is formed as well.
        Returns the slab means [n x ktot] of the new fields (``Engine.slab_means``' rule, bit for bit): ``{"QT", "QR"}``, ``"THL"``
        with ``thl`` and ``"QI"`` with ``temp``; ``means``: True, a dict of tensors to write into (pitched as in
        ``slab_means``), or False (no means: {}).  The constants default to those of ``microphysics``.  A written tensor that
        STARTS where another argument starts is refused (ValueError); views that overlap in part are not detected.  One launch; ktot == 1 is
        refused (SPC_ERR_UNSUPPORTED)."""
        from . import microphysics as mp
        shape = n, itot, jtot, ktot = self._extents("les_microphysics", "qt", qt)
        ck = _Checker(self.device, self.dtype)
        a = _abi.LesMicroArgs()
        a.n_les, a.itot, a.jtot, a.ktot, a.dt = n, itot, jtot, ktot, float(dt)
        for name, v, d in (("qc0", qc0, mp.QC0), ("k_auto", k_auto, mp.K_AUTO), ("k_acc", k_acc, mp.K_ACC), ("t_up", t_up, mp.T_UP),
                           ("t_dn", t_dn, mp.T_DN)):
            setattr(a, name, float(d if v is None else v))
        fields = {"qt": qt, "ql": ql, "qr": qr, "qr_new": qr_new, "thl": thl, "temp": temp}
        for name, t in fields.items():
            if t is not None:
                setattr(a, name, self._field4(name, t, shape).data_ptr())
            elif name not in ("thl", "temp"):
                raise ValueError("les_microphysics: %s is required" % name)
        a.sed_out, a.pitch_prof = ck.mat("sed_out", sed_out, n, ktot)
        profs = {"sed_out": sed_out, "sed_in": sed_in, "lcpex": lcpex, "w": w}
        for name in ("sed_in", "lcpex", "w"):
            ptr, _ = ck.mat(name, profs[name], n, ktot, pitch=a.pitch_prof)
            setattr(a, name, ptr)
        if rain is not None:
            a.rain = self._plane("les_microphysics: rain", rain, (n, itot, jtot)).data_ptr()
        res, a.pitch_mean = {}, ktot
        if means is not False and means is not None:
            given = means if isinstance(means, dict) else {}
            names = ["QT", "QR"] + (["THL"] if thl is not None else []) + (["QI"] if temp is not None else [])
            unknown = [k for k in given if k not in names]
            if unknown:
                raise ValueError("les_microphysics: means of %s are not computed (%s are)" % (unknown, names))
            pitch = None
            for k in names:
                res[k], p = self._out(given.get(k), n, ktot)
                pitch = self._same_pitch("les_microphysics: means[%s]" % k, p, pitch, n)
                setattr(a, {"QT": "qt_mean", "QR": "qr_mean", "THL": "thl_mean", "QI": "qi_mean"}[k], res[k].data_ptr())
            a.pitch_mean = pitch
        self._no_alias("les_microphysics: a written array is an input or another written array (qr_new must not be qr)",
                       [qt, qr_new, thl, rain] + list(res.values()), [ql, qr, temp] + list(profs.values()), n)
        self._call(self._sym("les_microphysics"), ctypes.byref(a), stream=stream)
        return res

    # -- K15: implicit vertical diffusion of device-resident LES fields with the surface fluxes, one launch -----------------
    @_on_engine_stream
    def les_diffuse(self, fields, a, m, cp, s0=None, flux=None, stream=None):
        """One backward-Euler step of the vertical diffusion (include/spc.h has the rule) IN PLACE on every tensor of ``fields``
        (dict name -> contiguous [n x itot x jtot x ktot], at most ``_abi.SPC_DIFFUSE_MAX_FIELDS`` of one shape).  ``a``, ``m``,
        ``cp`` [n x ktot] and ``s0`` [n] are ``diffusion.profiles`` in the engine's dtype (rows may be pitched, all with one
        pitch).  ``flux``: dict name -> [n], the kinematic surface flux (positive upward) that enters level 0 of that field;
        fields without one take none, and ``s0`` may be None when no field has one.  A field that STARTS where another field,
        a profile, ``s0`` or a flux starts is refused (ValueError); views that overlap in part are not detected.  One launch;
        more levels than ``diffuse_cols_per_block`` carries are refused (SPC_ERR_UNSUPPORTED)."""
        names = list(fields)
        if not 1 <= len(names) <= _abi.SPC_DIFFUSE_MAX_FIELDS:
            raise ValueError("les_diffuse takes 1 ... %d fields per launch, got %d" % (_abi.SPC_DIFFUSE_MAX_FIELDS, len(names)))
        flux = {} if flux is None else flux
        unknown = [k for k in flux if k not in fields]
        if unknown:
            raise ValueError("les_diffuse: fluxes %s have no field" % unknown)
        flux = {k: v for k, v in flux.items() if v is not None}
        if flux and s0 is None:
            raise ValueError("les_diffuse: a flux needs s0")
        shape = n, itot, jtot, ktot = self._extents("les_diffuse", names[0], fields[names[0]])
        ck = _Checker(self.device, self.dtype)
        g = _abi.LesDiffuseArgs()
        g.n_les, g.itot, g.jtot, g.ktot, g.n_fields = n, itot, jtot, ktot, len(names)
        g.a, g.pitch_prof = ck.mat("a", a, n, ktot)
        g.m, _ = ck.mat("m", m, n, ktot, pitch=g.pitch_prof)
        g.cp, _ = ck.mat("cp", cp, n, ktot, pitch=g.pitch_prof)
        read = [a, m, cp]
        if s0 is not None:
            g.s0 = ck.vec("s0", s0, n)
            read.append(s0)
        for f, name in enumerate(names):
            g.fields[f] = self._field4(name, fields[name], shape).data_ptr()
            if name in flux:
                g.flux[f] = ck.vec("flux[%s]" % name, flux[name], n)
                read.append(flux[name])
        self._no_alias("les_diffuse: a field is another field, a profile, s0 or a flux", [fields[k] for k in names], read, n)
        self._call(self._sym("les_diffuse"), ctypes.byref(g), stream=stream)

    def diffuse_cols_per_block(self, ktot):
        """columns of ``ktot`` levels a workgroup of K15 takes into LDS in the engine's dtype (64, 32 or 16); 0: unsupported"""
        return self._geometry("diffuse_cols_per_block", ktot)

    # -- K16: horizontal upwind advection of device-resident LES fields on the periodic plane, one launch ----------------------
    @_on_engine_stream
    def les_advect(self, fields, out, u, v, hx, hy, cmax=True, stream=None):
        """One explicit upwind step of the horizontal advection (include/spc.h has the rule) of every tensor of ``fields`` (dict
        name -> contiguous [n x itot x jtot x ktot], at most ``_abi.SPC_ADVECT_MAX_FIELDS`` of one shape, read only) by the
        winds ``u`` and ``v`` (the same shape, read only; a field may be ``u`` or ``v`` itself) into the tensors of ``out``
        (the same names, written whole).  ``hx`` and ``hy`` [n] are ``advection.coefficients`` in the engine's dtype.
        ``cmax``: True (a fresh [n] tensor), a tensor [n] to write into, or False / None; returned: the largest Courant sum of
        every LES, or None.  ``fields`` may be empty with a ``cmax``: the probe, which reads the winds only.  An ``out`` that
        STARTS where an input, ``cmax`` or another ``out`` starts is refused (ValueError); views that overlap in part are not
        detected.  One launch."""
        return self._les_transport_step("les_advect", _abi.LesAdvectArgs, _abi.SPC_ADVECT_MAX_FIELDS, fields, out, u, v, hx, hy, None, cmax, {},
                                        None, stream)

    def _les_transport_step(self, name, args, cap, fields, out, u, v, hx, hy, profiles, cmax, extras, limiter, stream):
        """the one body of ``les_advect``, ``les_vadvect``, ``les_transport`` and ``les_transport2``: ``name`` is the public
        method's (in every message, and ``spc_<name>_*`` is the library's symbol), ``args`` the class of its argument block,
        ``cap`` its fields per launch, ``profiles`` (g, r) or None for a kernel without them, ``extras`` the optional written
        tensors beyond ``cmax`` in the block's order ({"mtop": ...} / {"mtop": ..., "ftop": ...}; None: not given), ``limiter`` the
        code of the block's limiter or None for a kernel without one.  Returns ``cmax``'s tensor or None."""
        names = list(fields)
        if len(names) > cap:
            raise ValueError("%s takes at most %d fields per launch, got %d" % (name, cap, len(names)))
        if sorted(out) != sorted(names):
            raise ValueError("%s: out holds %s, the fields are %s" % (name, sorted(out), sorted(names)))
        want = cmax is not None and cmax is not False
        if not names and not want and extras.get("mtop") is None:
            probes = ["field", "cmax"] + [k for k in extras if k == "mtop"]               # what a launch without a field can be for
            raise ValueError("%s: no %s and no %s: nothing to do" % (name, ", no ".join(probes[:-1]), probes[-1]))
        if not names and extras.get("ftop") is not None:
            raise ValueError("%s: ftop without a field" % name)
        shape = n, itot, jtot, ktot = self._extents(name, "u", u)
        ck = _Checker(self.device, self.dtype)
        a = args()
        a.n_les, a.itot, a.jtot, a.ktot, a.n_fields = n, itot, jtot, ktot, len(names)
        if limiter is not None:
            a.limiter = limiter
        a.u, a.v = u.data_ptr(), self._field4("v", v, shape).data_ptr()
        a.hx, a.hy = ck.vec("hx", hx, n), ck.vec("hy", hy, n)
        read = [u, v, hx, hy]
        if profiles is not None:
            g, r = profiles
            a.g, a.pitch_prof = ck.mat("g", g, n, ktot)
            a.r, _ = ck.mat("r", r, n, ktot, pitch=a.pitch_prof)
            read += [g, r]
        res = self._largest(ck, "cmax", cmax, n)
        if want:
            a.cmax = res.data_ptr()
        for k, t in extras.items():
            if t is not None:
                setattr(a, k, self._field4(k, t, shape if k == "mtop" else (len(names), n, itot, jtot)).data_ptr())
        for f, k in enumerate(names):
            a.fields[f] = self._field4(k, fields[k], shape).data_ptr()
            a.out[f] = self._field4("out[%s]" % k, out[k], shape).data_ptr()
        self._no_alias("%s: an output is an input, %s or another output" % (name, ", ".join(["cmax"] + list(extras))),
                       [out[k] for k in names] + [res] + list(extras.values()), read + [fields[k] for k in names], n)
        self._call(self._sym(name), ctypes.byref(a), stream=stream)
        return res

    def advect_strip(self, n, itot, jtot, ktot):
        """(cells of the run [jtot x ktot] of one row i, rows i) a workgroup of K16 owns at these extents in the engine's dtype"""
        return self._geometry("advect_strip", jtot, ktot), int(self.lib.spc_les_advect_rows(int(n), int(itot), int(jtot), int(ktot)))

    # -- K17: vertical upwind advection of device-resident LES fields from continuity, one launch ---------------------------------
    @_on_engine_stream
    def les_vadvect(self, fields, out, u, v, hx, hy, g, r, cmax=True, mtop=None, stream=None):
        """One explicit upwind step of the vertical advection (include/spc.h has the rule) of every tensor of ``fields`` (dict
        name -> contiguous [n x itot x jtot x ktot], at most ``_abi.SPC_VADVECT_MAX_FIELDS`` of one shape, read only) by the
        mass flux that continuity gives the winds ``u`` and ``v`` (the same shape, read only; a field may be ``u`` or ``v``
        itself) into the tensors of ``out`` (the same names, written whole).  ``hx`` and ``hy`` [n] are
        ``advection.coefficients``, ``g`` and ``r`` [n x ktot] ``advection.vertical_profiles`` in the engine's dtype (rows may be
        pitched, both with one pitch).  ``cmax``: True (a fresh [n] tensor), a tensor [n] to write into, or False / None;
        returned: the largest vertical Courant sum of every LES, or None.  ``mtop``: a tensor of the fields' shape that takes
        the mass flux through the upper face of every cell, or None.  ``fields`` may be empty with ``cmax`` and / or ``mtop``:
        the probe.  A written tensor that STARTS where an input or another written tensor starts is refused (ValueError);
        views that overlap in part are not detected.  One launch; more levels than ``vadvect_cols_per_block`` carries are
        refused (SPC_ERR_UNSUPPORTED)."""
        return self._les_transport_step("les_vadvect", _abi.LesVadvectArgs, _abi.SPC_VADVECT_MAX_FIELDS, fields, out, u, v, hx, hy, (g, r), cmax,
                                        {"mtop": mtop}, None, stream)

    def vadvect_cols_per_block(self, ktot):
        """columns of ``ktot`` levels a workgroup of K17 takes into LDS in the engine's dtype (64, 32 or 16); 0: unsupported"""
        return self._geometry("vadvect_cols_per_block", ktot)

    # -- K22: conservative flux-form transport of device-resident LES fields along i, j and k, one launch -------------------------
    @_on_engine_stream
    def les_transport(self, fields, out, u, v, hx, hy, g, r, cmax=True, mtop=None, ftop=None, stream=None):
        """One unsplit donor-cell step in flux form (include/spc.h has the rule) of every tensor of ``fields`` (dict name ->
        contiguous [n x itot x jtot x ktot], at most ``_abi.SPC_TRANSPORT_MAX_FIELDS`` of one shape, read only) by the winds
        ``u`` and ``v`` (the same shape, read only; a field may be ``u`` or ``v`` itself) and the mass flux that continuity
        gives them, into the tensors of ``out`` (the same names, written whole).  ``hx``, ``hy``, ``g`` and ``r`` are those of
        ``les_vadvect``.  ``cmax``: True (a fresh [n] tensor), a tensor [n] to write into, or False / None; returned: the
        largest outflow Courant sum of every LES, or None.  ``mtop``: a tensor of the fields' shape that takes the mass flux
        through the upper face of every cell (K17's, bit for bit), or None.  ``ftop``: a contiguous tensor
        [len(fields) x n x itot x jtot] that takes, in the order of ``fields``, what left every column through the lid in
        units of g x, or None.  ``fields`` may be empty with ``cmax`` and / or ``mtop``: the probe.  A written tensor that
        STARTS where an input or another written tensor starts is refused (ValueError); views that overlap in part are not
        detected.  One launch; more levels than ``transport_cols_per_block`` carries are refused (SPC_ERR_UNSUPPORTED)."""
        return self._les_transport_step("les_transport", _abi.LesTransportArgs, _abi.SPC_TRANSPORT_MAX_FIELDS, fields, out, u, v, hx, hy, (g, r), cmax,
                                        {"mtop": mtop, "ftop": ftop}, None, stream)

    def transport_cols_per_block(self, ktot):
        """columns of ``ktot`` levels a workgroup of K22 takes into LDS in the engine's dtype (64, 32 or 16); 0: unsupported"""
        return self._geometry("transport_cols_per_block", ktot)

    # -- K23: second-order limited flux-form transport of device-resident LES fields, one launch ----------------------------------
    @_on_engine_stream
    def les_transport2(self, fields, out, u, v, hx, hy, g, r, limiter="mc", cmax=True, mtop=None, ftop=None, stream=None):
        """``les_transport`` with a second-order face value (include/spc.h has the rule): every face adds to K22's donor flux a
        correction from the slope of its upwind cell, ``limiter`` ``"mc"`` (monotonized central: no new extremum in 1-D) or
        ``"none"`` (the unlimited slope); anything else is a ValueError.  Every argument, refusal and return value is
        ``les_transport``'s; ``cmax`` and ``mtop`` are K22's bit for bit, ``ftop`` takes the second-order lid flux, and empty
        ``fields`` are the same probe.  One launch; more levels than ``transport2_cols_per_block`` carries are refused."""
        if limiter not in _abi.LIMITERS:
            raise ValueError("les_transport2: limiter %r is none of %s" % (limiter, sorted(_abi.LIMITERS)))
        return self._les_transport_step("les_transport2", _abi.LesTransport2Args, _abi.SPC_TRANSPORT_MAX_FIELDS, fields, out, u, v, hx, hy, (g, r), cmax,
                                        {"mtop": mtop, "ftop": ftop}, _abi.LIMITERS[limiter], stream)

    def transport2_cols_per_block(self, ktot):
        """columns of ``ktot`` levels a workgroup of K23 takes into LDS in the engine's dtype (K22's: 64, 32 or 16); 0: unsupported"""
        return self._geometry("transport2_cols_per_block", ktot)

    # -- K18: longwave cooling and warming of device-resident LES fields by their liquid water, one launch ------------------------
    @_on_engine_stream
    def les_radiate(self, ql, thl, w, c, f0, f1, *, flux=None, fsfc=None, stream=None):
        """One step of the parametrised longwave flux (include/spc.h has the rule) on contiguous device fields
        [n x itot x jtot x ktot]: the liquid water ``ql`` (read only) gives the optical depths above and below every face,
        ``thl`` takes the divergence of the flux IN PLACE.  ``w`` and ``c`` [n x ktot] are ``radiation.profiles`` in the engine's
        dtype (rows may be pitched, both with one pitch), ``f0`` and ``f1`` [n] the flux scales of every LES in W/m2.  ``flux``:
        a tensor of the fields' shape that takes the flux at the upper face of every cell, or None; ``fsfc``: a tensor
        [n x itot x jtot] that takes the flux at the ground, or None.  The table of exp(-x) (``radiation.exp_table``) is
        uploaded once per engine.  A written tensor that STARTS where an input or another written tensor starts is refused
        (ValueError); views that overlap in part are not detected.  One launch; more levels than ``radiate_cols_per_block``
        carries are refused (SPC_ERR_UNSUPPORTED)."""
        from . import radiation
        shape = n, itot, jtot, ktot = self._extents("les_radiate", "ql", ql)
        if self._exp_tab is None:
            self._exp_tab = torch.from_numpy(radiation.exp_table(self.dtype)).to(self.device)
        ck = _Checker(self.device, self.dtype)
        a = _abi.LesRadiateArgs()
        a.n_les, a.itot, a.jtot, a.ktot = n, itot, jtot, ktot
        a.ql, a.thl = ql.data_ptr(), self._field4("thl", thl, shape).data_ptr()
        a.w, a.pitch_prof = ck.mat("w", w, n, ktot)
        a.c, _ = ck.mat("c", c, n, ktot, pitch=a.pitch_prof)
        a.f0, a.f1 = ck.vec("f0", f0, n), ck.vec("f1", f1, n)
        a.etab, a.n_tab, a.inv_step = self._exp_tab.data_ptr(), int(self._exp_tab.numel()), radiation.INV_STEP
        if flux is not None:
            a.flux = self._field4("flux", flux, shape).data_ptr()
        if fsfc is not None:
            a.fsfc = self._plane("les_radiate: fsfc", fsfc, (n, itot, jtot)).data_ptr()
        self._no_alias("les_radiate: thl, flux or fsfc is an input or another of them", (thl, flux, fsfc), (ql, w, c, f0, f1), n)
        self._call(self._sym("les_radiate"), ctypes.byref(a), stream=stream)

    def radiate_cols_per_block(self, ktot):
        """columns of ``ktot`` levels a workgroup of K18 takes into LDS in the engine's dtype (64, 32 or 16); 0: unsupported"""
        return self._geometry("radiate_cols_per_block", ktot)

    # -- K19: the local cloud-water forcing of device-resident LES moisture (qt_forcing 'local' | 'strong') ------------------------
    @_on_engine_stream
    def les_qt_local(self, qt, ql, a, qtm, *, count=None, split=0, stream=None):
        """The local cloud-water forcing (include/spc.h has the rule) on contiguous device fields [n x itot x jtot x ktot]:
        per LES and level the wet cells of the plane are counted (``qt > qtm`` where ``a > 0``, ``ql > 0`` where ``a < 0``) and
        ``qt`` takes ``a * N / c`` in its wet cells and gives ``a * N / (N - c)`` in its dry ones IN PLACE; levels with a zero
        or NaN ``a``, with no wet cell or with none dry keep their bits.  ``ql`` is read only.  ``a`` and ``qtm`` [n x ktot] are
        ``qt_forcing.increments`` and the slab means of ``qt`` in the engine's dtype (rows may be pitched, both with one pitch).
        Returns the int32 [n x ktot] counts (``count``: a tensor to write them into, rows may be pitched).  ``split``: 0 lets
        the library choose how many workgroups share a plane (``qt_local_split``), another value forces it; the bits do not
        depend on it.  ``qt`` STARTING where ``ql`` starts is refused (ValueError)."""
        shape = n, itot, jtot, ktot = self._extents("les_qt_local", "qt", qt)
        if int(split) < 0:
            raise ValueError("les_qt_local: split must be >= 0, got %r" % (split,))
        ck = _Checker(self.device, self.dtype)
        args = _abi.LesQtLocalArgs()
        args.n_les, args.itot, args.jtot, args.ktot, args.split = n, itot, jtot, ktot, int(split)
        args.qt, args.ql = qt.data_ptr(), self._field4("ql", ql, shape).data_ptr()
        args.a, args.pitch_prof = ck.mat("a", a, n, ktot)
        args.qtm, _ = ck.mat("qtm", qtm, n, ktot, pitch=args.pitch_prof)
        out, args.pitch_count = self._out(count, n, ktot, dtype=torch.int32)
        args.count = out.data_ptr()
        self._no_alias("les_qt_local: qt and ql are the same tensor", [qt], [ql], n)
        self._call(self._sym("les_qt_local"), ctypes.byref(args), stream=stream)
        return out

    def qt_local_split(self, n, itot, jtot, ktot):
        """workgroups that share a plane of K19 for these extents in the engine's dtype, as the library chooses; 0: bad extents"""
        return self._geometry("qt_local_split", n, itot, jtot, ktot)

    # -- K20: the second moments of device-resident LES fields (variances, covariances, resolved fluxes) ---------------------------
    @_on_engine_stream
    def les_moments(self, fields, pairs=(), mean=True, var=True, std=False, face=None, out=None, stream=None):
        """The moments per LES and level (include/spc.h has the rule) of contiguous device fields [n x itot x jtot x ktot] of ONE
        shape, in ONE launch: ``fields`` is a dict name -> tensor (at most ``_abi.MOMENTS_MAX_FIELDS``), ``pairs`` a sequence of
        ``(name, name)`` of two different fields (at most ``_abi.MOMENTS_MAX_PAIRS``), ``face`` the name of the one field that
        is given at the upper faces of the cells (K17's W; it is brought to the centres first) or None.  Returns
        ``{"mean": {name: t}, "var": {...}, "std": {...}, "cov": {(a, b): t}}`` with only the kinds asked for (``cov`` where
        there are pairs), each tensor [n x ktot]: ``numpy.mean / var / std(field[l], axis=(0, 1))`` and the mean of the product
        of the deviations of a pair, bit for bit.  ``out``: the same structure of tensors to write into (rows may be pitched,
        all with one pitch); a kind or a name that ``out`` leaves out is allocated.  A field of one level (ktot == 1) is
        refused (SPC_ERR_UNSUPPORTED)."""
        names = list(fields)
        if not 1 <= len(names) <= _abi.MOMENTS_MAX_FIELDS:
            raise ValueError("les_moments takes 1 ... %d fields per launch, got %d" % (_abi.MOMENTS_MAX_FIELDS, len(names)))
        pairs = [tuple(p) for p in pairs]
        if len(pairs) > _abi.MOMENTS_MAX_PAIRS:
            raise ValueError("les_moments takes at most %d pairs per launch, got %d" % (_abi.MOMENTS_MAX_PAIRS, len(pairs)))
        for p in pairs:
            if len(p) != 2 or p[0] not in fields or p[1] not in fields or p[0] == p[1]:
                raise ValueError("les_moments: pair %r is not two different names of fields" % (p,))
        if len(set(pairs)) != len(pairs):
            raise ValueError("les_moments: a pair is asked for twice")
        if face is not None and face not in fields:
            raise ValueError("les_moments: the face field %r is not among the fields %s" % (face, names))
        kinds = [k for k, on in (("mean", mean), ("var", var), ("std", std)) if on]
        if not kinds and not pairs:
            raise ValueError("les_moments: no output asked for")
        shape = n, itot, jtot, ktot = self._extents("les_moments", names[0], fields[names[0]])
        a = _abi.LesMomentsArgs()
        a.n_les, a.itot, a.jtot, a.ktot = n, itot, jtot, ktot
        a.n_fields, a.n_pairs, a.face_field = len(names), len(pairs), -1 if face is None else names.index(face)
        for f, name in enumerate(names):
            a.fields[f] = self._field4(name, fields[name], shape).data_ptr()
        out = out or {}
        wanted = [(kind, name) for kind in kinds for name in names] + [("cov", p) for p in pairs]
        missing = [w for w in wanted if w[1] not in out.get(w[0], {})]
        fresh = torch.empty(len(missing), n, ktot, dtype=self.dtype, device=self.device) if missing else None
        res, pitch = {}, None
        for kind, key in wanted:
            if (kind, key) in missing:
                o, p = self._out(fresh[missing.index((kind, key))], n, ktot)
            else:
                o, p = self._out(out[kind][key], n, ktot)
            pitch = self._same_pitch("les_moments: out[%s][%s]" % (kind, key), p, pitch, n)
            res.setdefault(kind, {})[key] = o
            if kind == "cov":
                q = pairs.index(key)
                a.pair_a[q], a.pair_b[q] = names.index(key[0]), names.index(key[1])
                a.cov[q] = o.data_ptr()
            else:
                getattr(a, kind)[names.index(key)] = o.data_ptr()
        a.pitch_out = pitch
        self._call(self._sym("les_moments"), ctypes.byref(a), stream=stream)
        return res

    # -- K21: the hydrostatic pressure force of device-resident LES fields on their winds, two launches ---------------------------
    @_on_engine_stream
    def les_buoyancy(self, thl, qt, ql, u, v, hx, hy, t0, lex, s, phi, psfc=None, amax=True, stream=None):
        """The hydrostatic pressure force (include/spc.h has the rule) on contiguous device fields [n x itot x jtot x ktot]:
        the buoyancy of ``thl``, ``qt`` and ``ql`` (read only; ``ql`` may be None: no liquid water) against ``t0`` is integrated
        downward from the lid into ``phi`` (written whole), and ``u`` and ``v`` take the horizontal gradient of ``phi`` IN
        PLACE.  ``hx`` and ``hy`` [n] are ``advection.coefficients``, ``t0``, ``lex`` and ``s`` [n x ktot]
        ``buoyancy.profiles`` in the engine's dtype (rows may be pitched, all with one pitch).  ``psfc``: a tensor
        [n x itot x jtot] that takes the pressure perturbation at the ground, or None.  ``amax``: True (a fresh [n] tensor),
        a tensor [n] to write into, or False / None; returned: the largest wind change |du| + |dv| of every LES (a NaN where
        any cell's is one), or None.  A written tensor that STARTS where an input or another written tensor starts is refused
        (ValueError); views that overlap in part are not detected.  Two launches; more levels than
        ``buoyancy_cols_per_block`` carries are refused (SPC_ERR_UNSUPPORTED)."""
        from . import buoyancy
        shape = n, itot, jtot, ktot = self._extents("les_buoyancy", "thl", thl)
        ck = _Checker(self.device, self.dtype)
        a = _abi.LesBuoyancyArgs()
        a.n_les, a.itot, a.jtot, a.ktot = n, itot, jtot, ktot
        a.thl, a.qt = thl.data_ptr(), self._field4("qt", qt, shape).data_ptr()
        if ql is not None:
            a.ql = self._field4("ql", ql, shape).data_ptr()
        a.u, a.v = self._field4("u", u, shape).data_ptr(), self._field4("v", v, shape).data_ptr()
        a.hx, a.hy = ck.vec("hx", hx, n), ck.vec("hy", hy, n)
        a.t0, a.pitch_prof = ck.mat("t0", t0, n, ktot)
        a.lex, _ = ck.mat("lex", lex, n, ktot, pitch=a.pitch_prof)
        a.s, _ = ck.mat("s", s, n, ktot, pitch=a.pitch_prof)
        a.c1, a.c2 = buoyancy.C1, buoyancy.C2
        a.phi = self._field4("phi", phi, shape).data_ptr()
        if psfc is not None:
            a.psfc = self._plane("les_buoyancy: psfc", psfc, (n, itot, jtot)).data_ptr()
        res = self._largest(ck, "amax", amax, n)
        if res is not None:
            a.amax = res.data_ptr()
        self._no_alias("les_buoyancy: phi, u, v, psfc or amax is an input or another of them", (phi, u, v, psfc, res),
                       (thl, qt, ql, hx, hy, t0, lex, s), n)
        self._call(self._sym("les_buoyancy"), ctypes.byref(a), stream=stream)
        return res

    def buoyancy_cols_per_block(self, ktot):
        """columns of ``ktot`` levels a workgroup of K21's k_les_hydrostatic takes into LDS in the engine's dtype (64, 32 or 16);
        0: unsupported"""
        return self._geometry("buoyancy_cols_per_block", ktot)

    # -- K24: the Smagorinsky-Lilly subgrid mixing of device-resident LES fields, two launches --------------------------------------
    @_on_engine_stream
    def les_mix(self, fields, out, u, v, theta, gx, gy, gz, bz, l2, kcap, km, ax, ay, kmax=True, stream=None):
        """The Smagorinsky-Lilly closure (include/spc.h has the rule) on contiguous device fields [n x itot x jtot x ktot]: the
        eddy viscosity of the winds ``u`` and ``v`` and of ``theta`` (read only; ``theta`` may be None: no stratification
        term, ``bz`` may then be None too) is written whole into ``km``, and every tensor of ``fields`` (dict name -> tensor, at
        most ``_abi.SPC_MIX_MAX_FIELDS`` of one shape, read only; a field may be ``u``, ``v`` or ``theta`` itself) is mixed
        along i and j by it into the tensors of ``out`` (the same names, written whole).  ``gx``, ``gy`` and ``kcap`` [n] and
        ``gz``, ``bz`` and ``l2`` [n x ktot] are ``mixing.coefficients`` / ``cap`` / ``profiles`` in the engine's dtype (rows may be
        pitched, all with one pitch); ``ax`` and ``ay`` are dicts name -> [n] with the names of ``fields`` (fields may share a
        tensor).  ``kmax``: True (a fresh [n] tensor), a tensor [n] to write into, or False / None; returned: the largest
        uncapped viscosity of every LES, or None.  ``fields`` may be empty: the probe / the diagnostic, one launch.  A written
        tensor that STARTS where an input or another written tensor starts is refused (ValueError); views that overlap in part
        are not detected.  Two launches."""
        names = list(fields)
        if len(names) > _abi.SPC_MIX_MAX_FIELDS:
            raise ValueError("les_mix takes at most %d fields per launch, got %d" % (_abi.SPC_MIX_MAX_FIELDS, len(names)))
        for what, d in (("out", out), ("ax", ax), ("ay", ay)):
            if sorted(d) != sorted(names):
                raise ValueError("les_mix: %s holds %s, the fields are %s" % (what, sorted(d), sorted(names)))
        if theta is not None and bz is None:
            raise ValueError("les_mix: theta without bz")
        shape = n, itot, jtot, ktot = self._extents("les_mix", "u", u)
        ck = _Checker(self.device, self.dtype)
        a = _abi.LesMixArgs()
        a.n_les, a.itot, a.jtot, a.ktot, a.n_fields = n, itot, jtot, ktot, len(names)
        a.u, a.v = u.data_ptr(), self._field4("v", v, shape).data_ptr()
        if theta is not None:
            a.theta = self._field4("theta", theta, shape).data_ptr()
        a.gx, a.gy, a.kcap = ck.vec("gx", gx, n), ck.vec("gy", gy, n), ck.vec("kcap", kcap, n)
        a.gz, a.pitch_prof = ck.mat("gz", gz, n, ktot)
        if bz is not None:
            a.bz, _ = ck.mat("bz", bz, n, ktot, pitch=a.pitch_prof)
        a.l2, _ = ck.mat("l2", l2, n, ktot, pitch=a.pitch_prof)
        a.km = self._field4("km", km, shape).data_ptr()
        res = self._largest(ck, "kmax", kmax, n)
        if res is not None:
            a.kmax = res.data_ptr()
        for f, k in enumerate(names):
            a.fields[f] = self._field4(k, fields[k], shape).data_ptr()
            a.out[f] = self._field4("out[%s]" % k, out[k], shape).data_ptr()
            a.ax[f], a.ay[f] = ck.vec("ax[%s]" % k, ax[k], n), ck.vec("ay[%s]" % k, ay[k], n)
        self._no_alias("les_mix: km, kmax or an output is an input or another of them", [km, res] + [out[k] for k in names],
                       [u, v, theta, gx, gy, kcap, gz, bz if theta is not None else None, l2] + [fields[k] for k in names]
                       + [ax[k] for k in names] + [ay[k] for k in names], n)
        self._call(self._sym("les_mix"), ctypes.byref(a), stream=stream)
        return res

    # -- K25: implicit vertical mixing of device-resident LES fields by each column's own eddy viscosity, two launches ---------------
    @_on_engine_stream
    def les_vmix(self, fields, km, el, eu, kb, kv2, s0=None, flux=None, drag=None, u=None, v=None, speed=None, stream=None):
        """One backward-Euler step of the vertical mixing (include/spc.h has the rule) IN PLACE on every tensor of ``fields``
        (dict name -> contiguous [n x itot x jtot x ktot], at most ``_abi.SPC_VMIX_MAX_FIELDS`` of one shape) by the eddy
        viscosity ``km`` (the same shape, read only).  ``el`` and ``eu`` are dicts name -> [n x ktot] with the names of
        ``fields`` (fields may share a tensor), ``kb`` [n x ktot] and ``kv2``, ``s0`` [n] are ``vertical_mixing``'s arrays in the
        engine's dtype (rows may be pitched, all with one pitch).  ``flux``: dict name -> [n], the kinematic surface flux that
        enters level 0 of that field (needs ``s0``).  ``drag``: dict name -> [n], ``vertical_mixing.drag`` of that wind; it
        needs the winds ``u`` and ``v`` (which may be fields) and the plane ``speed`` [n x itot x jtot], which is written whole
        with the speed of the lowest level BEFORE any field changes.  A field that STARTS where another field, ``km``,
        ``speed``, a profile, a flux or a drag starts is refused (ValueError); views that overlap in part are not detected.  Two
        launches (one without a drag); more levels than ``vmix_cols_per_block`` carries are refused (SPC_ERR_UNSUPPORTED)."""
        names = list(fields)
        if not 1 <= len(names) <= _abi.SPC_VMIX_MAX_FIELDS:
            raise ValueError("les_vmix takes 1 ... %d fields per launch, got %d" % (_abi.SPC_VMIX_MAX_FIELDS, len(names)))
        for what, d in (("el", el), ("eu", eu)):
            if sorted(d) != sorted(names):
                raise ValueError("les_vmix: %s holds %s, the fields are %s" % (what, sorted(d), sorted(names)))
        flux = {} if flux is None else {k: t for k, t in flux.items() if t is not None}
        drag = {} if drag is None else {k: t for k, t in drag.items() if t is not None}
        for what, d in (("fluxes", flux), ("drags", drag)):
            unknown = [k for k in d if k not in fields]
            if unknown:
                raise ValueError("les_vmix: %s %s have no field" % (what, unknown))
        if flux and s0 is None:
            raise ValueError("les_vmix: a flux needs s0")
        if drag and (u is None or v is None or speed is None):
            raise ValueError("les_vmix: a drag needs u, v and speed")
        shape = n, itot, jtot, ktot = self._extents("les_vmix", names[0], fields[names[0]])
        ck = _Checker(self.device, self.dtype)
        g = _abi.LesVmixArgs()
        g.n_les, g.itot, g.jtot, g.ktot, g.n_fields = n, itot, jtot, ktot, len(names)
        g.km = self._field4("km", km, shape).data_ptr()
        g.kb, g.pitch_prof = ck.mat("kb", kb, n, ktot)
        g.kv2 = ck.vec("kv2", kv2, n)
        read = [km, kb, kv2]
        if s0 is not None:
            g.s0 = ck.vec("s0", s0, n)
            read.append(s0)
        written = [fields[k] for k in names]
        if drag:
            g.u, g.v = self._field4("u", u, shape).data_ptr(), self._field4("v", v, shape).data_ptr()
            g.speed = self._plane("speed", speed, shape[:3]).data_ptr()
            self._no_alias("les_vmix: speed is an input", [speed], [u, v], n)
            written.append(speed)
        for f, name in enumerate(names):
            g.fields[f] = self._field4(name, fields[name], shape).data_ptr()
            g.el[f], _ = ck.mat("el[%s]" % name, el[name], n, ktot, pitch=g.pitch_prof)
            g.eu[f], _ = ck.mat("eu[%s]" % name, eu[name], n, ktot, pitch=g.pitch_prof)
            read += [el[name], eu[name]]
            if name in flux:
                g.flux[f] = ck.vec("flux[%s]" % name, flux[name], n)
                read.append(flux[name])
            if name in drag:
                g.dr[f] = ck.vec("drag[%s]" % name, drag[name], n)
                read.append(drag[name])
        self._no_alias("les_vmix: a field or speed is another field, km, a profile, s0, a flux or a drag", written, read, n)
        self._call(self._sym("les_vmix"), ctypes.byref(g), stream=stream)

    def vmix_cols_per_block(self, ktot):
        """columns of ``ktot`` levels a workgroup of K25's k_les_vmix takes into LDS in the engine's dtype (64, 32 or 16);
        0: unsupported"""
        return self._geometry("vmix_cols_per_block", ktot)

    # -- K26: implicit horizontal mixing of device-resident LES fields by each line's own eddy viscosity, two launches ---------------
    @_on_engine_stream
    def les_hmix(self, fields, km, ax, ay, kh2, axes=3, stream=None):
        """One backward-Euler step of the horizontal mixing (include/spc.h has the rule) IN PLACE on every tensor of ``fields``
        (dict name -> contiguous [n x itot x jtot x ktot], at most ``_abi.SPC_HMIX_MAX_FIELDS`` of one shape) by the eddy
        viscosity ``km`` (the same shape, read only): every periodic line along i, then every line along j.  ``ax`` and ``ay``
        are dicts name -> [n] with the names of ``fields`` (``mixing.coefficients``; fields may share a tensor) and ``kh2`` [n]
        is ``horizontal_mixing.bound`` in the engine's dtype.  ``axes``: 1 the sweep along i alone, 2 the sweep along j alone, 3
        both.  A field that STARTS where another field, ``km``, ``kh2`` or a coefficient starts is refused (ValueError); views
        that overlap in part are not detected.  Two launches; longer lines than ``hmix_lines_per_block`` carries are refused
        (SPC_ERR_UNSUPPORTED)."""
        names = list(fields)
        if not 1 <= len(names) <= _abi.SPC_HMIX_MAX_FIELDS:
            raise ValueError("les_hmix takes 1 ... %d fields per launch, got %d" % (_abi.SPC_HMIX_MAX_FIELDS, len(names)))
        for what, d in (("ax", ax), ("ay", ay)):
            if sorted(d) != sorted(names):
                raise ValueError("les_hmix: %s holds %s, the fields are %s" % (what, sorted(d), sorted(names)))
        if axes not in (1, 2, 3):
            raise ValueError("les_hmix: axes %r is none of 1 (along i), 2 (along j) and 3 (both)" % (axes,))
        shape = n, itot, jtot, ktot = self._extents("les_hmix", names[0], fields[names[0]])
        ck = _Checker(self.device, self.dtype)
        g = _abi.LesHmixArgs()
        g.n_les, g.itot, g.jtot, g.ktot, g.n_fields, g.axes = n, itot, jtot, ktot, len(names), axes
        g.km = self._field4("km", km, shape).data_ptr()
        g.kh2 = ck.vec("kh2", kh2, n)
        read = [km, kh2]
        for f, name in enumerate(names):
            g.fields[f] = self._field4(name, fields[name], shape).data_ptr()
            g.ax[f], g.ay[f] = ck.vec("ax[%s]" % name, ax[name], n), ck.vec("ay[%s]" % name, ay[name], n)
            read += [ax[name], ay[name]]
        self._no_alias("les_hmix: a field is another field, km, kh2 or a coefficient", [fields[k] for k in names], read, n)
        self._call(self._sym("les_hmix"), ctypes.byref(g), stream=stream)

    def hmix_lines_per_block(self, n):
        """lines of ``n`` cells a workgroup of K26's k_les_hline takes in the engine's dtype (256 ... 16); 0: unsupported"""
        return self._geometry("hmix_lines_per_block", n)

    # -- K7: the helpers of splib/sputils.py as batched operators (sp_coupler_amd/sputils.py keeps their names) -------
    # Each operator has a ``plan_*`` form (arguments checked and the C argument block frozen ONCE, output allocated once
    # or taken from ``out=``: ``plan.run()`` is then one foreign call, no allocation) and a convenience form that builds
    # the plan and runs it.  Arguments are read IN PLACE when they are contiguous along their rows; anything else (a
    # transposed view, a shared fp of interp, q / rho of different pitch) goes through a private packed copy that run()
    # refreshes from the caller's tensor before every launch -- a plan never serves a stale snapshot.
    def _rows(self, name, t, n_rows=None, shared_ok=False, refresh=None):
        """(tensor, data_ptr, pitch, n): a [n_rows x n] matrix contiguous along n (pitch = row stride), or -- where the
        operator allows it -- ONE [n] row shared by all rows (pitch 0).  A tensor the kernels cannot read in place is
        copied; the (copy, original) pair is appended to ``refresh`` so that a plan can redo the copy before every run."""
        orig = t
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if t.device != self.device or t.dtype != self.dtype:
            raise ValueError("%s must be %s on %s (got %s on %s)" % (name, self.dtype, self.device, t.dtype, t.device))
        if t.dim() == 1:
            if not shared_ok and n_rows not in (None, 1):
                raise ValueError("%s must have %d rows, got one" % (name, n_rows))
            t = t.contiguous()
            if refresh is not None and t is not orig:
                refresh.append((t, orig))
            return t, t.data_ptr(), (0 if shared_ok and n_rows not in (None, 1) else max(1, t.shape[0])), int(t.shape[0])
        if t.dim() != 2:
            raise ValueError("%s must be [n] or [n_rows x n], got %s" % (name, tuple(t.shape)))
        if n_rows is not None and t.shape[0] != n_rows:
            raise ValueError("%s must have %d rows, got %d" % (name, n_rows, t.shape[0]))
        if t.shape[1] > 1 and t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            t = t.contiguous()
            if refresh is not None:
                refresh.append((t, orig))
        return t, t.data_ptr(), (int(t.stride(0)) if t.shape[0] > 1 else max(1, int(t.shape[1]))), int(t.shape[1])

    def _out(self, out, n_rows, n, dtype=None):
        """the operator's [n_rows x n] result: the caller's ``out`` (checked; may be [n] when n_rows == 1, may be pitched)
        or a fresh tensor.  Returns (2-D tensor, pitch)."""
        dtype = dtype or self.dtype
        if out is None:
            out = torch.empty(n_rows, n, dtype=dtype, device=self.device)
        else:
            if not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != dtype:
                raise ValueError("out must be a %s tensor on %s" % (dtype, self.device))
            if out.dim() == 1 and n_rows == 1:
                out = out.unsqueeze(0)
            if tuple(out.shape) != (n_rows, n) or (n > 1 and out.stride(1) != 1) or (n_rows > 1 and out.stride(0) < n):
                raise ValueError("out must be [%d x %d], contiguous along its rows, got %s (strides %s)"
                                 % (n_rows, n, tuple(out.shape), out.stride()))
        return out, (int(out.stride(0)) if n_rows > 1 else max(1, n))

    def _call(self, fn, *args, stream=None):
        with torch.cuda.device(self.device):
            rc = fn(*args, _stream_ptr(stream if stream is not None else self.stream, self.device))
        _abi.check(self.lib, rc)

    @_on_engine_stream
    def plan_exner(self, p, inverse=False, out=None):
        """sputils.exner / iexner (splib/sputils.py:28-34), elementwise on a device tensor of any shape"""
        if p.device != self.device or p.dtype != self.dtype:
            raise ValueError("p must be %s on %s" % (self.dtype, self.device))
        refresh = []
        if not p.is_contiguous():
            src, p = p, p.contiguous()
            refresh.append((p, src))
        if out is None:
            out = torch.empty_like(p)
        elif not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != self.dtype or out.shape != p.shape or not out.is_contiguous():
            raise ValueError("out must be a contiguous %s tensor of shape %s on %s" % (self.dtype, tuple(p.shape), self.device))
        fn = self._sym("exner")
        return OperatorPlan(self, fn, (p.numel(), p.data_ptr(), out.data_ptr(), 1 if inverse else 0), [p, out], {"out": out}, result=out,
                            refresh=refresh)

    def exner(self, p, inverse=False, stream=None, out=None):
        return self.plan_exner(p, inverse, out=out).run(stream)

    @_on_engine_stream
    def plan_interp(self, x, xp, fp, out=None):
        """sputils.interp == numpy.interp (splib/sputils.py:82-86) for every row: fp [n_rows x n_xp] (or [n_xp]), xp the
        same shape or one shared [n_xp], x [n_rows x n_x] or one shared [n_x].  Result [n_rows x n_x] ([n_x] when every
        argument is 1-D)."""
        one = fp.dim() == 1 and xp.dim() == 1 and x.dim() == 1
        n_rows = max(int(t.shape[0]) if t.dim() == 2 else 1 for t in (x, xp, fp))
        refresh = []
        if fp.dim() == 1 and n_rows > 1:          # the ABI has one fp row per result row: a shared fp is spread (and re-spread per run)
            fp2 = fp.unsqueeze(0).expand(n_rows, -1).contiguous()
            refresh.append((fp2, fp.unsqueeze(0)))
        else:
            fp2 = fp
        fp2, p_fp, pitch_fp, n_xp = self._rows("fp", fp2, n_rows, refresh=refresh)
        xp2, p_xp, pitch_xp, n_xp2 = self._rows("xp", xp, n_rows, shared_ok=True, refresh=refresh)
        x2, p_x, pitch_x, n_x = self._rows("x", x, n_rows, shared_ok=True, refresh=refresh)
        if n_xp2 != n_xp:
            raise ValueError("fp and xp are not of the same length")          # numpy.interp's message
        out, pitch_out = self._out(out, n_rows, n_x)
        a = _abi.InterpArgs(n_rows, n_x, n_xp, pitch_x, pitch_xp, pitch_fp, pitch_out, p_x, p_xp, p_fp, out.data_ptr())
        fn = self._sym("interp")
        return OperatorPlan(self, fn, (ctypes.byref(a),), [fp2, xp2, x2, out, a], {"out": out}, result=out[0] if one else out, refresh=refresh)

    def interp(self, x, xp, fp, stream=None, out=None):
        return self.plan_interp(x, xp, fp, out=out).run(stream)

    @_on_engine_stream
    def plan_searchsorted(self, a, v, side="left", out=None):
        """sputils.searchsorted == numpy.searchsorted (splib/sputils.py:88-91) per row; int64 indices"""
        if side not in ("left", "right"):
            raise ValueError("side must be 'left' or 'right'")
        one = a.dim() == 1 and v.dim() == 1
        n_rows = max(int(t.shape[0]) if t.dim() == 2 else 1 for t in (a, v))
        refresh = []
        a2, p_a, pitch_a, n_a = self._rows("a", a, n_rows, shared_ok=True, refresh=refresh)
        v2, p_v, pitch_v, n_v = self._rows("v", v, n_rows, shared_ok=True, refresh=refresh)
        out, pitch_out = self._out(out, n_rows, n_v, dtype=torch.int64)
        args = _abi.SearchsortedArgs(n_rows, n_a, n_v, pitch_a, pitch_v, pitch_out, p_a, p_v, out.data_ptr(), 1 if side == "right" else 0, 0)
        fn = self._sym("searchsorted")
        return OperatorPlan(self, fn, (ctypes.byref(args),), [a2, v2, out, args], {"out": out}, result=out[0] if one else out, refresh=refresh)

    def searchsorted(self, a, v, side="left", stream=None, out=None):
        return self.plan_searchsorted(a, v, side, out=out).run(stream)

    @_on_engine_stream
    def plan_interp_c(self, Zh, zh, q, rho=None, mode="interp_c", out=None):
        """sputils.interp_c / interp_rho / integral (splib/sputils.py:94-197) per row: Zh [n_rows x (nG+1)] layer bounds, zh
        [nL] (shared) or [n_rows x nL] grid points, q (and rho) [n_rows x nL'] with nL' >= nL - 1 cell values.
        mode 'interp_c' (rho required), 'interp_rho' (q is the density), 'integral' (rho optional)."""
        modes = {"interp_c": 0, "interp_rho": 1, "integral": 2}
        if mode not in modes:
            raise ValueError("mode must be one of %s" % sorted(modes))
        one = Zh.dim() == 1 and q.dim() == 1
        n_rows = max(int(t.shape[0]) if t.dim() == 2 else 1 for t in (Zh, q))
        refresh = []
        Zh2, p_Zh, pitch_Zh, nGh = self._rows("Zh", Zh, n_rows, refresh=refresh)
        zh2, p_zh, pitch_zh, nL = self._rows("zh", zh, n_rows, shared_ok=True, refresh=refresh)
        q2, p_q, pitch_q, nq = self._rows("q", q, n_rows, refresh=refresh)
        if nq < nL - 1:
            raise ValueError("q has %d values, the %d grid points of zh bound %d cells" % (nq, nL, nL - 1))
        p_rho, rho2 = None, None
        if rho is not None and mode != "interp_rho":
            rho2, p_rho, pitch_rho, nr = self._rows("rho", rho, n_rows, refresh=refresh)
            if nr != nq:
                raise ValueError("rho and q must have the same shape")
            if n_rows > 1 and pitch_rho != pitch_q:            # the ABI has ONE pitch for q and rho: both packed (and re-packed per run)
                refresh[:] = [pr for pr in refresh if pr[0] is not rho2 and pr[0] is not q2]
                rho2, q2 = rho.contiguous(), q.contiguous()
                if rho2 is rho:
                    rho2 = rho.clone()
                if q2 is q:
                    q2 = q.clone()
                refresh += [(rho2, rho), (q2, q)]
                p_rho, p_q, pitch_q = rho2.data_ptr(), q2.data_ptr(), max(1, nq)
        elif mode == "interp_c":
            raise ValueError("interp_c needs the weights rho")
        nG = nGh - 1
        out, pitch_out = self._out(out, n_rows, max(nG, 0))
        a = _abi.InterpCArgs(n_rows, nG, nL, pitch_Zh, pitch_zh, pitch_q, pitch_out, p_Zh, p_zh, p_q, p_rho, out.data_ptr(), modes[mode], 0)
        fn = self._sym("interp_c")
        return OperatorPlan(self, fn, (ctypes.byref(a),), [Zh2, zh2, q2, rho2, out, a], {"out": out}, result=out[0] if one else out, refresh=refresh)

    def interp_c(self, Zh, zh, q, rho=None, mode="interp_c", stream=None, out=None):
        return self.plan_interp_c(Zh, zh, q, rho, mode, out=out).run(stream)

    @_on_engine_stream
    def plan_rms(self, a, out=None):
        """sputils.rms (splib/sputils.py:23-24) of every row of a [n_rows x n] tensor (of the one row of a 1-D tensor)"""
        one = a.dim() == 1
        refresh = []
        a2, p_a, pitch, n = self._rows("a", a, refresh=refresh)
        n_rows = 1 if one else int(a2.shape[0])
        if out is None:
            out = self.empty(n_rows)
        elif not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != self.dtype or tuple(out.shape) != (n_rows,) \
                or not out.is_contiguous():
            raise ValueError("out must be a contiguous %s vector of %d on %s" % (self.dtype, n_rows, self.device))
        fn = self._sym("rms")
        return OperatorPlan(self, fn, (n_rows, n, max(pitch, n), p_a, out.data_ptr()), [a2, out], {"out": out}, result=out[0] if one else out,
                            refresh=refresh)

    def rms(self, a, stream=None, out=None):
        return self.plan_rms(a, out=out).run(stream)

    # -- surface fluxes of columns without an LES -------------------------------------------------
    @_on_engine_stream
    def plan_surface_fluxes(self, Ph_s, T_s, QLflux, QIflux, SHflux, TSflux, out=None):
        """(wthl, wqt) of spcpl.convert_surface_fluxes (splib/spcpl.py:153-161) for [n] scalars."""
        n = int(Ph_s.shape[0])
        ck = _Checker(self.device, self.dtype)
        ptrs = [ck.vec(nm, t, n) for nm, t in (("Ph_s", Ph_s), ("T_s", T_s), ("QLflux", QLflux), ("QIflux", QIflux),
                                               ("SHflux", SHflux), ("TSflux", TSflux))]
        out = dict(out or {})
        wthl = out["wthl"] if "wthl" in out else self.empty(n)
        wqt = out["wqt"] if "wqt" in out else self.empty(n)
        optr = [ck.vec("wthl", wthl, n), ck.vec("wqt", wqt, n)]
        fn = self._sym("surface_fluxes")
        return SurfacePlan(self, fn, [n] + ptrs + optr, ck.keep, {"wthl": wthl, "wqt": wqt})

    @_on_engine_stream
    def surface_fluxes(self, Ph_s, T_s, QLflux, QIflux, SHflux, TSflux, stream=None):
        r = self.plan_surface_fluxes(Ph_s, T_s, QLflux, QIflux, SHflux, TSflux).launch(stream)
        return r["wthl"], r["wqt"]

    # -- K8: the geometry of sputils.get_mask_indices (splib/sputils.py:46-73); float64 on every engine ---------------
    def _vector(self, name, t, n=None, dtype=torch.float64):
        """``t`` as a contiguous 1-D ``dtype`` tensor on the engine's device (converted / copied where it is not one)"""
        t = torch.as_tensor(t, dtype=dtype)
        if t.dim() != 1 or (n is not None and t.shape[0] != n):
            raise ValueError("%s must be a vector%s, got %s" % (name, "" if n is None else " of %d" % n, tuple(t.shape)))
        return t.to(device=self.device, dtype=dtype).contiguous()

    @_on_engine_stream
    def point_in_polygon(self, lon, lat, vx, vy, ring_start, ring_role, ring_poly, n_polys=None, stream=None):
        """Location (include/spc.h SPC_LOC_*) of every grid point (lon[i], lat[i]) and of its image
        ((lon - 180) % 360 - 180, lat) in every polygon: a uint8 tensor [n_polys x n x 2] ([..., 0] the point, [..., 1] its
        image).  Rings: vertices vx / vy concatenated, ring r = vx[ring_start[r]:ring_start[r+1]], closed, grouped by
        polygon (ring_poly non-decreasing, shell first); ring_role SPC_RING_SHELL / _HOLE / _RECTANGLE.  float64 whatever
        the engine's dtype: an fp32 engine takes the same decisions."""
        lon = self._vector("lon", lon)
        n = int(lon.shape[0])
        lat = self._vector("lat", lat, n)
        vx = self._vector("vx", vx)
        nv = int(vx.shape[0])
        vy = self._vector("vy", vy, nv)
        ring_role = self._vector("ring_role", ring_role, dtype=torch.int32)
        nr = int(ring_role.shape[0])
        ring_start = self._vector("ring_start", ring_start, nr + 1, dtype=torch.int64)
        ring_poly = self._vector("ring_poly", ring_poly, nr, dtype=torch.int32)
        if n_polys is None:
            n_polys = int(ring_poly.max()) + 1 if nr else 0
        out = torch.zeros(n_polys, n, 2, dtype=torch.uint8, device=self.device)
        a = _abi.PipArgs(n, nv, nr, n_polys, lon.data_ptr(), lat.data_ptr(), vx.data_ptr(), vy.data_ptr(), ring_start.data_ptr(),
                         ring_role.data_ptr(), ring_poly.data_ptr(), out.data_ptr())
        self._call(self.lib.spc_point_in_polygon_f64, ctypes.byref(a), stream=stream)
        return out

    @_on_engine_stream
    def haversine(self, lon, lat, lon0, lat0, stream=None):
        """great-circle distance in km of every (lon[i], lat[i]) to (lon0, lat0), splib/haversine.py:12-36; float64"""
        lon = self._vector("lon", lon)
        n = int(lon.shape[0])
        lat = self._vector("lat", lat, n)
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        self._call(self.lib.spc_haversine_f64, n, lon.data_ptr(), lat.data_ptr(), float(lon0), float(lat0), out.data_ptr(), stream=stream)
        return out

    # -- K9: the initial LES state of spcpl.set_les_state (splib/spcpl.py:274-294); float64 on every engine ---------------
    @_on_engine_stream
    def les_state(self, shapes, u, v, thl, qt, state, amps=LES_STATE_AMPS, gens_per_substream=0, stream=None):
        """``amp[f] * numpy.random.uniform(-1., 1., (itot, jtot, ktot)) + profile`` for the fields U, V, THL, QT of every LES
        in list order, drawn from NumPy's legacy MT19937 state ``state`` ((key, pos) or what ``numpy.random.get_state()``
        returns) as the reference loop draws them, bit for bit.  ``shapes``: (itot, jtot, ktot) per LES; ``u`` ... ``qt``:
        profiles [n x >= ktot] (device tensors or host arrays, any float type: promoted to float64 exactly).  Returns
        (fields, (key, pos)): fields[name] a float64 tensor [n x itot x jtot x ktot] on this device when all LES have one
        shape, else a list of n tensors; (key, pos) the state NumPy holds after the same draws.  The call returns once the
        launch has finished (the state comes back to the host)."""
        import numpy
        n = len(shapes)
        sizes = [int(i) * int(j) * int(k) for i, j, k in shapes]
        ktot = numpy.array([int(s[2]) for s in shapes], dtype=numpy.int32)
        elem_off = numpy.zeros(n + 1, dtype=numpy.int64)
        numpy.cumsum(sizes, out=elem_off[1:])
        key, pos = (state[1], state[2]) if len(state) == 5 else state
        key = numpy.ascontiguousarray(key, dtype=numpy.uint32)
        if key.shape != (_abi.MT_N,):
            raise ValueError("MT19937 key must hold 624 words, got %s" % (key.shape,))
        prof = []
        for name, p in (("u", u), ("v", v), ("thl", thl), ("qt", qt)):
            t = torch.as_tensor(p).to(device=self.device, dtype=torch.float64)
            if t.dim() != 2 or t.shape[0] != n or (n and t.shape[1] < int(ktot.max())):
                raise ValueError("%s must be [%d x >= %d], got %s" % (name, n, int(ktot.max()) if n else 0, tuple(t.shape)))
            prof.append(t.contiguous())
        pitch = int(prof[0].shape[1]) if n else 1
        if any(int(p.shape[1]) != pitch for p in prof):
            raise ValueError("the four profiles must have one level count")
        total = int(elem_off[-1])
        flat = [torch.empty(max(total, 1), dtype=torch.float64, device=self.device) for _ in range(4)]
        wb = int(self.lib.spc_les_state_workspace_bytes(n, total, int(pos), int(gens_per_substream)))
        if wb < 0:
            _abi.check(self.lib, wb)
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.device)
        key_out = numpy.empty(_abi.MT_N, dtype=numpy.uint32)
        pos_out = ctypes.c_int32()
        a = _abi.LesStateArgs()
        a.n_les, a.elem_off, a.ktot, a.pitch_prof = n, elem_off.ctypes.data, ktot.ctypes.data, pitch
        for f in range(4):
            a.prof[f], a.out[f], a.amp[f] = prof[f].data_ptr(), flat[f].data_ptr(), float(amps[f])
        a.key_in, a.pos_in, a.key_out = key.ctypes.data, int(pos), key_out.ctypes.data
        a.pos_out = ctypes.cast(ctypes.byref(pos_out), ctypes.c_void_p)
        a.gens_per_substream, a.work, a.work_bytes = int(gens_per_substream), work.data_ptr(), wb
        self._call(self.lib.spc_les_state_f64, ctypes.byref(a), stream=stream)
        fields = {}
        uniform = len(set(tuple(int(x) for x in s) for s in shapes)) <= 1
        for name, t in zip(LES_STATE_FIELDS, flat):
            if uniform and n:
                fields[name] = t[:total].view(n, *[int(x) for x in shapes[0]])
            else:
                fields[name] = [t[elem_off[l]:elem_off[l + 1]].view(*[int(x) for x in shapes[l]]) for l in range(n)]
        return fields, (key_out, int(pos_out.value))
