"""The helpers of ``splib/sputils.py`` on the GPU, under the reference's names.

``exner``, ``iexner`` (sputils.py:28-34), ``interp`` (:82-86), ``searchsorted`` (:88-91), ``integral`` (:94-161),
``interp_c`` (:173-189), ``interp_rho`` (:191-197) and ``rms`` (:23-24) take what the reference's functions take -- one
column as 1-D arrays (NumPy, or AMUSE quantities: ``.number`` is used, every unit of this path is SI-coherent) -- and,
beyond the reference, whole batches ``[n_cols x n_lev]`` in one call.  The arithmetic runs in the K7 kernels of
``libspc_hip.so`` (``include/spc.h``: ``spc_exner_*``, ``spc_interp_*``, ``spc_searchsorted_*``, ``spc_interp_c_*``,
``spc_rms_*``) on the engine of ``spcpl.get_engine()``; there is no CPU path here.  NumPy in -> NumPy out (one upload, one
download); device tensors in -> device tensors out (no transfer).  Results equal NumPy's bit for bit, except
``exner`` / ``iexner`` (own ``pow``: <= 2 ulp of ``numpy.power``).

The fused step kernels (K1 / K3 / K4) contain the same arithmetic and do not call these; they serve callers that use a
helper on its own.

``get_mask_indices`` (sputils.py:46-73), the column selection of ``splib.initialize``, runs on the K8 kernels
(``spc_point_in_polygon_f64``, ``spc_haversine_f64``) in float64 on any engine, with the masks of
``sp_coupler_amd.geometry`` (shapely's ``Point`` / ``Polygon`` / ``box`` / ``shape``) or shapely's own objects; shapely
itself is not needed.  ``find_closest_points`` is plain host code.  ``link_dir`` (file system, start-up) is out of scope
(DESIGN.md section 7).
"""
import numpy
import torch

from .transfer import Sharded

# Physical constants, splib/sputils.py:14-20 (plain numbers: SI-coherent units, factor 1)
pref0 = 1e5       # Pa reference pressure
rd = 287.04       # J/kg/K gas constant for dry air
rv = 461.5        # J/kg/K gas constant for water vapor
cp = 1004.        # J/kg/K specific heat at constant pressure (dry air)
rlv = 2.53e6      # J/kg latent heat for vaporisation
grav = 9.81       # m/s^2 gravity acceleration
mair = 28.967     # g/mol molar mass of air


def _engine():
    from . import spcpl
    return spcpl.get_engine()


def _num(a, unit=None):
    """bare numbers of a (possibly unit-carrying) value; with ``unit`` (the unit of ANOTHER argument the reference
    converts to: ``xp.value_in(x.unit)``, splib/sputils.py:86, 91) a quantity is converted, so that mixed units
    (km against m) give the reference's numbers instead of silently wrong ones"""
    if unit is not None and hasattr(a, "value_in"):
        return a.value_in(unit)
    return a.number if hasattr(a, "number") else a


def _unit(a):
    return getattr(a, "unit", None) if hasattr(a, "number") else None


def _with_unit(value, unit):
    """``value | unit`` as the reference returns it (``... | fp.unit``, splib/sputils.py:86); plain numbers without one"""
    if unit is None:
        return value
    new = getattr(unit, "new_quantity", None)       # amuse.units.core.unit: what `number | unit` calls
    return new(value) if new is not None else (value | unit)


class _Io:
    """moves the arguments of one call to the engine's device(s) and the result back to where they came from.  With a
    multi.MultiDeviceEngine a batch of rows (2-D arguments from the host, enough rows) is dealt out in row blocks, one per
    device, each device runs the operator on ITS rows and the result is concatenated on the host (round 5; rounds 3-4 ran
    every helper on the first device); 1-D arguments shared by all rows are replicated."""

    def __init__(self):
        eng = _engine()
        self.multi = eng if hasattr(eng, "engines") else None
        self.eng = eng
        self.on_device = False
        self.sharded = False

    def _host(self, a, unit=None):
        a = _num(a, unit)
        if isinstance(a, torch.Tensor):
            return a
        a = numpy.asarray(a, dtype=numpy.float64)
        if a.ndim:                                  # (ascontiguousarray would turn a 0-d scalar into a vector)
            a = numpy.ascontiguousarray(a)          # negative strides ([::-1] views) included
        return a.copy() if not a.flags.writeable else a

    def devs(self, *args, shard=True):
        """every argument of one call -- bare values or (value, unit-to-convert-to) pairs; None passes through -- on the
        device(s): ONE decision for the whole call, so that row-sharded and replicated arguments share a partition"""
        pairs = [(a if isinstance(a, tuple) else (a, None)) for a in args]
        vals = [None if v is None else self._host(v, u) for v, u in pairs]
        tensors = [v for v in vals if isinstance(v, torch.Tensor)]
        self.on_device = any(t.device.type == "cuda" for t in tensors)
        nrows = {v.shape[0] for v in vals if isinstance(v, numpy.ndarray) and v.ndim == 2}
        rows = max(nrows or [0])
        if shard and self.multi is not None and not tensors and len(nrows) == 1 and self.multi.devices_for(rows) > 1:
            self.sharded = True
            return [None if v is None else self.multi.to_devices(v, rows=rows if v.ndim == 2 else None, n_cols=rows) for v in vals]
        self.eng = primary = getattr(self.eng, "primary", self.eng)
        return [None if v is None else (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)).to(primary.device, primary.dtype)
                for v in vals]

    def dev(self, a, dtype=None, unit=None):
        return self.devs((a, unit))[0]

    def back(self, t, scalar=False):
        if isinstance(t, Sharded):
            return t.to_host()
        if self.on_device:
            return t
        out = t.cpu().numpy()
        return out[()] if scalar else out


def exner(p):
    """Exner function (p / pref0) ** (rd / cp), splib/sputils.py:28-29"""
    io = _Io()
    pd = io.dev(p)
    return io.back(io.eng.exner(pd, inverse=False), scalar=pd.dim() == 0)


def iexner(p):
    """inverse Exner function (p / pref0) ** (-rd / cp), splib/sputils.py:33-34"""
    io = _Io()
    pd = io.dev(p)
    return io.back(io.eng.exner(pd, inverse=True), scalar=pd.dim() == 0)


def rms(a, axis=None):
    """root mean square sqrt(mean(a ** 2)), splib/sputils.py:23-24: ONE number over the whole array whatever its shape, as
    the reference (numpy.mean over every axis).  ``axis=-1`` (beyond the reference): the rms of every row of a 2-D array."""
    io = _Io()
    unit = _unit(a)
    if axis is None:
        a = _num(a)
        a = a.reshape(-1) if isinstance(a, torch.Tensor) else numpy.asarray(a, dtype=numpy.float64).reshape(-1)   # C order: ONE flat run
    ad = io.dev(a)
    if axis is not None and (axis not in (-1, 1) or ad.dim() != 2):
        raise ValueError("rms: axis must be None (whole array, as the reference) or -1 on a 2-D array (per row)")
    return _with_unit(io.back(io.eng.rms(ad), scalar=ad.dim() == 1), unit)


def _periodic(x, xp, fp, period):
    """``numpy.interp(..., period=)`` (what ``**kwargs`` of splib/sputils.py:82-86 passes through) is a host-side
    normalisation in NumPy itself followed by the ordinary interpolation: abscissae modulo ``|period|``, samples sorted, one
    wrapped sample added at either end, ``left`` / ``right`` ignored.  The same steps with the same NumPy operations here --
    per row for batches -- so the kernel that follows returns numpy's bits."""
    period = float(_num(period))
    if period == 0:
        raise ValueError("period must be a non-zero value")
    period = abs(period)
    host = lambda a: numpy.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else _num(a), dtype=numpy.float64)   # noqa: E731
    x, xp, fp = host(x) % period, host(xp) % period, host(fp)
    if xp.shape[-1] != fp.shape[-1]:
        raise ValueError("fp and xp are not of the same length")
    if xp.ndim == 1 and fp.ndim == 2:
        xp = numpy.broadcast_to(xp, fp.shape)
    if fp.ndim == 1 and xp.ndim == 2:
        fp = numpy.broadcast_to(fp, xp.shape)
    order = numpy.argsort(xp, axis=-1)
    xp, fp = numpy.take_along_axis(xp, order, axis=-1), numpy.take_along_axis(fp, order, axis=-1)
    xp = numpy.concatenate((xp[..., -1:] - period, xp, xp[..., 0:1] + period), axis=-1)
    fp = numpy.concatenate((fp[..., -1:], fp, fp[..., 0:1]), axis=-1)
    return x, numpy.ascontiguousarray(xp), numpy.ascontiguousarray(fp)


def _outside(r, xd, xpd, left, right):
    """numpy.interp's ``left`` / ``right``: two selects behind the kernel (NaN abscissae keep the kernel's NaN)"""
    def fix(r_, x_, xp_):
        lo, hi = xp_[..., :1], xp_[..., -1:]
        if left is not None:
            r_ = torch.where(x_ < lo, torch.as_tensor(float(_num(left)), dtype=r_.dtype, device=r_.device), r_)
        if right is not None:
            r_ = torch.where(x_ > hi, torch.as_tensor(float(_num(right)), dtype=r_.dtype, device=r_.device), r_)
        return r_
    return r.map(fix, xd, xpd) if isinstance(r, Sharded) else fix(r, xd, xpd)


def interp(x, xp, fp, **kwargs):
    """numpy.interp(x, xp, fp, **kwargs) (splib/sputils.py:82-86) for one column (1-D arguments) or for every row of 2-D
    arguments (x and xp may stay 1-D: shared by all rows).  As the reference: ``xp`` is converted to ``x``'s unit, the
    result carries ``fp``'s unit; ``left`` / ``right`` (the values outside [xp[0], xp[-1]]) and ``period`` are honoured as numpy
    does (no call site of the reference uses any of the three)."""
    left, right, period = kwargs.pop("left", None), kwargs.pop("right", None), kwargs.pop("period", None)
    if kwargs:
        raise TypeError("interp() got an unexpected keyword argument %r" % sorted(kwargs)[0])
    io = _Io()
    ux, ufp = _unit(x), _unit(fp)
    if period is not None:              # numpy's own preprocessing, on the host; then the same kernel
        x, xp, fp = _periodic(x, _num(xp, ux) if hasattr(xp, "value_in") and ux is not None else xp, fp, period)
        left = right = ux = None
    xd, xpd, fpd = io.devs(x, (xp, ux), fp)
    scalar = xd.dim() == 0
    if scalar:
        xd = xd.reshape(1)
    r = io.eng.interp(xd, xpd, fpd)
    if left is not None or right is not None:
        with io.eng.on_stream():
            r = _outside(r, xd, xpd, left, right)
    return _with_unit(io.back(r[..., 0] if scalar else r, scalar=scalar and r.dim() == 1), ufp)


def searchsorted(a, v, **kwargs):
    """numpy.searchsorted(a, v, side=...) (splib/sputils.py:88-91) for one column or per row; int64 indices"""
    side = kwargs.pop("side", "left")
    if kwargs:
        raise NotImplementedError("sputils.searchsorted on the GPU: numpy.searchsorted's %s not supported" % sorted(kwargs))
    io = _Io()
    ad, vd = io.devs(a, (v, _unit(a)))                                # v.value_in(a.unit), splib/sputils.py:91
    scalar = vd.dim() == 0
    if scalar:
        vd = vd.reshape(1)
    r = io.eng.searchsorted(ad, vd, side=side)
    return io.back(r[..., 0] if scalar else r, scalar=scalar and r.dim() == 1)


def integral(a, b, z, q, w=None):
    """integral from a to b of the piece-wise constant q(z) (value q[i] on [z[i], z[i+1]]), optionally weighted by w:
    splib/sputils.py:94-161.  Returns None when an end point lies outside z, as the reference does (scalar call); with
    arrays a, b of n_rows end points (and 2-D z / q / w or shared 1-D z) the rows outside give NaN."""
    io = _Io()
    ad, bd, zd, qd, wd = io.devs(a, b, z, q, w, shard=False)            # end points per row: assembled with torch ops on ONE device
    scalar = ad.dim() == 0 and bd.dim() == 0
    if not scalar:                                                       # one end point given for all rows: broadcast
        ad, bd = torch.broadcast_tensors(ad.reshape(-1) if ad.dim() else ad.reshape(1), bd.reshape(-1) if bd.dim() else bd.reshape(1))
    Zh = torch.stack([bd.reshape(-1), ad.reshape(-1)], dim=1)            # layer k = [Zh[k+1], Zh[k]] = [a, b]
    if scalar:
        if zd.shape[-1] != qd.shape[-1] + 1:
            print("len(z) should be len(q) + 1. len(z)=%d, len(q) = %d", (zd.shape[-1], qd.shape[-1]))      # sputils.py:111-112
        r = io.eng.interp_c(Zh[0], zd, qd, wd, mode="integral")
        val = float(r[0])
        if val != val and not bool(torch.isnan(ad) | torch.isnan(bd)):
            lo, hi = float(zd[0]), float(zd[-1])
            if float(ad) < lo or float(ad) > hi or float(bd) < lo or float(bd) > hi:
                print("integral: Interval end point outside range.")                                       # sputils.py:114
                return None
        return r[0] if io.on_device else val
    if qd.dim() == 1:
        qd = qd.unsqueeze(0).expand(Zh.shape[0], -1)
        wd = wd.unsqueeze(0).expand(Zh.shape[0], -1) if wd is not None else None
    r = io.eng.interp_c(Zh, zd, qd, wd, mode="integral")
    return io.back(r[:, 0])


def interp_c(Zh, zh, q, rho):
    """conservative interpolation from fine to coarse levels (splib/sputils.py:173-189): Q[i] = rho-weighted mean of q over
    [Zh[i+1], Zh[i]] where Zh[i] < zh[-1], else 0.  One column (1-D) or [n_cols x ...] batches (zh may stay 1-D)."""
    io = _Io()
    Zd, zd, qd, rd_ = io.devs(Zh, zh, q, rho)
    return io.back(io.eng.interp_c(Zd, zd, qd, rd_, mode="interp_c"))


def interp_rho(Zh, zh, rho):
    """a density on the coarser grid (splib/sputils.py:191-197): integral(Zh[i+1], Zh[i], zh, rho) / (Zh[i] - Zh[i+1])"""
    io = _Io()
    Zd, zd, rd_ = io.devs(Zh, zh, rho)
    return io.back(io.eng.interp_c(Zd, zd, rd_, None, mode="interp_rho"))


def find_closest_points(points, target):
    """indices of ``points`` sorted by great-circle distance to ``target`` (splib/sputils.py:40-42 with splib/haversine.py:
    first coordinate = longitude, second = latitude, 6371 km sphere).  Start-up geometry on a handful of grid points,
    not column arithmetic: plain host code, as in the reference."""
    lng1, lat1 = numpy.radians(numpy.asarray(points, dtype=numpy.float64)).T
    lng2, lat2 = numpy.radians(numpy.asarray(target, dtype=numpy.float64))
    d = numpy.sin((lat2 - lat1) * 0.5) ** 2 + numpy.cos(lat1) * numpy.cos(lat2) * numpy.sin((lng2 - lng1) * 0.5) ** 2
    return numpy.argsort(2 * 6371 * numpy.arcsin(numpy.sqrt(d)))


def _lonlat(points, eng):
    """(lon, lat) float64 vectors on the engine's device from a list of (lon, lat) tuples, an [n x 2] array or an [n x 2]
    tensor; and whether the caller's points were on a device"""
    if isinstance(points, torch.Tensor):
        on_device = points.device.type == "cuda"
        t = points.reshape(-1, 2)
    else:
        on_device = False
        t = torch.from_numpy(numpy.asarray(points, dtype=numpy.float64).reshape(-1, 2))
    t = t.to(device=eng.device, dtype=torch.float64)
    return t[:, 0].contiguous(), t[:, 1].contiguous(), on_device


SPC_LOC_BOUNDARY, SPC_LOC_INTERIOR = 1, 2          # include/spc.h SPC_LOC_*


def _contains(codes):
    """[n x 2] bool: where ``contains`` holds for the point and for its image, from the location codes [n_polys x n x 2] of
    the polygons of ONE geometry -- GEOS's point locator with the Mod-2 boundary rule: an odd number of boundaries is the
    boundary, else interior where any polygon holds the point or a boundary was hit; contains == interior"""
    nb = (codes == SPC_LOC_BOUNDARY).sum(dim=0)
    inside = (codes == SPC_LOC_INTERIOR).any(dim=0)
    return (nb % 2 == 0) & (inside | (nb > 0))



def get_mask_indices(points, mask_geoms, nmax=-1):
    """The grid columns a set of mask geometries selects, splib/sputils.py:46-73 step by step, on the GPU: which points
    (``(lon, lat)`` tuples as splib.initialize passes them, an [n x 2] array, or an [n x 2] device tensor) lie in the
    polygons, or lie nearest to the points, of ``mask_geoms`` (sp_coupler_amd.geometry, or shapely's own objects).

    * ``nmax == 0``: ``[]``.
    * ONE Point: the ``nmax`` nearest columns (great-circle distance, splib/haversine.py) as an int64 array (a device tensor
      for device points) in a STABLE order -- the reference's ``numpy.argsort`` is not stable, so among exactly equal
      distances its order is NumPy's, ours the index order; ``nmax < 0``: ``[argmin]``, the first of the nearest.
    * otherwise (``nmax`` ignored, as in the reference): a Point adds the argmin of its distances, a polygon every ``i``
      whose point ``p`` or image ``q = ((lon - 180) % 360 - 180, lat)`` it contains, ascending; the result is
      ``list(set(result))`` of ints, built as the reference builds it, so its order (the order in which the LES are
      created) is the reference's.
    ``contains`` is GEOS's point locator in exact arithmetic: a point on a polygon's boundary is
    not contained."""
    from . import geometry
    if nmax == 0:
        return []                                   # requested no points
    eng = _engine()
    eng = getattr(eng, "primary", eng)
    masks = [geometry.as_mask(g) for g in mask_geoms]
    lon, lat, on_device = _lonlat(points, eng)

    def nearest(g):
        if lon.shape[0] == 0:
            raise ValueError("attempt to get argmin of an empty sequence")
        return eng.haversine(lon, lat, g.x, g.y)

    if len(masks) == 1 and isinstance(masks[0], geometry.Point):
        d = nearest(masks[0])
        if nmax > 0:
            with eng.on_stream():
                idx = torch.sort(d, stable=True).indices[:nmax]
            return idx if on_device else idx.cpu().numpy()
        return [int(torch.argmin(d))]
    result = []
    for m in masks:
        if isinstance(m, geometry.Point):
            result.append(int(torch.argmin(nearest(m))))
        else:
            codes = eng.point_in_polygon(lon, lat, *geometry.pack(*m))
            result.extend(torch.nonzero(_contains(codes).any(dim=1)).flatten().tolist())
    return list(set(result))                        # remove duplicates, in the reference's order
