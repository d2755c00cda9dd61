"""NumPy oracle of K10 (slab means and cloud fraction of the LES 3-D fields) and the host twin of
``models.DeviceLESEnsemble``: the same arithmetic on NumPy fields, through the host-field path of spcpl.

The cloud-fraction rule is this project's definition: the reference reaches DALES's routine through OMUSE
and contains no such code; the rule is derived from the geometry of splib/spcpl.py:760-765."""
import numpy

from sp_coupler_amd import models


def slab_means(field):
    """[n x itot x jtot x ktot] -> [n x ktot]: numpy.mean over the horizontal plane of every LES, in the field's dtype"""
    return numpy.stack([f.mean(axis=(0, 1)) for f in field]) if len(field) else numpy.empty((0, field.shape[-1]), field.dtype)


def sequential_mean(f):
    """what numpy.mean(f, axis=(0, 1)) does for ktot >= 2: acc = 0; acc += f[i, j, :] row by row in f's dtype; one division"""
    rows = f.reshape(-1, f.shape[-1])
    acc = numpy.zeros(f.shape[-1], dtype=f.dtype)
    for r in rows:
        acc = acc + r
    return acc / f.dtype.type(rows.shape[0])


def layer_ranges(idx, ktot):
    """[(lo, hi)] per GCM layer r counted from the ground: LES levels [hi[r-1], hi[r]), hi[r] = clip(idx[r], 0, ktot)"""
    hi = numpy.clip(numpy.asarray(idx, dtype=numpy.int64), 0, ktot)
    lo = numpy.concatenate([[0], hi[:-1]])
    return [(int(a), int(b)) for a, b in zip(lo, hi)]


def cloud_fraction(ql, idx):
    """ql [n x itot x jtot x ktot], idx [n x nG] -> A [n x nG] in ql's dtype: the fraction of (i, j) columns with ql > 0
    at some level of the layer; 0 for an empty layer; NaN and -0.0 are not cloudy"""
    n, itot, jtot, ktot = ql.shape
    A = numpy.zeros((n, idx.shape[1]), dtype=ql.dtype)
    with numpy.errstate(invalid="ignore"):
        cloudy = ql > 0
    for l in range(n):
        for r, (lo, hi) in enumerate(layer_ranges(idx[l], ktot)):
            if hi > lo:
                A[l, r] = ql.dtype.type(int(cloudy[l, :, :, lo:hi].any(axis=2).sum())) / ql.dtype.type(itot * jtot)
    return A


def hand_case(dtype):
    """a small QL (8 x 8 x 20) with a NaN, a -0.0 and a negative value, two index maps (the reference's known answer; one
    with an index beyond ktot and a non-monotone step) and the cloudy-column counts of every layer, counted by hand
    (tests/test_slab_cpu.py spells the same case out against the oracle)"""
    ql = numpy.zeros((1, 8, 8, 20), dtype=dtype)
    ql[0, 0, 0, 0] = 1e-5
    ql[0, 0, 1, 0] = numpy.nan
    ql[0, 0, 2, 0] = -0.0
    ql[0, 0, 3, 0] = -1e-5
    ql[0, 1, 0, 1] = 2e-5
    ql[0, 1, 1, 2] = 2e-5
    ql[0, 1, 1, 4] = 3e-5
    ql[0, 2, 2, 4] = 1e-6
    ql[0, 7, 7, 19] = 1e-4
    ql[0, 1, 0, 5] = 1e-4
    idx = numpy.array([[0, 0, 1, 5, 20], [1, 99, 5, 20, 20]], dtype=numpy.int32)
    counts = numpy.array([[0, 0, 1, 3, 2], [1, 4, 0, 2, 0]])
    return ql, idx, counts


class _HostRow(models._LESRow):
    """per-column face of the twin: a profile getter returns row i of what get_profiles_batched((key,)) returns at that
    moment (the fields are the truth: after a nudge or set_fields_batched the raw ``p`` still holds the means of the old ones)"""

    def get_itot(self):
        return self._e.itot

    def get_jtot(self):
        return self._e.jtot


def _host_row_getter(key):
    plain = models._row_getter(key)

    def get(self, return_request=False):
        self._e._refresh_profile(key)
        return plain(self, return_request)
    return get


for _m, _k in (("get_profile_U", "U"), ("get_profile_V", "V"), ("get_profile_THL", "THL"), ("get_profile_QT", "QT"),
               ("get_profile_QL", "QL"), ("get_profile_QL_ice", "QL_ice"), ("get_profile_QR", "QR"), ("get_profile_T", "T")):
    setattr(_HostRow, _m, _host_row_getter(_k))


class HostFieldLESEnsemble(models.SyntheticLESEnsemble):
    """models.DeviceLESEnsemble with NumPy fields of ``dtype`` T (float64, or float32 for the twin of an ensemble on a float32
    engine): spcpl takes its host-field path.  The executable definition of what the device ensemble computes.  The rule of T,
    stated here and in every twin above this one without a helper of device_les.py (with T = float64 every ``astype`` below is
    the identity):
      * the fields and every kernel output are T (km, phi, counts' partners, water paths, fluxes, mtop, statistics);
      * a quantity the host forms is formed in float64 from float64 inputs and rounded ONCE, ``_r``: .astype(T), where a kernel
        takes it (hx, hy, a, m, cp, s0, gx ... l2, kcap, kh2, w, c, tables, t0, lex, s, g, r, the surface fluxes);
      * the step is (tend.astype(T) * T(dt)).astype(T), then one add in T (``_step``);
      * what comes back from a kernel enters ``p`` widened exactly, ``_w``; the host arithmetic on p (PS, T, QL_ice, Rain
        without the microphysics) stays float64;
      * a comparison the host makes uses the rounded value on both sides (mixing_capped, the substeps from the Courant maximum)."""

    MEAN_KEYS = ("U", "V", "THL", "QT", "QL")
    STEP_KEYS = ("U", "V", "THL", "QT")
    dtype = numpy.float64                                          # T: a class attribute, or the ``dtype`` of for_gcm

    def _r(self, a):
        """a float64 quantity of the host rounded once to T, contiguous: what a kernel takes"""
        return numpy.ascontiguousarray(numpy.asarray(a, dtype=numpy.float64).astype(self.dtype))

    @staticmethod
    def _w(a):
        """what came back from a kernel, widened exactly: what enters p"""
        return numpy.asarray(a, dtype=numpy.float64)

    def _step(self, dt, keys=STEP_KEYS):
        """every field of ``keys`` that has a tendency takes (tend.astype(T) * T(dt)).astype(T) in one add in T"""
        f, T = self.fields3d, numpy.dtype(self.dtype).type
        for key in keys:
            if key in self.tend and key in f:
                inc = (self._r(self.tend[key]) * T(dt)).astype(self.dtype)
                f[key] = f[key] + inc[:, None, None, :]

    def __init__(self, grid_indices, zf, zh, prof, itot=8, jtot=8):
        super().__init__(grid_indices, zf, zh, prof)
        self.itot, self.jtot = itot, jtot
        self.fields3d = {}

    @classmethod
    def for_gcm(cls, gcm, grid_indices, nL=160, seed=0, itot=8, jtot=8, dtype=None):
        ens = super().for_gcm(gcm, grid_indices, nL, seed)
        ens.itot, ens.jtot = itot, jtot
        if dtype is not None:
            ens.dtype = numpy.dtype(dtype).type
        return ens

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.n))]
        if self._rows[i] is None:
            self._rows[i] = _HostRow(self, i)
        return self._rows[i]

    def _refresh_profile(self, key):
        if key in self.MEAN_KEYS and key in self.fields3d:
            self._slab_means()

    def attach_fields(self, fields):
        for k, v in fields.items():
            self.set_fields_batched(k, v)

    def set_fields_batched(self, name, values):
        """the field rounded to T: what the upload of the device ensemble does"""
        super().set_fields_batched(name, values)
        self.fields3d[name] = self.fields3d[name].astype(self.dtype)

    def _ensure_ql(self):
        f = self.fields3d
        if "QL" not in f:
            f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)

    def get_fields_batched(self, name):
        if name == "QL":
            self._ensure_ql()
        return self.fields3d[name].copy()

    def _slab_means(self):
        if "QT" in self.fields3d and "Qsat" in self.fields3d:
            self._ensure_ql()
        m = {k: self._w(slab_means(self.fields3d[k])) for k in self.MEAN_KEYS if k in self.fields3d}
        self.p.update(m)
        return m

    def get_profiles_batched(self, keys, out):
        means = self._slab_means() if any(k in self.MEAN_KEYS and k in self.fields3d for k in keys) else {}
        for k in keys:
            numpy.copyto(out[k], means[k] if k in means else self.p[k])

    def get_cloudfraction_batched(self, indices, out):
        self._ensure_ql()
        numpy.copyto(out, cloud_fraction(self.fields3d["QL"], numpy.asarray(indices)))          # (T, widened exactly)

    def evolve_model_batched(self, t):
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        f, p = self.fields3d, self.p
        self._step(dt)
        if "QL" in f or ("QT" in f and "Qsat" in f):
            f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
        self._slab_means()
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        p["QL_ice"] = numpy.minimum(p["QL_ice"], p["QL"])
        p["T"] = p["THL"] * (p["presf"] / 1e5) ** (287.04 / 1004.) + 2.53e6 * p["QL"] / 1004.
        p["Rain"] = p["Rain"] + 1e-6 * dt
        self.model_time = float(t)
