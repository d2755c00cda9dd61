"""NumPy oracle of K13 (include/spc.h: spc_les_water_paths_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_water_paths_gpu.py (each takes an engine: tools/mutation_control.py --waterpath hands them the engines of its
mutant libraries), the host twin of models.DeviceLESEnsemble's water-path methods and an oracle-backed engine with
``les_water_paths`` for the CPU suite.

Every device array of the bodies is the LEADING part of a poisoned buffer (tests/les_harness.Poisoned); the bytes behind it
(and in front of a view off the 16-byte grid) are checked after the launch."""
import numpy
import torch

from sp_coupler_amd import _abi, models, spcpl
from tests import les_thermo_ref as ltr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import DTYPES, NP, Poisoned, np_of, on_both, run_bodies, twin_kw  # noqa: F401  (DTYPES: for the tests)
from tests.test_vnudge import make_les_fields

PLANES = [(1, 1), (3, 5), (8, 8)]
#: below, on and above 8 (the sequential rows), 128 (one pairwise block), 256 / 512 (splits that halve exactly); 160 the LES
#: of the benchmark; 300 splits at 150 -> 144 on the unrolled recursion (the other lengths below 968 split at multiples of 8
#: anyway); 1000 is above 968: the explicit stack, and splits at 500 -> 496
KTOTS = [1, 2, 7, 8, 9, 127, 128, 129, 160, 257, 300, 512, 1000]
ROWS_PER_WORKGROUP = 32


# -- the rule --------------------------------------------------------------------------------------------------------------
def water_paths(field, w):
    """[n x itot x jtot x ktot], [n x ktot] -> [n x itot x jtot]: the product rounded first, then NumPy's sum along the
    contiguous axis"""
    assert field.dtype == w.dtype and field.flags.c_contiguous
    with numpy.errstate(all="ignore"):
        prod = field * w[:, None, None, :]
        return prod.sum(axis=3)


def cloud_top(field):
    """int32 [n x itot x jtot]: the largest k with field > 0, else -1; NaN and -0.0 are not cloudy"""
    with numpy.errstate(invalid="ignore"):
        cloudy = field > 0
    ktot = field.shape[-1]
    top = ktot - 1 - numpy.argmax(cloudy[..., ::-1], axis=-1)
    return numpy.where(cloudy.any(axis=-1), top, -1).astype(numpy.int32)


def cloud_cover(top):
    """[n] float64 counts / the plane size are formed by the caller's dtype: see ``cover_of``"""
    return (top >= 0).reshape(top.shape[0], -1).sum(axis=1)


def cover_of(top, dtype):
    T = numpy.dtype(dtype).type
    nij = int(numpy.prod(top.shape[1:]))
    return numpy.array([T(int(c)) / T(nij) for c in cloud_cover(top)], dtype=dtype)


def sequential(field, w):
    """the k loop: what the result would be if the row were summed in order"""
    acc = numpy.zeros(field.shape[:3], dtype=field.dtype)
    with numpy.errstate(all="ignore"):
        for k in range(field.shape[-1]):
            acc = acc + field[..., k] * w[:, None, None, k]
    return acc


def per_row_sum(field, w):
    """ndarray.sum() of every row's products on its own"""
    out = numpy.empty(field.shape[:3], dtype=field.dtype)
    with numpy.errstate(all="ignore"):
        for l, i, j in numpy.ndindex(*field.shape[:3]):
            out[l, i, j] = (field[l, i, j, :] * w[l, :]).sum()
    return out


# -- inputs ------------------------------------------------------------------------------------------------------------------
def case(shape, dtype, nf=1, seed=0):
    """``nf`` fields of mixed sign and magnitude (sums that depend on their order) and a positive weight profile"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(4000 + seed + 13 * ktot + itot * jtot + 1000 * n)
    fields = [(rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 3, shape)).astype(dtype) for _ in range(nf)]
    w = (rng.random((n, ktot)) * 30.0 + 1.0).astype(dtype)
    return fields, w


def cloud_case(dtype, ktot=40, plane=(3, 5), n=3):
    """QL-like field: LES 0 has no cloudy cell at all (cover 0), LES 1 is cloudy in every column (cover 1), LES 2 holds one
    column cloudy only at k = 0, one only at k = ktot - 1, one with NaN cells, one with -0.0 cells, one with negative cells (none
    of the last three cloudy) and ordinary columns"""
    dtype = numpy.dtype(dtype).type
    rng = numpy.random.default_rng(77 + ktot)
    shape = (n,) + plane + (ktot,)
    q = numpy.where(rng.random(shape) < 0.1, rng.random(shape) * 1e-3, 0.0)
    q[0] = 0.0
    q[0, 0, 0, :] = -0.0
    q[1, ..., rng.integers(0, ktot)] += 1e-4
    q[2, 0, :, :] = 0.0
    q[2, 0, 0, 0] = 1e-4
    q[2, 0, 1, ktot - 1] = 1e-4
    q[2, 0, 2, :] = numpy.nan
    q[2, 0, 3, :] = -0.0
    q[2, 0, 4, :] = -1e-4
    w = (rng.random((n, ktot)) * 30.0 + 1.0).astype(dtype)
    return q.astype(dtype), w


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one launch through ``eng.les_water_paths`` with every array inside a poisoned buffer; ``check`` compares every output with
    the oracle bit for bit, the inputs with what was uploaded, and looks at the bytes around every array"""

    def __init__(self, eng, fields, w, cloud=None, top=False, cover=False, lead=0, pad=0, lead_w=0):
        self.eng, self.fields, self.w, self.cloud, self.pad = eng, fields, w, cloud, pad
        dtype, shape = w.dtype, fields[0].shape
        n, ktot = shape[0], shape[-1]
        self.mem = Poisoned(eng, tail_elems=max(64, 4 * ktot))
        put = self.mem.put
        self.names = ["F%d" % f for f in range(len(fields))]
        self.dfields = {k: put(k, a, float("nan"), lead) for k, a in zip(self.names, fields)}
        self.dw = self.mem.rows("w", w, 1e30, lead_w, pad)
        self.out = {k: put("out " + k, numpy.full(shape[:3], -3.0, dtype), -5.0, lead) for k in self.names}
        self.dtop = put("top", numpy.full(shape[:3], -9, numpy.int32), -11, lead) if top else False
        self.dcover = put("cover", numpy.full((n,), -3.0, dtype), -5.0, lead) if cover else False
        self.got = eng.les_water_paths(self.dfields, self.dw, cloud=None if cloud is None else self.names[cloud], out=self.out,
                                       top=self.dtop, cover=self.dcover)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        want = {k: water_paths(a, self.w) for k, a in zip(self.names, self.fields)}
        keys = list(self.names)
        if self.dtop is not False:
            want["top"] = cloud_top(self.fields[self.cloud])
            keys.append("top")
        if self.dcover is not False:
            want["cover"] = cover_of(cloud_top(self.fields[self.cloud]), self.w.dtype)
            keys.append("cover")
        assert list(self.got) == keys, (what, list(self.got))
        for k in keys:
            mine = self.out[k] if k in self.out else (self.dtop if k == "top" else self.dcover)
            assert self.got[k].data_ptr() == mine.data_ptr() and self.got[k].shape == mine.shape, (what, k)
            assert self.got[k].cpu().numpy().dtype == want[k].dtype, (what, k)
            assert_bits("%s %s" % (what, k), self.got[k].cpu().numpy(), want[k])
        for k, a in zip(self.names, self.fields):
            assert Poisoned.read_only(self.dfields[k], a), (what, k, "read only")
        assert numpy.array_equal(self.dw.cpu().numpy(), self.w), (what, "w read only")
        self.mem.check_around(what)
        return want


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, nf=1, n=3):
    """n x plane rows (3, 45 and 192 rows with n = 3: less than one workgroup of 32 rows, one and a part, six whole ones) of nf
    fields against the oracle; from ktot = 8 on the inputs tell the pairwise order from the k loop"""
    fields, w = case((n,) + tuple(plane) + (ktot,), np_of(eng), nf)
    want = Run(eng, fields, w).check("plane %s ktot %d nf %d" % (plane, ktot, nf))
    if ktot >= 8 and plane != (1, 1):
        assert not numpy.array_equal(want["F0"], sequential(fields[0], w))


def check_rows(eng):
    """row counts that are no multiple of the rows per workgroup: one LES (n = 1) of 1, 15 and 35 rows; 5 LES of 7 rows (a wave's
    eight rows span two LES: the cover's per-row atomics); 3 LES of 33 rows, with the cloud outputs"""
    for n, plane in ((1, (1, 1)), (1, (3, 5)), (1, (5, 7)), (5, (7, 1)), (3, (3, 11))):
        assert (n * plane[0] * plane[1]) % ROWS_PER_WORKGROUP
        fields, w = case((n,) + plane + (24,), np_of(eng), 2, seed=n)
        fields[1] = numpy.where(fields[1] > 30.0, fields[1], 0).astype(fields[1].dtype)             # a sparse cloud field
        want = Run(eng, fields, w, cloud=1, top=True, cover=True).check("n %d plane %s" % (n, plane))
        assert n * plane[0] * plane[1] < 15 or ((want["top"] >= 0).any() and (want["top"] < 0).any())


def check_few_rows(eng):
    """fewer than 8 rows over several LES, so that ONE wave holds live rows of several LES and dead groups behind them: 2 ... 7
    LES of 1 x 1 and 2 LES of 1 x 3, every row cloudy (cover 1 in EVERY LES, not their sum in the first), then one LES clear"""
    for n, plane in [(n, (1, 1)) for n in range(2, 8)] + [(2, (1, 3))]:
        fields, w = case((n,) + plane + (12,), np_of(eng), 1, seed=20 + n)
        q = numpy.abs(fields[0]) + fields[0].dtype.type(1e-3)
        want = Run(eng, [q], w, cloud=0, top=True, cover=True).check("few rows, all cloudy: n %d plane %s" % (n, plane))
        assert (want["cover"] == 1).all() and len(want["cover"]) == n
        q[n - 1] = 0.0
        want = Run(eng, [q], w, cloud=0, cover=True).check("few rows, the last LES clear: n %d plane %s" % (n, plane))
        assert want["cover"].tolist() == [1.0] * (n - 1) + [0.0]


def check_four_fields(eng):
    """four fields in one launch, the cloud outputs taken from the third; ktot on both sides of the first split"""
    for ktot in (7, 129, 160):
        fields, w = case((3, 3, 5, ktot), np_of(eng), 4, seed=9)
        fields[2] = numpy.where(fields[2] > 20.0, fields[2], 0).astype(fields[2].dtype)
        want = Run(eng, fields, w, cloud=2, top=True, cover=True).check("four fields ktot %d" % ktot)
        assert len({want[k].tobytes() for k in ("F0", "F1", "F2", "F3")}) == 4


def check_alignment(eng, lead, lead_w, pad):
    """views one (or more) elements off the 16-byte grid and a pitched w"""
    fields, w = case((3, 3, 5, 65), np_of(eng), 2, seed=lead + 10 * lead_w + 100 * pad)
    Run(eng, fields, w, cloud=0, top=True, cover=True, lead=lead, lead_w=lead_w, pad=pad).check("lead %d %d pad %d" % (lead, lead_w, pad))


def check_cloud(eng):
    """cloudy only at k = 0, only at k = ktot - 1, nowhere; NaN and -0.0 cells; cover 0 and 1; top alone, cover alone, both"""
    for ktot in (5, 40, 130):
        q, w = cloud_case(np_of(eng), ktot)
        want = Run(eng, [q], w, cloud=0, top=True, cover=True).check("cloud ktot %d" % ktot)
        assert want["cover"][0] == 0 and want["cover"][1] == 1 and 0 < want["cover"][2] < 1
        assert want["top"][2, 0].tolist() == [0, ktot - 1, -1, -1, -1] and (want["top"][0] == -1).all()
        Run(eng, [q], w, cloud=0, top=True).check("top alone")
        Run(eng, [q], w, cloud=0, cover=True).check("cover alone")


def check_nonfinite(eng):
    """a row holding inf against w = 0 (NaN), inf against w > 0 (inf), both signs of inf (NaN), NaN, and rows of -0.0 (+0.0)"""
    for ktot in (5, 8, 200):
        fields, w = case((2, 3, 5, ktot), np_of(eng), 1, seed=3)
        f = fields[0]
        w[:, 2] = 0.0
        f[:, 0, 0, 2] = numpy.inf
        f[:, 0, 1, 1] = numpy.inf
        f[:, 0, 2, 1], f[:, 0, 2, 3] = numpy.inf, -numpy.inf
        f[:, 0, 3, ktot - 1] = numpy.nan
        f[:, 0, 4, :] = -0.0
        f[:, 1, 0, :] = 0.0
        want = Run(eng, [f], w).check("non-finite ktot %d" % ktot)["F0"]
        assert numpy.isnan(want[:, 0, 0]).all() and (want[:, 0, 1] == numpy.inf).all() and numpy.isnan(want[:, 0, 2]).all()
        assert numpy.isnan(want[:, 0, 3]).all() and (want[:, 0, 4] == 0).all() and not numpy.signbit(want[:, 0, 4]).any()


def check_refusals(eng):
    """ktot = 8193 is refused by the library; n = 0 returns empties without a launch; the engine's own argument checks"""
    dev = eng.device
    w = torch.ones((1, 8193), dtype=eng.dtype, device=dev)
    f = torch.ones((1, 1, 1, 8193), dtype=eng.dtype, device=dev)
    try:
        eng.les_water_paths({"A": f}, w)
        raise AssertionError("ktot = 8193 was not refused")
    except _abi.SpcError as e:
        assert e.code == _abi.SPC_ERR_UNSUPPORTED and "8192" in str(e), str(e)
    ok = eng.les_water_paths({"A": f[..., :8192].contiguous()}, w[:, :8192].contiguous())["A"]
    assert float(ok[0, 0, 0]) == 8192.0
    res = eng.les_water_paths({"A": f[:0, :, :, :7].contiguous()}, w[:0, :7], cloud="A", top=True, cover=True)
    assert tuple(res["A"].shape) == (0, 1, 1) and tuple(res["top"].shape) == (0, 1, 1) and tuple(res["cover"].shape) == (0,)
    g = torch.ones((2, 3, 4, 6), dtype=eng.dtype, device=dev)
    v = torch.ones((2, 6), dtype=eng.dtype, device=dev)
    other = torch.float32 if eng.dtype == torch.float64 else torch.float64
    for bad in (lambda: eng.les_water_paths({}, v),
                lambda: eng.les_water_paths({k: g for k in "abcde"}, v),
                lambda: eng.les_water_paths({"A": g, "B": g[:, :, :, :3]}, v),
                lambda: eng.les_water_paths({"A": g.to(other)}, v),
                lambda: eng.les_water_paths({"A": g}, v[:, :5]),
                lambda: eng.les_water_paths({"A": g}, v, top=True),
                lambda: eng.les_water_paths({"A": g}, v, cloud="B"),
                lambda: eng.les_water_paths({"A": g}, v, out={"A": g[:, :, :, 0]}),
                lambda: eng.les_water_paths({"A": g}, v, cloud="A", cover=torch.ones(3, dtype=eng.dtype, device=dev)),
                lambda: eng.les_water_paths({"top": g}, v)):
        try:
            bad()
            raise AssertionError("an argument error was not refused")
        except ValueError:
            pass


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    fields, w = case((n, 3, 5, 40), np_of(one), 2, seed=n)
    fields[1] = numpy.where(fields[1] > 20.0, fields[1], 0).astype(fields[1].dtype)
    (_, _, dev), (_, _, sh) = on_both(one, multi, n)
    r1 = one.les_water_paths({"A": dev(fields[0]), "B": dev(fields[1])}, dev(w), cloud="B", top=True, cover=True)
    rm = multi.les_water_paths({"A": sh(fields[0]), "B": sh(fields[1])}, sh(w), cloud="B", top=True, cover=True)
    multi.synchronize()
    top = cloud_top(fields[1])
    want = {"A": water_paths(fields[0], w), "B": water_paths(fields[1], w), "top": top, "cover": cover_of(top, w.dtype)}
    assert list(r1) == list(rm) == list(want)
    for k, v in want.items():
        assert_bits("one " + k, r1[k].cpu().numpy(), v)
        assert_bits("multi " + k, rm[k].to_host(), v)
    return [int(p.shape[0]) for p in rm["A"].parts]


BODIES = ("parity", "rows", "few_rows", "four_fields", "alignment", "cloud", "nonfinite")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in KTOTS]),
            ("rows", lambda: check_rows(eng)),
            ("few_rows", lambda: check_few_rows(eng)),
            ("four_fields", lambda: check_four_fields(eng)),
            ("alignment", lambda: [check_alignment(eng, *a) for a in ((1, 0, 0), (0, 1, 0), (0, 0, 3), (3, 1, 5))]),
            ("cloud", lambda: check_cloud(eng)),
            ("nonfinite", lambda: check_nonfinite(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_water_paths (CPU suite) ----------------------------------------------------------------
class WaterPathOracleEngine(ltr.ThermoOracleEngine):
    """tests/les_thermo_ref.ThermoOracleEngine with ``les_water_paths`` by the NumPy oracle above"""

    def les_water_paths(self, fields, w, cloud=None, out=None, top=False, cover=False, **kw):
        wn = w.numpy()
        res = {k: torch.from_numpy(water_paths(numpy.ascontiguousarray(v.numpy()), wn)) for k, v in fields.items()}
        for k, t in (out or {}).items():                          # written INTO the caller's tensors, as the HIP engine does
            res[k] = t.copy_(res[k])
        asked = lambda v: v is not False and v is not None                                # noqa: E731
        into = lambda v, r: v.copy_(r) if isinstance(v, torch.Tensor) else r              # noqa: E731
        if cloud is not None and (asked(top) or asked(cover)):
            t = cloud_top(fields[cloud].numpy())
            if asked(top):
                res["top"] = into(top, torch.from_numpy(t))
            if asked(cover):
                res["cover"] = into(cover, torch.from_numpy(cover_of(t, wn.dtype)))
        return res


# -- the host twin of the water-path methods of models.DeviceLESEnsemble -----------------------------------------------------
WATER_PATHS = {"LWP": "QL", "TWP": "QT", "RWP": "QR"}


class _HostWaterPaths:
    """NumPy fields: the executable definition of get_water_paths_batched, get_water_path_means and the rows' get_field"""

    def water_path_weights(self):
        zh = numpy.asarray(self.zh_cache, dtype=numpy.float64)
        dz = numpy.empty_like(zh)
        dz[..., :-1] = zh[..., 1:] - zh[..., :-1]
        dz[..., -1] = dz[..., -2]
        return numpy.asarray(self.p["Rhobf"], dtype=numpy.float64) * dz

    def get_water_paths_batched(self, names=("LWP", "TWP", "RWP"), cloud_cover=False):
        if "LWP" in names or cloud_cover:
            self._ensure_ql()
        f = self.fields3d
        have = [k for k in names if WATER_PATHS[k] in f]
        if not have:
            raise KeyError(names)
        w = self._r(self.water_path_weights())                     # .astype(T) of the float64 product
        res = {k: water_paths(numpy.ascontiguousarray(f[WATER_PATHS[k]]), w) for k in have}
        if cloud_cover:
            res["top"] = cloud_top(f["QL"])
            res["cover"] = cover_of(res["top"], self.dtype)
        return res

    def get_water_path_means(self, names=("LWP", "TWP", "RWP")):
        return {k: numpy.array([x.mean() for x in v], dtype=self.dtype) for k, v in self.get_water_paths_batched(names).items()}

    def row_field(self, i, name):
        return self.get_water_paths_batched((name,))[name][i]


class HostWaterPathLESEnsemble(_HostWaterPaths, slab_ref.HostFieldLESEnsemble):
    pass


class HostThermoWaterPathLESEnsemble(_HostWaterPaths, ltr.HostThermoLESEnsemble):
    pass


def _host(t):
    return t if isinstance(t, numpy.ndarray) else models.DeviceLESEnsemble._host(t)


def ensemble_run(engine, n, thermo, device, itot=4, jtot=5, nL=20, with_qr=True):
    """an ensemble with attached fields; its water paths, cover, means and two rows' get_field at the start, after one
    evolve_model_batched and after one variability nudge (constantT).  Returns (ens, list of records)"""
    spcpl.set_engine(engine)
    cls = models.DeviceLESEnsemble if device else (HostThermoWaterPathLESEnsemble if thermo else HostWaterPathLESEnsemble)
    fs = [make_les_fields(itot, jtot, nL, seed=60 + (i % 7)) for i in range(n)]
    stack = lambda k: numpy.stack([f[k] for f in fs])                                      # noqa: E731
    gcm = models.BatchedSyntheticGCM(n + 4, 19, 21)
    ens = cls.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=21, itot=itot, jtot=jtot, **twin_kw(cls, engine))
    fields = {"Qsat": stack("qsat"), "QT": stack("qt"), "THL": stack("thl"), "QL": stack("ql")}
    for i, j in ((0, 0), (1, 2)):                                  # two clear columns: top == -1, cover < 1
        fields["QT"][:, i, j, :] *= 0.3
        fields["QL"][:, i, j, :] = 0.0
    if thermo:
        del fields["Qsat"], fields["QL"]
        fields["QT"][:, 2, 1, :] *= 2.0                            # and one that K12 finds cloudy whatever the profile
    if with_qr:
        fields["QR"] = numpy.random.default_rng(n).random((n, itot, jtot, nL)) * 1e-5
    ens.attach_fields({k: v.copy() for k, v in fields.items()})
    ens.p["presf"] = stack("presf")
    ens.ql_ref = stack("ql_ref")
    ens.model_time = 900.0
    if thermo:
        ens.enable_thermo()
    rng = numpy.random.default_rng(5)
    ens.set_forcings_batched(THL=rng.normal(0, 2e-4, (n, nL)), QT=rng.normal(0, 2e-7, (n, nL)))
    names = ("LWP", "TWP", "RWP")
    log = []

    def record():
        wp = ens.get_water_paths_batched(names, cloud_cover=True)
        rec = {k: numpy.array(_host(v)) for k, v in wp.items()}
        rec.update({"mean " + k: v for k, v in ens.get_water_path_means(names).items()})
        for i in (0, n - 1):
            for k in names[:2]:
                rec["row %d %s" % (i, k)] = numpy.array(ens[i].get_field(k) if device else ens.row_field(i, k))
        log.append(rec)
    record()
    ens.evolve_model_batched(1800.0)
    record()
    numpy.random.seed(11)
    spcpl.variability_nudge_ensemble(ens, 900.0, True, write=False)
    record()
    return ens, log


def same_logs(host, dev, with_qr=True, thermo=False):
    keys = ["LWP", "TWP"] + (["RWP"] if with_qr else []) + ["top", "cover"]
    assert len(host) == len(dev) == 3
    for step, (a, b) in enumerate(zip(host, dev)):
        assert list(a)[:len(keys)] == keys and set(a) == set(b), (step, list(a), list(b))
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (step, k, a[k].dtype, b[k].dtype)
            assert_bits("step %d %s" % (step, k), b[k], a[k])
    for k in ("LWP", "TWP"):                                      # the step and the nudge moved the fields, the cache followed
        assert not numpy.array_equal(host[0][k], host[1][k]), k
        # (without K12 the QL field follows QT at the next step, not at the nudge)
        assert not numpy.array_equal(host[1][k], host[2][k]) or (k == "LWP" and not thermo), k
    assert (host[0]["LWP"] > 0).any() and (host[0]["top"] >= 0).any() and (host[0]["top"] < 0).any()


def check_ensemble(one, engines, n, thermo, with_qr=True):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``"""
    host = ensemble_run(one, n, thermo, False, with_qr=with_qr)[1]
    for engine in engines:
        ens, dev = ensemble_run(engine, n, thermo, True, with_qr=with_qr)
        same_logs(host, dev, with_qr, thermo)
    return host


def check_ensemble_dtype(engine, n, thermo, itot=4, jtot=5, nL=20):
    """models.DeviceLESEnsemble on an engine of either dtype (the host twin is float64 only): at the start, after one
    evolve_model_batched and after one variability nudge, its water paths, top, cover, means and a row's get_field against the
    oracle on the ensemble's OWN fields as they are then -- copied to the host, in the engine's dtype, with
    w = water_path_weights().astype(T) and the cover's division in T"""
    T = NP[engine.dtype]
    spcpl.set_engine(engine)
    fs = [make_les_fields(itot, jtot, nL, seed=60 + (i % 7)) for i in range(n)]
    stack = lambda k: numpy.stack([f[k] for f in fs])                                      # noqa: E731
    gcm = models.BatchedSyntheticGCM(n + 4, 19, 21)
    ens = models.DeviceLESEnsemble.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=21, itot=itot, jtot=jtot, engine=engine)
    fields = {"Qsat": stack("qsat"), "QT": stack("qt"), "THL": stack("thl"), "QL": stack("ql")}
    for i, j in ((0, 0), (1, 2)):
        fields["QT"][:, i, j, :] *= 0.3
        fields["QL"][:, i, j, :] = 0.0
    if thermo:
        del fields["Qsat"], fields["QL"]
        fields["QT"][:, 2, 1, :] *= 2.0
    fields["QR"] = numpy.random.default_rng(n).random((n, itot, jtot, nL)) * 1e-5
    ens.attach_fields(fields)
    ens.p["presf"] = stack("presf")
    ens.ql_ref = stack("ql_ref")
    ens.model_time = 900.0
    if thermo:
        ens.enable_thermo()
    rng = numpy.random.default_rng(5)
    ens.set_forcings_batched(THL=rng.normal(0, 2e-4, (n, nL)), QT=rng.normal(0, 2e-7, (n, nL)))
    names = ("LWP", "TWP", "RWP")
    seen = []

    def compare(what):
        got = ens.get_water_paths_batched(names, cloud_cover=True)
        assert list(got) == list(names) + ["top", "cover"]
        w = numpy.ascontiguousarray(ens.water_path_weights().astype(T))
        host = {k: numpy.ascontiguousarray(_host(ens.get_fields_batched(WATER_PATHS[k]))) for k in names}
        assert all(a.dtype == T for a in host.values())
        want = {k: water_paths(host[k], w) for k in names}
        want["top"] = cloud_top(host["LWP"])
        want["cover"] = cover_of(want["top"], T)
        for k, v in want.items():
            g = numpy.asarray(_host(got[k]))
            assert g.dtype == v.dtype, (what, k, g.dtype)
            assert_bits("%s %s" % (what, k), g, v)
        means = ens.get_water_path_means(names)
        for k in names:
            assert_bits("%s mean %s" % (what, k), means[k], numpy.array([x.mean() for x in want[k]], dtype=T))
            assert_bits("%s row %s" % (what, k), ens[n - 1].get_field(k), want[k][n - 1])
        seen.append(want)
    compare("start")
    ens.evolve_model_batched(1800.0)
    compare("stepped")
    numpy.random.seed(11)
    spcpl.variability_nudge_ensemble(ens, 900.0, True, write=False)
    compare("nudged")
    assert not numpy.array_equal(seen[0]["TWP"], seen[1]["TWP"]) and not numpy.array_equal(seen[1]["TWP"], seen[2]["TWP"])
    assert (seen[0]["LWP"] > 0).any() and (seen[0]["top"] < 0).any() and 0 < seen[0]["cover"].min() and seen[0]["cover"].max() < 1
