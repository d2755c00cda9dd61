"""NumPy oracle of K11 (include/spc.h: spc_les_advance_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_advance_gpu.py (each takes an engine: tools/mutation_control.py hands them the engines of its mutant
libraries) and an oracle-backed engine with ``les_advance`` for the CPU suite.

Every device array of the bodies is the LEADING part of a poisoned buffer (tests/les_harness.Poisoned); the bytes behind it
(and in front of a view off the 16-byte grid) are checked after the launch."""
import numpy
import torch

from tests import slab_ref
from tests.fake_engine import OracleEngine, _t
from tests.gpu_util import assert_bits
from tests.les_harness import DTYPES, NP, Poisoned, blocks_of, chain_cases, np_of, on_both, run_bodies  # noqa: F401  (DTYPES, NP: for the tests)

SHAPES = [(1, 1, 1, 2), (3, 3, 3, 5), (2, 5, 7, 64), (2, 4, 4, 66), (1, 9, 1, 130), (2, 8, 8, 160)]
#: itot * jtot = 1 ... 17: every remainder of the row look-ahead (batches of 8 rows, of 4 for the lanes of QT), one, two and
#: more whole batches, with and without single rows behind them
PLANES = [(1, 1), (2, 1), (3, 1), (2, 2), (5, 1), (3, 2), (1, 7), (4, 2), (3, 3), (2, 5), (11, 1), (4, 3), (1, 13), (7, 2), (5, 3),
          (4, 4), (17, 1)]
NAMES = ("U", "V", "THL", "QT", "E", "F", "G", "H")


# -- the rule --------------------------------------------------------------------------------------------------------------
def saturate(qt, qsat):
    """q of the rule: d > 0 ? d : (d != d ? d : +0.0) -- NaN stays NaN; -0.0 and negatives give +0.0"""
    with numpy.errstate(invalid="ignore"):
        d = qt - qsat
        return numpy.where(d > 0, d, numpy.where(d != d, d, d.dtype.type(0.0)))


def mean_rows(field):
    """[n x itot x jtot x ktot] -> [n x ktot] by k_slab_means' rule for ktot >= 2, spelled out (tests/slab_ref.py)"""
    with numpy.errstate(invalid="ignore", over="ignore"):
        return numpy.stack([slab_ref.sequential_mean(f) for f in field]) if len(field) else numpy.empty((0, field.shape[-1]), field.dtype)


def les_advance(fields, tend, dt, qsat=None, sat=None):
    """(new fields, q or None, means): fields dict name -> [n x itot x jtot x ktot] of ONE dtype T (not modified), tend dict
    name -> [n x ktot]; dt is rounded to T once; means holds "QL" (of q) when sat is given"""
    new, means, q = {}, {}, None
    for name, x in fields.items():
        T = x.dtype.type
        assert x.shape[-1] >= 2, "ktot == 1 is not K11's"
        if name in tend:
            with numpy.errstate(invalid="ignore", over="ignore"):
                inc = (tend[name].astype(x.dtype) * T(dt)).astype(x.dtype)
                x = (x + inc[:, None, None, :]).astype(x.dtype)
        new[name] = x
        means[name] = mean_rows(x)
    if sat is not None:
        q = saturate(new[sat], qsat).astype(new[sat].dtype)
        means["QL"] = mean_rows(q)
    return new, q, means


# -- inputs ------------------------------------------------------------------------------------------------------------------
def case(shape, dtype, n_fields=4, seed=0, sat=True):
    """fields of different magnitudes (the summation order and the two roundings of the update are visible in all of them),
    tendencies for all of them, and a qsat that leaves about half of the cells cloudy"""
    rng = numpy.random.default_rng(1000 + seed + 7 * shape[-1] + shape[1] * shape[2])
    n, ktot = shape[0], shape[-1]
    fields = {name: (rng.standard_normal(shape) * 3 + 1 + j).astype(dtype) for j, name in enumerate(NAMES[:n_fields])}
    tend = {name: (rng.standard_normal((n, ktot)) * 1e-3).astype(dtype) for name in fields}
    qsat = None
    if sat and "QT" in fields:
        fields["QT"] = (numpy.abs(fields["QT"]) * dtype(1e-3)).astype(dtype)
        tend["QT"] = (tend["QT"] * dtype(1e-3)).astype(dtype)
        qsat = (fields["QT"] * (1 + 0.3 * rng.standard_normal(shape))).astype(dtype)
    return fields, tend, qsat


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one launch through ``eng.les_advance`` with every array inside a poisoned buffer; ``check`` compares fields, ql and
    means with the oracle bit for bit and looks at the bytes around every array"""

    def __init__(self, eng, fields, tend, dt, qsat=None, sat=None, want_ql=True, ql_mean=True, lead=0, pad=0, lead_rows=0):
        self.eng, self.host, self.tend, self.dt, self.qsat, self.sat = eng, fields, tend, dt, qsat, sat
        self.lead, self.pad, self.lead_rows = lead, pad, lead_rows
        dtype = next(iter(fields.values())).dtype
        shape = next(iter(fields.values())).shape
        n, ktot = shape[0], shape[-1]
        self.mem = Poisoned(eng)
        put = self.mem.put
        rows = lambda tag, a, poison, lead: self.mem.rows(tag, a, poison, lead, pad)        # noqa: E731
        self.dev = {k: put("field " + k, v, float("nan"), lead) for k, v in fields.items()}
        self.dtend = {k: rows("tend " + k, v, 1e30, lead_rows) for k, v in tend.items()}
        self.dmeans = {k: rows("mean " + k, numpy.full((n, ktot), -1.0, dtype), -7.0, lead_rows)
                       for k in list(fields) + (["QL"] if sat is not None and ql_mean else [])}
        self.dqsat = put("qsat", qsat, float("nan"), lead) if sat is not None else None
        self.dql = put("ql", numpy.full(shape, -3.0, dtype), -5.0, lead) if sat is not None and want_ql else None
        self.got = eng.les_advance(self.dev, self.dtend, dt, qsat=self.dqsat, sat=sat, ql=self.dql, means=self.dmeans, ql_mean=ql_mean)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        new, q, means = les_advance(self.host, self.tend, self.dt, self.qsat, self.sat)
        assert sorted(self.got) == sorted(self.dmeans), (what, sorted(self.got))
        for k, v in new.items():
            assert_bits("%s field %s" % (what, k), self.dev[k].cpu().numpy(), v)
        if self.dql is not None:
            assert_bits("%s ql" % what, self.dql.cpu().numpy(), q)
        if self.dqsat is not None:
            assert_bits("%s qsat (read only)" % what, self.dqsat.cpu().numpy(), self.qsat)
        for k, t in self.dmeans.items():
            assert self.got[k].data_ptr() == t.data_ptr(), (what, k)
            assert_bits("%s mean %s" % (what, k), t.cpu().numpy(), means[k])
        for k, v in self.tend.items():
            assert_bits("%s tend %s (read only)" % (what, k), self.dtend[k].cpu().numpy(), v)
        self.check_surroundings(what)
        return new, q, means

    def check_surroundings(self, what=""):
        self.mem.check_around(what)


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, shape, dt=900.0):
    """every field, ql and every mean against the oracle; the step changed every field and every mean"""
    fields, tend, qsat = case(shape, np_of(eng))
    new, q, means = Run(eng, fields, tend, dt, qsat, "QT").check(str(shape))
    for k in fields:
        assert (new[k] != fields[k]).any() and (means[k] != mean_rows(fields[k])).any(), k
    if q.size >= 100:
        assert (q > 0).any() and (q == 0).any()


def check_planes(eng, ktot):
    """itot * jtot = 1 ... 17: whole batches of the look-ahead, single rows behind them, fewer rows than one batch.
    ktot picks the instantiation (160: 16-byte accesses; 33: one element per lane)"""
    for plane in PLANES:
        fields, tend, qsat = case((2,) + plane + (ktot,), np_of(eng), n_fields=2, seed=3)
        fields = {"THL": fields["U"], "QT": numpy.abs(fields["V"])}
        tend = {"THL": tend["U"], "QT": tend["V"]}
        qsat = (fields["QT"] * np_of(eng)(1.01)).astype(np_of(eng))
        qsat[:, ::2] = fields["QT"][:, ::2] * np_of(eng)(0.75)
        Run(eng, fields, tend, 60.0, qsat, "QT").check("plane %s ktot %d" % (plane, ktot))


def check_alignment(eng, lead, lead_rows, pad):
    """views off the 16-byte grid (``lead`` elements into the buffers of the 3-D arrays, ``lead_rows`` into those of the
    tendencies and means) and pitched tendencies / means (``pad`` elements between the rows)"""
    fields, tend, qsat = case((3, 5, 7, 160), np_of(eng), seed=lead + 10 * lead_rows + 100 * pad)
    Run(eng, fields, tend, 300.0, qsat, "QT", lead=lead, lead_rows=lead_rows, pad=pad).check("lead %d %d pad %d" % (lead, lead_rows, pad))


def check_optional(eng):
    """a subset of tendencies missing (those fields keep their bits, -0.0 included); no saturation; ql without its mean and
    the mean without ql; 1 and 8 fields"""
    dtype = np_of(eng)
    fields, tend, qsat = case((2, 5, 7, 64), dtype, seed=5)
    fields["U"][0, 0, 0, :8] = -0.0                              # a field without a tendency is not touched: -0.0 + 0.0 would be +0.0
    fields["U"][1, 3, 3, 5] = numpy.nan
    part = {k: tend[k] for k in ("V", "QT")}
    new, _, _ = Run(eng, fields, part, 900.0, qsat, "QT").check("subset")
    assert_bits("U untouched", new["U"], fields["U"])
    assert_bits("THL untouched", new["THL"], fields["THL"])
    assert (new["V"] != fields["V"]).any()
    new, _, _ = Run(eng, fields, {}, 900.0, qsat, "QT").check("no tendency at all")
    assert all(numpy.array_equal(new[k], fields[k], equal_nan=True) for k in fields)
    r = Run(eng, fields, tend, 900.0)
    r.check("sat_field = -1")
    assert "QL" not in r.got
    r = Run(eng, fields, tend, 900.0, qsat, "QT", want_ql=False)
    r.check("ql NULL, its mean wanted")
    assert "QL" in r.got
    r = Run(eng, fields, tend, 900.0, qsat, "QT", ql_mean=False)
    r.check("ql wanted, its mean not")
    assert "QL" not in r.got and r.dql is not None
    one, t1, _ = case((3, 3, 3, 5), dtype, n_fields=1, seed=6)
    Run(eng, one, t1, 10.0).check("one field")
    Run(eng, {"QT": numpy.abs(one["U"])}, {"QT": t1["U"]}, 10.0, (numpy.abs(one["U"]) * dtype(0.9)).astype(dtype), "QT").check("one field, QT")
    eight, t8, qs8 = case((2, 4, 4, 66), dtype, n_fields=8, seed=7)
    Run(eng, eight, t8, 10.0, qs8, "QT").check("eight fields")
    try:
        eng.les_advance({str(i): r.dev["U"] for i in range(9)}, {}, 1.0)
    except ValueError as e:
        assert "8" in str(e)
    else:
        raise AssertionError("nine fields were not refused")


def special_case(dtype):
    """qt - qsat equal to -0.0, +0.0, NaN and negative, level by level, and nothing else in the field's first LES; a tendency of
    -0.0 and one of NaN in single levels"""
    shape = (2, 3, 5, 12)
    rng = numpy.random.default_rng(77)
    qt = (rng.random(shape) * 1e-2 + 1e-3).astype(dtype)
    qsat = (qt * dtype(0.5)).astype(dtype)
    qt[:, :, :, 0], qsat[:, :, :, 0] = -0.0, 0.0                 # d = -0.0 - +0.0 = -0.0
    qt[:, :, :, 1], qsat[:, :, :, 1] = 0.0, 0.0                  # d = +0.0
    qsat[:, :, :, 2] = qt[:, :, :, 2]                            # d = +0.0 after the update (tendency 0 at this level)
    qsat[:, 1, 2, 3] = numpy.nan                                 # d = NaN
    qt[:, 2, 2, 4] = numpy.nan
    qsat[:, :, :, 5] = qt[:, :, :, 5] * dtype(2)                 # d < 0 everywhere
    qsat[:, :, :, 6] = numpy.inf                                 # d = -inf
    tend = (rng.standard_normal((2, 12)) * 1e-7).astype(dtype)
    tend[:, :3] = 0.0
    tend[:, 5] = 0.0
    tend[:, 0] = -0.0                                            # inc = -0.0: -0.0 + -0.0 stays -0.0
    tend[:, 8] = numpy.nan                                       # one level of NaN: its neighbours 7 and 9 stay finite
    thl = (rng.standard_normal(shape) + 300).astype(dtype)
    thl[:, :, :, 1] = -0.0
    tthl = numpy.zeros((2, 12), dtype=dtype)
    tthl[:, 1] = -0.0
    tthl[:, 7] = numpy.nan
    return {"THL": thl, "QT": qt}, {"THL": tthl, "QT": tend}, qsat


def check_special(eng):
    fields, tend, qsat = special_case(np_of(eng))
    new, q, means = Run(eng, fields, tend, 900.0, qsat, "QT").check("special values")
    # what the oracle itself says to these inputs is asserted in tests/test_les_advance_cpu.py; here: the levels next to a
    # NaN tendency stay finite on the device (the oracle's answer, compared above, has them finite)
    assert numpy.isnan(new["QT"][:, :, :, 8]).all() and numpy.isfinite(new["QT"][:, :, :, [7, 9]]).all()
    assert numpy.isnan(means["THL"][:, 7]).all() and numpy.isfinite(means["THL"][:, [6, 8]]).all()
    neg = (fields["QT"] * np_of(eng)(3)).astype(np_of(eng))
    new, q, means = Run(eng, fields, {k: numpy.zeros_like(v) for k, v in tend.items()}, 900.0, numpy.abs(numpy.nan_to_num(neg)) + np_of(eng)(1), "QT").check("negative everywhere")
    assert (q[~numpy.isnan(q)] == 0).all() and not numpy.signbit(q[~numpy.isnan(q)]).any()


def check_multi(one, multi, n, min_rows_expected=None):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    dtype = np_of(one)
    fields, tend, qsat = case((n, 6, 5, 40), dtype, seed=n)
    want_new, want_q, want_means = les_advance(fields, tend, 450.0, qsat, "QT")
    (_, _, dev), (_, _, sh) = on_both(one, multi, n)
    f1 = {k: dev(v) for k, v in fields.items()}
    ql1 = torch.full_like(f1["QT"], -3.0)
    m1 = one.les_advance(f1, {k: dev(v) for k, v in tend.items()}, 450.0, qsat=dev(qsat), sat="QT", ql=ql1)
    fm = {k: sh(v) for k, v in fields.items()}
    qlm = sh(numpy.full(qsat.shape, -3.0, dtype=dtype))
    mm = multi.les_advance(fm, {k: sh(v) for k, v in tend.items()}, 450.0, qsat=sh(qsat), sat="QT", ql=qlm)
    multi.synchronize()
    blocks = blocks_of(fm["QT"], multi, n)
    for k in fields:
        assert_bits("multi field " + k, fm[k].to_host(), want_new[k])
        assert_bits("one field " + k, f1[k].cpu().numpy(), want_new[k])
    assert_bits("multi ql", qlm.to_host(), want_q)
    assert_bits("one ql", ql1.cpu().numpy(), want_q)
    assert sorted(mm) == sorted(m1) == sorted(want_means)
    for k in want_means:
        assert_bits("multi mean " + k, mm[k].to_host(), want_means[k])
        assert_bits("one mean " + k, m1[k].cpu().numpy(), want_means[k])
    return blocks


def check_chain(eng):
    """the cases of the lane's walk (les_harness.chain_cases) for batches of 8 rows, which hold those of the 4 rows of the lanes
    of QT: a field with one input stream and QT with its two, every array in poison"""
    dtype = np_of(eng)
    for shape, lead in chain_cases(8, dtype):
        fields, tend, _ = case(shape, dtype, n_fields=2, seed=9)
        fields = {"THL": fields["U"], "QT": numpy.abs(fields["V"])}
        tend = {"THL": tend["U"], "QT": tend["V"]}
        qsat = (fields["QT"] * dtype(1.01)).astype(dtype)
        qsat[..., ::2] = fields["QT"][..., ::2] * dtype(0.75)
        Run(eng, fields, tend, 60.0, qsat, "QT", lead=lead, lead_rows=lead).check("chain %s lead %d" % (shape, lead))


BODIES = ("parity", "planes", "alignment", "optional", "special", "chain")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, s) for s in SHAPES]),
            ("planes", lambda: [check_planes(eng, k) for k in (160, 33)]),
            ("alignment", lambda: [check_alignment(eng, *a) for a in ((1, 0, 0), (0, 1, 0), (0, 0, 4), (0, 0, 3))]),
            ("optional", lambda: check_optional(eng)),
            ("special", lambda: check_special(eng)),
            ("chain", lambda: check_chain(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_advance (CPU suite) ------------------------------------------------------------------
class AdvanceOracleEngine(OracleEngine):
    """tests/fake_engine.OracleEngine with ``les_advance`` by the NumPy oracle above: fields and ql updated in place, as the
    HIP engine does"""

    def les_advance(self, fields, tend, dt, qsat=None, sat=None, ql=None, means=None, ql_mean=True, **kw):
        new, q, m = les_advance({k: v.numpy() for k, v in fields.items()}, {k: v.numpy() for k, v in tend.items()}, dt,
                                None if qsat is None else qsat.numpy(), sat)
        for k, v in new.items():
            fields[k].copy_(torch.from_numpy(v))
        if ql is not None:
            ql.copy_(torch.from_numpy(q))
        if sat is not None and not ql_mean:
            del m["QL"]
        return _t(m, means)
