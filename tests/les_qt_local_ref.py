"""NumPy oracle of K19 (include/spc.h: spc_les_qt_local_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_qt_local_gpu.py (each takes an engine: tools/mutation_control.py --qtlocal hands them the engines of its mutant
libraries), the host twins of models.DeviceLESEnsemble's enable_qt_forcing() mode and an oracle-backed engine with
``les_qt_local`` for the CPU suite.

The oracle is the rule with a Python loop per (LES, level), one NumPy call per operation in the element type, so nothing fuses.
Every device array of the bodies is the LEADING part of a poisoned buffer (tests/les_harness.Poisoned); the bytes behind it (and
in front of a view off the 16-byte grid, and between pitched rows) are checked after the launch."""

import numpy
import torch

from sp_coupler_amd import _abi, driver, models, spcpl
from sp_coupler_amd import qt_forcing as qf
from tests import les_micro_ref as lmr
from tests import les_radiate_ref as lrr
from tests import les_vadvect_ref as lvr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, ensemble_case, fill_args, host_of, np_of, on_both, run_bodies, twin_kw)
from tests.test_vnudge import make_les_fields  # noqa: F401  (for the tests)

#: one cell per plane (c is 0 or N: nothing may change), planes smaller than the row-lanes of a workgroup (2 x 3), of 64 rows
#: (8 x 8: 4 or 16 rows per row-lane) and of 85 (17 x 5: the last round of loads is partial)
PLANES = [(1, 1), (2, 3), (8, 8), (17, 5)]
#: one level, one vector of doubles (2), less than one tile (7), one narrow tile and one more level (64, 65: 65 is odd, the
#: narrow path), the flagship's 160 (wide: 5 or 3 tiles, the last one partial in float32) and 161 (narrow: 3 tiles)
KTOTS = [1, 2, 7, 64, 65, 160, 161]
NS = [1, 2, 5]
SPLITS = [1, 2, 3]
CLASSES = ("pos_mixed", "neg_mixed", "neg_none", "neg_all", "zero", "negzero", "nan")
COUNT_FILL = -7
DT = 900.0


# -- the rule --------------------------------------------------------------------------------------------------------------
def les_qt_local(qt, ql, A, QTM):
    """(the new qt, count int32 [n x ktot]), new arrays: qt, ql [n x itot x jtot x ktot] of dtype T, A, QTM [n x ktot] of T"""
    T = qt.dtype.type
    assert all(x.dtype == qt.dtype for x in (ql, A, QTM))
    n, itot, jtot, ktot = qt.shape
    N = itot * jtot
    new = qt.copy()
    count = numpy.zeros((n, ktot), dtype=numpy.int32)
    with numpy.errstate(all="ignore"):
        for l in range(n):
            for k in range(ktot):
                a, m = A[l, k], QTM[l, k]
                if not (a > 0 or a < 0):                          # +0, -0, NaN
                    continue
                plane = qt[l, :, :, k]
                wet = plane > m if a > 0 else ql[l, :, :, k] > 0
                c = int(wet.sum())
                count[l, k] = c
                if c == 0 or c == N:
                    continue
                s = a * T(N)
                dw = s / T(c)
                dd = s / T(N - c)
                up = plane + dw
                dn = plane - dd
                assert up.dtype == qt.dtype and type(dw) is T
                new[l, :, :, k] = numpy.where(wet, up, dn)
    return new, count


def les_qt_local_vectorised(qt, ql, A, QTM):
    """the rule stated a second time, without a loop: (the new qt, count)"""
    T = qt.dtype.type
    N = qt.shape[1] * qt.shape[2]
    a, m = A[:, None, None, :], QTM[:, None, None, :]
    with numpy.errstate(all="ignore"):
        signed = (A > 0) | (A < 0)
        wet = numpy.where(a > 0, qt > m, (a < 0) & (ql > 0))
        c = wet.sum(axis=(1, 2))
        act = signed & (c > 0) & (c < N)
        s = A * T(N)
        dw = (s / c.astype(qt.dtype))[:, None, None, :]
        dd = (s / (N - c).astype(qt.dtype))[:, None, None, :]
        new = numpy.where(act[:, None, None, :], numpy.where(wet, qt + dw, qt - dd), qt)
    assert new.dtype == qt.dtype
    return new, numpy.where(signed, c, 0).astype(numpy.int32)


def classes(qt, ql, A, QTM):
    """object array [n x ktot]: the class of every level: pos_ / neg_ + mixed / none / all, zero, negzero, nan"""
    count = les_qt_local(qt, ql, A, QTM)[1]
    N = qt.shape[1] * qt.shape[2]
    out = numpy.empty(A.shape, dtype=object)
    for idx in numpy.ndindex(*A.shape):
        a, c = A[idx], int(count[idx])
        if a != a:
            out[idx] = "nan"
        elif a == 0:
            out[idx] = "negzero" if numpy.signbit(a) else "zero"
        else:
            out[idx] = ("pos_" if a > 0 else "neg_") + ("none" if c == 0 else "all" if c == N else "mixed")
    return out


# -- inputs ------------------------------------------------------------------------------------------------------------------
def case(shape, dtype, seed=0):
    """dict of the arguments in ``dtype`` (qt, ql, a, qtm) and the qsat profile ql was made with: qt a profile that decreases
    with height plus noise, qsat a profile that crosses it, A of random sign.  One level of every class of CLASSES is PLANTED
    (as many as there are levels, spread over them, the order rotated by ``seed``) and the builder asserts that what it hands
    out holds them; a plane of one cell cannot be mixed, its planted mixed levels come out as levels without a wet cell."""
    T = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    N = itot * jtot
    rng = numpy.random.default_rng(9000 + seed + 7 * ktot + N + 31 * n)
    base = 8e-3 * (1.0 - 0.5 * numpy.arange(ktot) / ktot)
    qt = (base + 2e-4 * rng.standard_normal(shape)).astype(T)
    qtm = qt.astype(numpy.float64).mean(axis=(1, 2)).astype(T)                  # (any QTM is legal; an ensemble hands in K10's means)
    qsat = (base + 1e-4 * rng.standard_normal((n, ktot))).astype(T)
    A = (rng.choice([-1.0, 1.0], (n, ktot)) * 2e-5 * (0.5 + rng.random((n, ktot)))).astype(T)
    levels = n * ktot
    planted = {}
    for i in range(min(len(CLASSES), levels)):
        flat = i if levels < len(CLASSES) else (i * levels) // len(CLASSES)
        planted[divmod(flat, ktot)] = CLASSES[(i + seed) % len(CLASSES)]
    for (l, k), cls in planted.items():
        plane = numpy.sort(qt[l, :, :, k], axis=None)
        mag = abs(A[l, k])
        if cls == "pos_mixed":
            A[l, k], qsat[l, k] = mag, qtm[l, k]                   # the cells above the mean are the cloudy ones
        elif cls == "neg_mixed":
            A[l, k], qsat[l, k] = -mag, plane[(N - 1) // 2]        # at least one cell above it, and the cell itself is dry
        elif cls == "neg_none":
            A[l, k], qsat[l, k] = -mag, plane[-1]
        elif cls == "neg_all":
            A[l, k], qsat[l, k] = -mag, T(0.5) * plane[0]
        else:
            A[l, k] = {"zero": T(0.0), "negzero": T(-0.0), "nan": T(numpy.nan)}[cls]
    ql = numpy.maximum(qt - qsat[:, None, None, :], T(0))
    c = dict(qt=qt, ql=ql, a=numpy.ascontiguousarray(A), qtm=numpy.ascontiguousarray(qtm), qsat=qsat, planted=planted)
    have = classes(qt, ql, A, qtm)
    for (l, k), cls in planted.items():
        want = cls.replace("mixed", "none") if N == 1 else cls
        assert have[l, k] == want, (shape, seed, (l, k), cls, have[l, k])
    assert len(planted) == min(len(CLASSES), levels) and all(x.dtype == T for x in (qt, ql, c["a"], c["qtm"]))
    return c


def oracle(c):
    return les_qt_local(c["qt"], c["ql"], c["a"], c["qtm"])


# -- device plumbing ---------------------------------------------------------------------------------------------------------
def _sync(eng):
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)


class Run:
    """one launch through ``eng.les_qt_local`` with every array inside a poisoned buffer; ``check`` compares qt and count with
    the oracle bit for bit, the read-only inputs with what was uploaded, and looks at the bytes around every array.  ``leads``:
    elements in front of (qt, ql); ``pad``: elements between the rows of a and qtm; ``pad_count``: between those of count"""

    def __init__(self, eng, c, leads=(0, 0), pad=0, pad_count=0, split=0):
        self.eng, self.c, self.pad, self.pad_count = eng, c, pad, pad_count
        self.mem = Poisoned(eng)
        put = self.mem.put
        rows = lambda tag, a, fill, extra: self.mem.rows(tag, a, fill, pad=extra)           # noqa: E731
        self.dqt = put("qt", c["qt"], float("nan"), leads[0])
        self.dql = put("ql", c["ql"], float("nan"), leads[1])
        self.da, self.dm = rows("a", c["a"], 1e30, pad), rows("qtm", c["qtm"], 1e30, pad)
        self.dcount = rows("count", numpy.full(c["a"].shape, COUNT_FILL, dtype=numpy.int32), COUNT_FILL, pad_count)
        self.got = eng.les_qt_local(self.dqt, self.dql, self.da, self.dm, count=self.dcount, split=split)
        _sync(eng)

    def check(self, what=""):
        c = self.c
        new, count = oracle(c)
        assert self.got.data_ptr() == self.dcount.data_ptr() and self.got.dtype == torch.int32
        assert_bits("%s qt" % what, self.dqt.cpu().numpy(), new)
        got = self.dcount.cpu().numpy()
        assert numpy.array_equal(got, count), (what, "count", got[got != count][:8], count[got != count][:8])
        for tag, t, a in (("ql", self.dql, c["ql"]), ("a", self.da, c["a"]), ("qtm", self.dm, c["qtm"])):
            assert Poisoned.read_only(t, a), (what, tag, "read only")
        self.mem.check_around(what)
        return new, count


PTRS = ("qt", "ql", "a", "qtm", "count")


def raw_launch(eng, c, alias=None, extents=None, null=()):
    """spc_les_qt_local_* itself: (rc, host qt, host count).  ``alias``: (member, key) pairs that replace a pointer member by
    that of tensor ``key``; ``extents``: overrides of the scalar members; ``null``: members set to NULL"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    n, itot, jtot, ktot = c["qt"].shape
    t = {k: dev(c[k]) for k in ("qt", "ql", "a", "qtm")}
    t["count"] = dev(numpy.full((n, ktot), COUNT_FILL, dtype=numpy.int32))
    a = _abi.LesQtLocalArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.split, a.pitch_prof, a.pitch_count = n, itot, jtot, ktot, 0, ktot, ktot
    fill_args(a, t, PTRS, alias, extents, null)
    rc = abi_call(eng, "spc_les_qt_local", a)
    assert Poisoned.read_only(t["ql"], c["ql"]) and Poisoned.read_only(t["a"], c["a"]) and Poisoned.read_only(t["qtm"], c["qtm"])
    return rc, t["qt"].cpu().numpy(), t["count"].cpu().numpy()


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """every class of level against the oracle; where a plane can be mixed the answer is not the input, else it is"""
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    new, count = Run(eng, c).check("n %d plane %s ktot %d" % (n, plane, ktot))
    N = plane[0] * plane[1]
    mixed = (count > 0) & (count < N)
    touched = (new != c["qt"]).any(axis=(1, 2))
    assert not touched[~mixed].any() and (N == 1 or mixed.any()) and (touched[mixed].all() if N > 1 else not touched.any())


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 2 x 3: A and QTM differ per LES, so a wrong l shows; with and without a pitch on the profiles and on count"""
    for n in NS:
        for pad, pad_count in ((0, 0), (3, 0), (0, 5), (3, 5)):
            c = case((n, 2, 3, ktot), np_of(eng), seed=1)
            if n > 1 and ktot > 1:
                assert not numpy.array_equal(c["a"][0], c["a"][1]) and not numpy.array_equal(c["qtm"][0], c["qtm"][1])
            Run(eng, c, pad=pad, pad_count=pad_count).check("rows n %d ktot %d pad %d %d" % (n, ktot, pad, pad_count))


def check_shapes(eng):
    """every forced split factor among 1, 2, 3 and one larger than the number of rows against the unforced launch, the oracle
    and each other: qt and count bit-equal; what the library chooses for the sizes of the benchmark"""
    for shape in ((3, 2, 3, 7), (2, 8, 8, 65), (1, 17, 5, 160), (2, 1, 1, 64)):
        c = case(shape, np_of(eng), seed=2)
        N = shape[1] * shape[2]
        free = Run(eng, c)
        free.check("split 0 %s" % (shape,))
        assert eng.qt_local_split(*shape) == 1
        for split in SPLITS + [N + 3]:
            r = Run(eng, c, split=split)
            r.check("split %d %s" % (split, shape))
            assert Poisoned.read_only(r.dqt, free.dqt.cpu().numpy()) and Poisoned.read_only(r.dcount, free.dcount.cpu().numpy()), (shape, split)
    assert eng.qt_local_split(256, 8, 8, 160) == 1 and eng.qt_local_split(16, 64, 64, 160) == 22 and eng.qt_local_split(1, 128, 128, 160) == 256
    assert eng.qt_local_split(0, 8, 8, 160) == 0 and eng.qt_local_split(4, 0, 8, 160) == 0 and eng.qt_local_split(4, 4097, 4097, 16) == 0
    c = case((2, 16, 16, 70), np_of(eng), seed=3)                   # the library's own choice of a split: 4 parts of 64 rows
    assert eng.qt_local_split(2, 16, 16, 70) == 4
    Run(eng, c).check("the library's split")


def skipped_case(dtype, ktot=21):
    """(case, the levels (l, k) that must keep every bit): -0.0, NaN and infinities in qt on levels of every untouched class
    (a zero, -0 and NaN; a < 0 without a wet cell and without a dry one; a > 0 under a QTM of +inf and of -inf), and on the
    mixed levels a NaN qt cell that is dry (a > 0), a NaN qt cell that is wet (a < 0) and a NaN ql cell (dry)"""
    c = case((3, 2, 3, ktot), dtype, seed=4)
    T = c["qt"].dtype.type
    inv = {v: k for k, v in c["planted"].items()}
    keep = [inv[k] for k in ("zero", "negzero", "nan", "neg_none", "neg_all")]
    free = [(l, k) for l in range(3) for k in range(ktot) if (l, k) not in c["planted"]]
    for (l, k), m in zip(free[:2], (numpy.inf, -numpy.inf)):     # a > 0: no cell above +inf, every cell above -inf
        c["a"][l, k], c["qtm"][l, k] = T(2e-5), T(m)
        keep.append((l, k))
    for n, (l, k) in enumerate(keep):
        vals = [-0.0, numpy.inf] + ([-numpy.inf, numpy.nan] if (l, k) != free[1] else [])      # (-inf and NaN are not above -inf: dry cells would mix that level)
        for j, v in enumerate(vals):
            c["qt"][l, (j + n) % 2, j % 3, k] = T(v)
    l, k = inv["pos_mixed"]
    c["qt"][l, 1, 2, k] = T(numpy.nan)
    l, k = inv["neg_mixed"]
    wet = numpy.argwhere(c["ql"][l, :, :, k] > 0)
    c["qt"][l, wet[0][0], wet[0][1], k] = T(numpy.nan)
    if len(wet) > 1:
        c["ql"][l, wet[1][0], wet[1][1], k] = T(numpy.nan)
    return c, keep


def check_skipped(eng):
    """untouched levels keep every BYTE of qt, special values included; a NaN qt cell on a mixed level stays NaN and counts as
    dry where qt decides; a NaN ql cell is dry"""
    for ktot in (21, 64):
        c, keep = skipped_case(np_of(eng), ktot)
        before = c["qt"].copy()
        r = Run(eng, c)
        new, count = r.check("skipped ktot %d" % ktot)
        got = r.dqt.cpu().numpy()
        for l, k in keep:
            assert _same_host(got[l, :, :, k], before[l, :, :, k]), (l, k)
        inv = {v: k for k, v in c["planted"].items()}
        l, k = inv["pos_mixed"]
        assert numpy.isnan(got[l, 1, 2, k]) and 0 < count[l, k] == int((before[l, :, :, k] > c["qtm"][l, k]).sum()) < 6
        l, k = inv["neg_mixed"]
        assert numpy.isnan(got[l, :, :, k]).sum() == 1 and 0 < count[l, k] == int((c["ql"][l, :, :, k] > 0).sum()) < 6
        mixed = (count > 0) & (count < 6)
        assert (numpy.isnan(got) == numpy.isnan(before)).all() and (got != before)[~numpy.isnan(before)].any() and mixed.sum() > 3


def ties_case(dtype, ktot=9):
    """cells that sit exactly ON the threshold are dry: qt == QTM on the planted a > 0 level, ql == +0 and -0 on the a < 0 one"""
    c = case((2, 2, 3, ktot), dtype, seed=5)
    inv = {v: k for k, v in c["planted"].items()}
    l, k = inv["pos_mixed"]
    plane = numpy.sort(c["qt"][l, :, :, k], axis=None)
    c["qtm"][l, k] = plane[2]                                      # three cells above, one on it, two below
    l, k = inv["neg_mixed"]
    dry = numpy.argwhere(c["ql"][l, :, :, k] == 0)
    c["ql"][l, dry[0][0], dry[0][1], k] = -0.0
    return c, inv


def check_ties(eng):
    c, inv = ties_case(np_of(eng))
    new, count = Run(eng, c).check("ties")
    l, k = inv["pos_mixed"]
    assert count[l, k] == 3 and (c["qt"][l, :, :, k] == c["qtm"][l, k]).sum() == 1
    l, k = inv["neg_mixed"]
    assert count[l, k] == (c["ql"][l, :, :, k] > 0).sum() < 6 - 1 and numpy.signbit(c["ql"][l, :, :, k]).any()


def check_alignment(eng, leads, ktot=65, pad=0):
    """views off the 16-byte grid: qt and ql equally or each on its own (the narrow path whatever ktot), and on it (wide)"""
    c = case((3, 2, 3, ktot), np_of(eng), seed=sum(leads) + 10 * pad)
    Run(eng, c, leads=leads, pad=pad, pad_count=pad).check("leads %s pad %d ktot %d" % (leads, pad, ktot))


def check_refusals(eng):
    """n = 0 is a no-op; N > 2^24, pitch_prof < ktot, pitch_count < ktot, a NULL qt, ql, a, qtm or count, qt == ql and a
    negative split are refused by the library; the engine refuses the same alias and bad shapes; no refused call writes"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=6)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    t = {k: dev(c[k]) for k in ("qt", "ql", "a", "qtm")}
    got = eng.les_qt_local(t["qt"][:0], t["ql"][:0], t["a"][:0], t["qtm"][:0])
    assert tuple(got.shape) == (0, 8) and got.dtype == torch.int32
    rc, qt, count = raw_launch(eng, c, extents=dict(n_les=0))
    assert rc == 0 and (count == COUNT_FILL).all()
    assert_bits("n = 0", qt, c["qt"])
    rc, qt, count = raw_launch(eng, c, extents=dict(n_les=0), null=PTRS)
    assert rc == 0
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    bad = [(dict(extents=dict(itot=4097, jtot=4097)), b"2^24"), (dict(extents=dict(pitch_prof=7)), b"pitch_prof"),
           (dict(extents=dict(pitch_count=7)), b"pitch_count"), (dict(extents=dict(split=-1)), b"split"),
           (dict(alias=(("ql", "qt"),)), b"same array"), (dict(alias=(("qt", "ql"),)), b"same array"),
           (dict(extents=dict(ktot=0)), b">= 1"), (dict(extents=dict(n_les=-1)), b"n_les")]
    bad += [(dict(null=(k,)), b"required pointer " + k.encode()) for k in PTRS]
    for kw, text in bad:
        rc, qt, count = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        assert_bits("refused: qt", qt, c["qt"])
        assert (count == COUNT_FILL).all()
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    args = (t["qt"], t["ql"], t["a"], t["qtm"])
    for call in (lambda: eng.les_qt_local(t["qt"], t["qt"], t["a"], t["qtm"]),
                 lambda: eng.les_qt_local(*args, split=-2),
                 lambda: eng.les_qt_local(t["qt"], t["ql"][:1], t["a"], t["qtm"]),
                 lambda: eng.les_qt_local(t["qt"], t["ql"], t["a"][:, :4], t["qtm"]),
                 lambda: eng.les_qt_local(t["qt"], t["ql"], t["a"], t["qtm"][:1]),
                 lambda: eng.les_qt_local(t["qt"][..., ::2], t["ql"][..., ::2], t["a"][:, :4], t["qtm"][:, :4]),
                 lambda: eng.les_qt_local(t["qt"].to(other), *args[1:]),
                 lambda: eng.les_qt_local(*args, count=torch.zeros(2, 8, dtype=torch.int64, device=eng.device)),
                 lambda: eng.les_qt_local(*args, count=torch.zeros(2, 7, dtype=torch.int32, device=eng.device)),
                 lambda: eng.les_qt_local(t["qt"].cpu(), *args[1:])):
        try:
            call()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    _sync(eng)
    assert_bits("refused: qt", t["qt"].cpu().numpy(), c["qt"])
    assert_bits("refused: ql", t["ql"].cpu().numpy(), c["ql"])


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    c = case((n, 2, 3, 40), np_of(one), seed=n)
    new, count = oracle(c)
    for tag, eng, up in on_both(one, multi, n):
        t = {k: up(c[k]) for k in ("qt", "ql", "a", "qtm")}
        got = eng.les_qt_local(t["qt"], t["ql"], t["a"], t["qtm"])
        multi.synchronize()
        assert_bits("%s qt" % tag, host_of(t["qt"]), new)
        assert numpy.array_equal(host_of(got), count), tag
        assert _same_host(host_of(t["ql"]), c["ql"])
    return blocks_of(t["qt"], multi, n)


def _same_host(a, b):
    return numpy.array_equal(numpy.ascontiguousarray(a).view(numpy.uint8), numpy.ascontiguousarray(b).view(numpy.uint8))


BODIES = ("parity", "rows", "shapes", "skipped", "ties", "alignment", "refusals")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (1, 2, 7, 65, 160)]),
            ("rows", lambda: [check_rows(eng, k) for k in (2, 65)]),
            ("shapes", lambda: check_shapes(eng)),
            ("skipped", lambda: check_skipped(eng)),
            ("ties", lambda: check_ties(eng)),
            ("alignment", lambda: [check_alignment(eng, *a) for a in (((1, 1), 65, 0), ((1, 0), 64, 0), ((3, 3), 160, 5), ((0, 0), 160, 0))]),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_qt_local (CPU suite) ---------------------------------------------------------------------
class QtLocalOracleEngine(lrr.RadiateOracleEngine):
    """tests/les_radiate_ref.RadiateOracleEngine with ``les_qt_local`` by the NumPy oracle above: qt updated in place, the counts
    written into the caller's tensor or a new one, as the HIP engine does"""

    def les_qt_local(self, qt, ql, a, qtm, *, count=None, split=0, **kw):
        if qt.shape[0] and qt.data_ptr() == ql.data_ptr():
            raise ValueError("qt and ql are the same tensor")
        new, c = les_qt_local(qt.numpy(), ql.numpy(), numpy.ascontiguousarray(a.numpy()), numpy.ascontiguousarray(qtm.numpy()))
        qt.copy_(torch.from_numpy(new))
        if count is None:
            return torch.from_numpy(c)
        count.copy_(torch.from_numpy(c))
        return count


# -- the host twins of models.DeviceLESEnsemble after enable_qt_forcing() --------------------------------------------------------
class _HostQtLocal:
    """NumPy fields: the executable definition of what evolve_model_batched does after enable_qt_forcing(), on top of any of the
    other modes: the step, QL and the means of the stepped fields, K19 on QT with that QL and those means, then everything the
    twin below does behind its own step (which finds no tendency left to apply)"""

    qt_forcing_kind = None
    _counts = None
    STEP_KEYS = ("U", "V", "THL", "QT")

    def enable_qt_forcing(self, kind):
        if kind not in qf.KINDS or "QT" not in self.fields3d or not (self.THERMO or "Qsat" in self.fields3d):
            raise ValueError("the local QT forcing (K19) needs a kind of %s, a QT field and a Qsat field or enable_thermo()" % (qf.KINDS,))
        if kind != self.qt_forcing_kind:
            self.qt_forcing_kind, self._counts = kind, None

    def get_qt_forcing_counts_batched(self):
        return self._counts if self.qt_forcing_kind else None

    def evolve_model_batched(self, t):
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        kind = self.qt_forcing_kind
        if kind is None or {"local": "QL", "strong": "QL_ref"}[kind] not in self.tend:
            return super().evolve_model_batched(t)
        f, p = self.fields3d, self.p
        self._step(dt, self.STEP_KEYS)
        self._follow()                                            # QL and the means of the stepped fields
        a = qf.increments(kind, self.tend.get("QL"), self.tend.get("QL_ref"), p["QL"], dt)
        f["QT"], self._counts = les_qt_local(f["QT"], f["QL"], self._r(a), numpy.ascontiguousarray(slab_ref.slab_means(f["QT"])))
        stepped = {k: self.tend.pop(k) for k in self.STEP_KEYS if k in self.tend}
        try:
            super().evolve_model_batched(t)                       # (its step finds nothing to add; QL and the means follow the new QT)
        finally:
            self.tend.update(stepped)


class HostQtLocalLESEnsemble(_HostQtLocal, lrr.HostRadiateLESEnsemble):
    """without enable_thermo(): QL = max(QT - Qsat, 0)"""


class HostThermoQtLocalLESEnsemble(_HostQtLocal, lrr.HostThermoRadiateLESEnsemble):
    """after enable_thermo(): K12's oracle before and after K19"""


VARIANTS = {"plain": dict(), "all": dict(diffuse=True, thermo=True, micro=True, vertical=True, radiate=True)}


def ensemble_run(engine, n, device, kind="local", thermo=False, micro=False, diffuse=False, vertical=False, radiate=False, itot=4, jtot=5,
                 nL=20, steps=3):
    """tests/les_radiate_ref.ensemble_run with enable_qt_forcing(kind) (``kind`` None: never called) and the cloud-water
    forcing and reference profile of the coupler handed over: ``steps`` calls of evolve_model_batched and one variability nudge
    (constantT) before the last; after each of them every profile, the fields and the counts.  Returns (ens, list of records)"""
    def enable(ens):
        if kind:
            ens.enable_qt_forcing(kind)
            ens.enable_qt_forcing(kind)                           # (idempotent)

    def record(ens, rec):
        if kind:
            counts = ens.get_qt_forcing_counts_batched()
            rec["counts"] = numpy.zeros((n, nL)) if counts is None else numpy.array(host_of(counts), dtype=numpy.float64)

    def before(ens):
        assert not kind or ens.get_qt_forcing_counts_batched() is None
    return ensemble_case(engine, n, models.DeviceLESEnsemble if device else (HostThermoQtLocalLESEnsemble if thermo else HostQtLocalLESEnsemble),
                         thermo=thermo, micro=micro, diffuse=diffuse, edit=lvr.raise_u if vertical else None,
                         advection=dict(dx=lvr.DX, dy=1.5 * lvr.DX, vertical=True) if vertical else None,
                         radiation=lrr.radiation_of(n, "f0", "kappa") if radiate else None, enable=enable,
                         forcings=lambda rng, stack: dict(QL=rng.normal(0, 2e-8, (n, nL)), QLp=stack("ql_ref") * (0.5 + rng.random((n, nL)))),
                         record=record, before=before, itot=itot, jtot=jtot, nL=nL, steps=steps)


def check_ensemble(one, engines, n, variant, kind):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``; the QT field of the twin's first
    step differs from the same run without enable_qt_forcing() on levels the counts call mixed, its slab means follow that run
    to rounding where nothing else acts on QT, and the device run without the call is bit-equal to its twin as well"""
    kw = VARIANTS[variant]
    host = ensemble_run(one, n, False, kind=kind, **kw)[1]
    plain = ensemble_run(one, n, False, kind=None, **kw)[1]
    N = host[1]["field QT"].shape[1] * host[1]["field QT"].shape[2]
    mixed = (host[1]["counts"] > 0) & (host[1]["counts"] < N)
    assert mixed.any() and not numpy.array_equal(host[1]["field QT"], plain[1]["field QT"])
    if variant == "plain":
        touched = (host[1]["field QT"] != plain[1]["field QT"]).any(axis=(1, 2))
        assert numpy.array_equal(touched, mixed)
        scale = numpy.finfo(host[1]["field QT"].dtype).eps / numpy.finfo(numpy.float64).eps          # (the same count of roundings, of T)
        numpy.testing.assert_allclose(host[1]["p QT"], plain[1]["p QT"], rtol=1e-13 * scale, atol=0)
    for engine in engines:
        lmr.same_logs(host, ensemble_run(engine, n, True, kind=kind, **kw)[1])
    lmr.same_logs(plain, ensemble_run(engines[0], n, True, kind=None, **kw)[1])
    return host


# -- the coupler: Coupler(qt_forcing="local" | "strong") on an ensemble that offers enable_qt_forcing -----------------------------
def coupler_run(engine, cls, qt_forcing, n=4, nG=19, nL=24, itot=4, jtot=4):
    """tests/device_fields_multi._loop with another qt_forcing: the initial state, one spin-up step and one coupled step; the
    profiles, the QT and QL fields and the counts after each.  Returns (ens, log)"""
    spcpl.set_engine(engine)
    gcm = models.BatchedSyntheticGCM(n + 7, nG, 3)
    ens = cls.for_gcm(gcm, numpy.arange(1, 2 * n + 1, 2), nL=nL, seed=4, itot=itot, jtot=jtot, **twin_kw(cls, engine))
    rng = numpy.random.default_rng(8)
    ens.attach_fields({"Qsat": ens.p["QT"][:, None, None, :] * (1.0 + 2e-3 * rng.normal(size=(n, itot, jtot, nL)))})
    cpl = driver.Coupler(gcm, ens, cplsurf=True, qt_forcing=qt_forcing)
    numpy.random.seed(42)
    cpl.init_les_state()
    log = []

    def record():
        rec = {"p " + k: numpy.array(v) for k, v in ens.p.items()}
        rec.update({"field " + k: numpy.array(host_of(ens.get_fields_batched(k))) for k in ("QT", "QL")})
        counts = ens.get_qt_forcing_counts_batched()
        rec["counts"] = numpy.zeros((n, nL)) if counts is None else numpy.array(host_of(counts), dtype=numpy.float64)
        rec["ql_ref"] = numpy.array(ens.tend["QL_ref"])
        rec["f_ql"] = numpy.array(ens.tend["QL"])
        log.append(rec)
    cpl.run_spinup(900.0, 1)
    record()
    cpl.step()
    record()
    return ens, log


def check_coupler(engine, cls, kinds=qf.KINDS):
    """Coupler(qt_forcing=kind) enables the mode of an ensemble that offers it; its first step moves QT inside the planes the
    counts call mixed and nowhere else, the slab-mean QT follows the "sp" run to rounding and the slab-mean cloud water moves
    with the sign of the forcing in sum and on most mixed levels.  Returns {qt_forcing: log}"""
    ens, sp = coupler_run(engine, cls, "sp")
    assert ens.qt_forcing_kind is None and not sp[0]["counts"].any()
    logs = {"sp": sp}
    for kind in kinds:
        ens, log = coupler_run(engine, cls, kind)
        assert ens.qt_forcing_kind == kind
        N = ens.itot * ens.jtot
        first = log[0]
        mixed = (first["counts"] > 0) & (first["counts"] < N)
        touched = (first["field QT"] != sp[0]["field QT"]).any(axis=(1, 2))
        assert mixed.any() and numpy.array_equal(touched, mixed), kind
        numpy.testing.assert_allclose(first["p QT"], sp[0]["p QT"], rtol=1e-13, atol=0)
        a = first["f_ql"] * 900.0 if kind == "local" else first["ql_ref"] - sp[0]["p QL"]      # ("sp": the QL of the stepped fields)
        moved = (first["p QL"] - sp[0]["p QL"]) * numpy.sign(a)
        # (not on EVERY level: where a < 0 and few cells are dry, each of them takes a large share and can turn cloudy itself)
        assert moved[mixed].sum() > 0 and (moved[mixed] > 0).sum() > 2 * (moved[mixed] < 0).sum() and not moved[~mixed].any(), kind
        assert not numpy.array_equal(log[1]["field QT"], sp[1]["field QT"])
        logs[kind] = log
    return logs
