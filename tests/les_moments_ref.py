"""NumPy oracle of K20 (include/spc.h: spc_les_moments_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_moments_gpu.py (each takes an engine: tools/mutation_control.py --moments hands them the engines of its mutant
libraries), the host twin of models.DeviceLESEnsemble's get_statistics() and an oracle-backed engine with ``les_moments`` for
the CPU suite.

The oracle is the rule with a literal Python loop over (i, j), one NumPy call per operation in the element type, so nothing
fuses.  Every device array of the bodies is the LEADING part of a poisoned buffer (tests/slab_edges.with_tail); the bytes behind
it (and in front of a view off the 16-byte grid, and between pitched rows) are checked after the launch, and the inputs are
compared with what was uploaded."""

import numpy
import torch

from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import statistics as st
from tests import les_qt_local_ref as qlr
from tests import slab_edges
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, chain_cases, host_of, np_of, on_both, run_bodies)

#: one row (every deviation is zero), fewer rows than the loads in flight (2 x 3), whole rounds of loads (8 x 8: 64 rows) and a
#: ragged last round (17 x 5: 85 rows)
PLANES = [(1, 1), (2, 3), (8, 8), (17, 5)]
#: one vector of doubles (2), less than one vector of floats (7: narrow), one wave of single levels and one more (64, 65: 65 is
#: odd, the narrow path), the flagship's 160 (wide) and 161 (narrow)
KTOTS = [2, 7, 64, 65, 160, 161]
NS = [1, 2, 5]
KINDS = ("mean", "var", "std")
NAMES = ("A", "B", "C", "D", "E", "F", "G", "H")
POISON = -7.5e30


# -- the oracle ----------------------------------------------------------------------------------------------------------------
def centre(x):
    """a field given at the upper faces brought to the cell centres along its last axis: 0.5 * (x[k - 1] + x[k]), x[-1] = +0.0"""
    below = numpy.concatenate([numpy.zeros_like(x[..., :1]), x[..., :-1]], axis=-1)
    s = below + x
    return x.dtype.type(0.5) * s


def les_moments(fields, pairs=(), face=None):
    """the rule of include/spc.h: ``fields`` name -> [n x itot x jtot x ktot] of one dtype; returns {"mean": {name: [n x ktot]},
    "var": ..., "std": ..., "cov": {(a, b): ...}} in that dtype"""
    x = {k: (centre(v) if k == face else v) for k, v in fields.items()}
    first = next(iter(x.values()))
    T = first.dtype.type
    n, itot, jtot, ktot = first.shape
    N = T(itot * jtot)
    with numpy.errstate(all="ignore"):
        mean = {}
        for k, v in x.items():
            acc = numpy.zeros((n, ktot), dtype=T)
            for i in range(itot):
                for j in range(jtot):
                    acc = acc + v[:, i, j, :]
            mean[k] = acc / N

        def second(a, b):
            acc = numpy.zeros((n, ktot), dtype=T)
            for i in range(itot):
                for j in range(jtot):
                    da = x[a][:, i, j, :] - mean[a]
                    db = x[b][:, i, j, :] - mean[b]
                    q = da * db
                    acc = acc + q
            return acc / N
        var = {k: second(k, k) for k in x}
        std = {k: numpy.sqrt(v) for k, v in var.items()}
        cov = {(a, b): second(a, b) for a, b in pairs}
    for d in (mean, var, std, cov):
        assert all(v.dtype == first.dtype for v in d.values())
    return {"mean": mean, "var": var, "std": std, "cov": cov}


def les_moments_vectorised(fields, pairs=(), face=None):
    """the same through ndarray.mean, ndarray.var and ndarray.std of every LES's [itot x jtot x ktot] block"""
    x = {k: (centre(v) if k == face else v) for k, v in fields.items()}
    n = next(iter(x.values())).shape[0]
    with numpy.errstate(all="ignore"):
        res = {"mean": {k: numpy.stack([v[l].mean(axis=(0, 1)) for l in range(n)]) for k, v in x.items()},
               "var": {k: numpy.stack([v[l].var(axis=(0, 1)) for l in range(n)]) for k, v in x.items()},
               "std": {k: numpy.stack([v[l].std(axis=(0, 1)) for l in range(n)]) for k, v in x.items()},
               "cov": {(a, b): numpy.stack([((x[a][l] - x[a][l].mean(axis=(0, 1))) * (x[b][l] - x[b][l].mean(axis=(0, 1)))).mean(axis=(0, 1))
                                            for l in range(n)]) for a, b in pairs}}
    return res


def case(shape, dtype, seed=0, n_fields=5):
    """``n_fields`` fields of NAMES of another size and spread each, another draw per LES"""
    rng = numpy.random.default_rng(1000 * seed + 17 * n_fields + int(numpy.prod(shape)) % 97)
    fields = {}
    for f in range(n_fields):
        base, spread = (5.0, 290.0, 0.3, 9e-3, -2.0, 1e-4, 40.0, -300.0)[f], (1.0, 0.5, 0.4, 4e-4, 1.5, 1e-4, 7.0, 20.0)[f]
        fields[NAMES[f]] = (base + spread * rng.standard_normal(shape)).astype(dtype)
    return fields


PAIRS3 = (("A", "B"), ("C", "E"), ("D", "C"))                         # with face "C": one pair without it, one with it on each side


def same_results(what, got, want):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for kind in want:
        assert set(got[kind]) == set(want[kind]), (what, kind)
        for key in want[kind]:
            assert_bits("%s %s %s" % (what, kind, key), got[kind][key], want[kind][key])


def pick(res, kinds, pairs):
    """the part of a result of les_moments that a launch with these kinds and pairs returns"""
    out = {k: dict(res[k]) for k in kinds}
    if pairs:
        out["cov"] = {tuple(p): res["cov"][tuple(p)] for p in pairs}
    return out


# -- device plumbing ---------------------------------------------------------------------------------------------------------
_same, _sync = Poisoned.read_only, qlr._sync


class Run:
    """one launch through ``eng.les_moments`` with every array inside a poisoned buffer; ``check`` compares every output with
    the oracle bit for bit, the fields with what was uploaded, and looks at the bytes around every array.  ``leads``: name ->
    elements of NaN in front of that field; ``pad``: elements between the rows of every output"""

    def __init__(self, eng, fields, pairs=(), face=None, kinds=KINDS, leads=None, pad=0):
        self.eng, self.fields, self.pairs, self.face, self.kinds, self.pad = eng, fields, [tuple(p) for p in pairs], face, tuple(kinds), pad
        self.bufs, self.dev, self.out = {}, {}, {}
        for k, a in fields.items():
            lead = (leads or {}).get(k, 0)
            t, b = slab_edges.with_tail(eng, a, float("nan"), lead=lead)
            self.bufs[("field", k)] = (t, b, lead, float("nan"))
            self.dev[k] = t
        first = next(iter(fields.values()))
        n, ktot = first.shape[0], first.shape[-1]
        for kind, key in [(kind, k) for kind in self.kinds for k in fields] + [("cov", p) for p in self.pairs]:
            t, b = slab_edges.with_tail(eng, numpy.full((n, ktot + pad), POISON, dtype=first.dtype), POISON)
            self.bufs[(kind, key)] = (t, b, 0, POISON)
            self.out.setdefault(kind, {})[key] = t[:, :ktot]
        self.got = eng.les_moments(self.dev, self.pairs, mean="mean" in self.kinds, var="var" in self.kinds, std="std" in self.kinds,
                                   face=face, out=self.out)
        _sync(eng)

    def host(self):
        return {kind: {key: t.cpu().numpy() for key, t in d.items()} for kind, d in self.out.items()}

    def check(self, what=""):
        full = les_moments(self.fields, self.pairs, self.face)
        want = pick(full, self.kinds, self.pairs)
        assert set(self.got) == set(want), (what, sorted(self.got))
        for kind, d in self.got.items():
            for key, t in d.items():
                assert t.data_ptr() == self.out[kind][key].data_ptr(), (what, kind, key, "not written into out")
        same_results(what, self.host(), want)
        ktot = next(iter(self.fields.values())).shape[-1]
        for (kind, key), (t, b, lead, poison) in self.bufs.items():
            if kind == "field":
                assert _same(t, self.fields[key]), (what, key, "read only")
            around = torch.cat([b[:lead], b[lead + t.numel():]])
            assert bool((torch.isnan(around) if poison != poison else around == poison).all()), (what, kind, key, "written around the array")
            if kind != "field" and t.shape[1] > ktot:
                assert bool((t[:, ktot:] == poison).all()), (what, kind, key, "written between the rows")
        return full


FIELD_SLOTS = ("fields", "mean", "var", "std")


def raw_launch(eng, fields, pairs=(), face=-1, kinds=KINDS, extents=None, alias=None, null=()):
    """spc_les_moments_* itself: (rc, host outputs {(member, index): array}).  ``extents``: overrides of the scalar members;
    ``alias``: ((member, index), (member, index)) pairs, the first pointer replaced by the second; ``null``: (member, index)
    pointers set to NULL.  The fields are compared with what was uploaded."""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    names = list(fields)
    first = fields[names[0]]
    n, itot, jtot, ktot = first.shape
    a = _abi.LesMomentsArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.n_pairs, a.face_field, a.pitch_out = n, itot, jtot, ktot, len(names), len(pairs), face, ktot
    t = {}
    for f, k in enumerate(names):
        t[("fields", f)] = dev(fields[k])
        for kind in kinds:
            t[(kind, f)] = dev(numpy.full((n, ktot), POISON, dtype=first.dtype))
    for q, (pa, pb) in enumerate(pairs):
        a.pair_a[q], a.pair_b[q] = pa, pb
        t[("cov", q)] = dev(numpy.full((n, ktot), POISON, dtype=first.dtype))
    for (member, i), v in t.items():
        getattr(a, member)[i] = v.data_ptr()
    for (member, i), src in (alias or ()):
        getattr(a, member)[i] = t[src].data_ptr()
    for key, val in (extents or {}).items():
        if isinstance(val, dict):
            for i, v in val.items():
                getattr(a, key)[i] = v
        else:
            setattr(a, key, val)
    for member, i in null:
        getattr(a, member)[i] = None
    rc = abi_call(eng, "spc_les_moments", a)
    for f, k in enumerate(names):
        assert _same(t[("fields", f)], fields[k])
    return rc, {key: v.cpu().numpy() for key, v in t.items() if key[0] != "fields"}


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """five fields, three pairs, the face field in two of them, all four kinds; a plane of one row has no variance at all"""
    fields = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    res = Run(eng, fields, PAIRS3, "C").check("n %d plane %s ktot %d" % (n, plane, ktot))
    if tuple(plane) == (1, 1):
        for kind in ("var", "std", "cov"):
            for key, v in res[kind].items():
                assert not v.any() and not numpy.signbit(v).any(), (kind, key)
    else:
        assert all((v > 0).all() for v in res["var"].values()) and all(v.any() for v in res["cov"].values())


def check_counts(eng):
    """one field and eight, no pair and eight, a field in four pairs, (a, b) and (b, a), each kind alone, only the covariances"""
    dtype = np_of(eng)
    for ktot in (7, 64):
        shape = (2, 2, 3, ktot)
        Run(eng, case(shape, dtype, 1, 1)).check("one field ktot %d" % ktot)
        eight = case(shape, dtype, 2, 8)
        Run(eng, eight).check("eight fields, no pair ktot %d" % ktot)
        pairs = [("A", "B"), ("A", "C"), ("D", "A"), ("A", "H"), ("B", "A"), ("G", "F"), ("F", "G"), ("H", "E")]
        run = Run(eng, eight, pairs, "A")
        run.check("eight fields, eight pairs ktot %d" % ktot)
        got = run.host()["cov"]
        assert_bits("(a, b) and (b, a)", got[("A", "B")], got[("B", "A")])
        assert_bits("(a, b) and (b, a)", got[("G", "F")], got[("F", "G")])
        five = case(shape, dtype, 3)
        for kind in KINDS:
            Run(eng, five, (), "B", kinds=(kind,)).check("%s alone ktot %d" % (kind, ktot))
        Run(eng, five, PAIRS3, "C", kinds=()).check("only cov ktot %d" % ktot)
        Run(eng, five, PAIRS3[:1], None, kinds=("std",)).check("std and one pair ktot %d" % ktot)


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 2 x 3 with other data per LES, so a wrong l shows; with and without a pitch on the outputs; at ktot 7 and
    8 all LES of a launch share one wave"""
    for n in NS:
        for pad in (0, 3, 4):
            fields = case((n, 2, 3, ktot), np_of(eng), seed=4 + n, n_fields=3)
            if n > 1:
                assert not numpy.array_equal(fields["A"][0], fields["A"][1])
            Run(eng, fields, (("A", "C"),), "C", pad=pad).check("rows n %d ktot %d pad %d" % (n, ktot, pad))


def check_face(eng):
    """the face field first, last and in the middle of the list; k = 0 and the seams between the vectors; NaN directly in front
    of every field's first element (x[-1] is never read); without ``face`` the bits are others"""
    dtype = np_of(eng)
    on_grid = 16 // numpy.dtype(dtype).itemsize
    for ktot in (2, 3, 8, 65):
        fields = case((2, 2, 3, ktot), dtype, seed=ktot, n_fields=3)
        plain = les_moments(fields, (("A", "C"),), None)
        for face in ("A", "B", "C"):
            for lead in (on_grid, 1):
                leads = {k: lead for k in fields}
                res = Run(eng, fields, (("A", "C"), ("C", "B")), face, leads=leads).check("face %s ktot %d lead %d" % (face, ktot, lead))
                assert not numpy.array_equal(res["mean"][face], plain["mean"][face]) and not numpy.array_equal(res["var"][face], plain["var"][face])
                others = [k for k in fields if k != face]
                assert all(numpy.array_equal(res["var"][k], plain["var"][k]) for k in others)
                assert_bits("level 0 of a face field is half its first face", res["mean"][face][:, 0],
                            les_moments({face: dtype(0.5) * fields[face]})["mean"][face][:, 0])


def special_cases(dtype, ktot=9):
    """name -> (fields, pairs, face): a NaN cell in a centre field and one in the face field, an infinity, planes of -0.0, a
    constant plane, and large values with small deviations (1e5 with some 1e-3: an fma or a one-pass formula shows; the
    draw has a spread of 4e-3 because float32 has a grid of 2^-7 = 7.8e-3 there: a spread of 1e-3 would round every cell to 1e5)"""
    shape = (2, 4, 5, ktot)
    base = case(shape, dtype, seed=9, n_fields=3)
    cases = {"clean": (base, (("A", "C"), ("B", "A")), "C")}
    nan = {k: v.copy() for k, v in base.items()}
    nan["A"][1, 2, 3, 4] = numpy.nan
    nan["C"][0, 1, 1, 6] = numpy.nan
    cases["nan"] = (nan, (("A", "C"), ("B", "A")), "C")
    inf = {k: v.copy() for k, v in base.items()}
    inf["B"][1, 0, 0, 2] = numpy.inf
    inf["A"][0, 3, 4, 7] = -numpy.inf
    cases["inf"] = (inf, (("A", "C"), ("B", "A")), "C")
    zero = {k: v.copy() for k, v in base.items()}
    zero["A"][0, :, :, 3] = -0.0
    zero["C"][:, :, :, :2] = -0.0
    zero["B"][1, :, :, 5] = 287.25
    cases["zeros"] = (zero, (("A", "C"), ("B", "A")), "C")
    rng = numpy.random.default_rng(3)
    big = {"A": (1e5 + 4e-3 * rng.standard_normal(shape)).astype(dtype), "B": (-3e4 + 1e-2 * rng.standard_normal(shape)).astype(dtype)}
    cases["big"] = (big, (("A", "B"),), None)
    return cases


def check_special(eng):
    dtype = np_of(eng)
    cases = special_cases(dtype)
    res = {name: Run(eng, *c).check("special " + name) for name, c in cases.items()}
    clean, nan, inf, zero = res["clean"], res["nan"], res["inf"], res["zeros"]
    # a NaN cell: that level of that LES (a face field: the level above too) NaN in everything its field touches, all else equal
    hit = {"A": numpy.zeros(clean["mean"]["A"].shape, dtype=bool), "B": None, "C": None}
    hit["A"][1, 4] = True
    hit["C"] = numpy.zeros_like(hit["A"])
    hit["C"][0, 6:8] = True
    hit["B"] = numpy.zeros_like(hit["A"])
    touched = {("A", "C"): hit["A"] | hit["C"], ("B", "A"): hit["A"]}
    for kind in KINDS + ("cov",):
        for key, v in nan[kind].items():
            where = touched[key] if kind == "cov" else hit[key]
            assert numpy.isnan(v[where]).all() and where.sum() == numpy.isnan(v).sum(), (kind, key)
            assert_bits("beside the NaN %s %s" % (kind, key), v[~where], clean[kind][key][~where])
    # an infinity: the mean is infinite, the deviations are NaN
    assert inf["mean"]["B"][1, 2] == numpy.inf and inf["mean"]["A"][0, 7] == -numpy.inf
    assert numpy.isnan(inf["var"]["B"][1, 2]) and numpy.isnan(inf["std"]["A"][0, 7]) and numpy.isnan(inf["cov"][("B", "A")][1, 2])
    assert numpy.isnan(inf["var"]["B"]).sum() == 1
    # planes of -0.0 have the mean +0.0 (the face average of two -0.0 levels: +0.0 + -0.0), no variance; a constant plane none
    for key, l, k in (("A", 0, 3), ("C", 0, 0), ("C", 1, 1)):
        for kind in KINDS:
            v = zero[kind][key][l, k]
            assert v == 0 and not numpy.signbit(v), (kind, key, l, k)
    assert zero["mean"]["B"][1, 5] == dtype(287.25) and zero["var"]["B"][1, 5] == 0 and zero["cov"][("B", "A")][1, 5] == 0
    # 1e5 +- some 1e-3: in float32 the deviations are one or two ulp of the values; the two-pass rule still sees them
    big = res["big"]
    assert (big["var"]["A"] > 0).all() and (big["var"]["A"] < 1e-3).all()


def check_alignment(eng, ktot, pad=0, plane=(17, 5)):
    """views one, two and three elements off the 16-byte grid, every field differently (single elements whatever ktot), and
    all on it with a pitch that is off it"""
    fields = case((2,) + plane + (ktot,), np_of(eng), seed=ktot + pad)
    for leads in ({"A": 1, "B": 2, "C": 0, "D": 3, "E": 1}, {"A": 0, "B": 0, "C": 1, "D": 0, "E": 0}, {}):
        Run(eng, fields, PAIRS3, "C", leads=leads, pad=pad).check("leads %s ktot %d pad %d" % (leads, ktot, pad))


def check_refusals(eng):
    """n = 0 is a no-op; ktot == 1 is unsupported; N > 2^24, a pitch below ktot, a NULL field, no output, a bad pair, a bad
    face_field and an output that is a field or another output are refused by the library; the engine refuses the same and bad
    shapes; no refused call writes"""
    dtype = np_of(eng)
    fields = case((2, 2, 3, 8), dtype, seed=6, n_fields=3)
    pairs = ((0, 2), (1, 0))
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    t = {k: dev(v) for k, v in fields.items()}
    got = eng.les_moments({k: v[:0] for k, v in t.items()}, (("A", "B"),), std=True, face="B")
    assert sorted(got) == ["cov", "mean", "std", "var"] and all(tuple(v.shape) == (0, 8) for d in got.values() for v in d.values())

    def untouched(out):
        assert all((v == dtype(POISON)).all() for v in out.values())
    rc, out = raw_launch(eng, fields, pairs, 1, extents=dict(n_les=0))
    assert rc == 0
    untouched(out)
    rc, out = raw_launch(eng, fields, pairs, 1, extents=dict(n_les=0), null=[("fields", f) for f in range(3)] + [("cov", 0), ("cov", 1)], kinds=())
    assert rc == 0
    rc, out = raw_launch(eng, fields, pairs, 1)
    assert rc == 0 and not any((v == dtype(POISON)).any() for v in out.values())
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    bad = [(dict(extents=dict(ktot=1, pitch_out=1)), U, b"ktot == 1"),
           (dict(extents=dict(itot=4097, jtot=4097)), E, b"2^24"),
           (dict(extents=dict(pitch_out=7)), E, b"pitch_out"),
           (dict(null=[("fields", 1)]), E, b"required pointer fields"),
           (dict(kinds=(), null=[("cov", 0), ("cov", 1)]), E, b"no output"),
           (dict(extents=dict(pair_a={0: 3})), E, b"pair 0"), (dict(extents=dict(pair_b={1: -1})), E, b"pair 1"),
           (dict(extents=dict(pair_b={0: 0})), E, b"pair 0"),
           (dict(extents=dict(face_field=3)), E, b"face_field"), (dict(extents=dict(face_field=-2)), E, b"face_field"),
           (dict(extents=dict(n_fields=0)), E, b"field count"), (dict(extents=dict(n_fields=9)), E, b"field count"),
           (dict(extents=dict(n_pairs=9)), E, b"pair count"), (dict(extents=dict(n_pairs=-1)), E, b"pair count"),
           (dict(alias=[(("mean", 0), ("fields", 2))]), E, b"same array"), (dict(alias=[(("cov", 1), ("fields", 0))]), E, b"same array"),
           (dict(alias=[(("var", 1), ("std", 1))]), E, b"same array"), (dict(alias=[(("cov", 0), ("mean", 2))]), E, b"same array"),
           (dict(extents=dict(ktot=0)), E, b">= 1"), (dict(extents=dict(n_les=-1)), E, b"n_les")]
    for kw, code, text in bad:
        rc, out = raw_launch(eng, fields, pairs, 1, **kw)
        assert rc == code and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        untouched(out)
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    out8 = lambda: torch.full((2, 8), POISON, dtype=eng.dtype, device=eng.device)         # noqa: E731
    one_level = {k: v[..., :1].contiguous() for k, v in t.items()}
    nine = {NAMES[0] + str(i): t["A"] for i in range(9)}
    for call in (lambda: eng.les_moments({}),
                 lambda: eng.les_moments(nine),
                 lambda: eng.les_moments(t, [("A", "B")] * 2),
                 lambda: eng.les_moments(t, [("A", "A")]),
                 lambda: eng.les_moments(t, [("A", "Z")]),
                 lambda: eng.les_moments(t, [("A", "B"), ("B", "A"), ("A", "C"), ("C", "A"), ("B", "C"), ("C", "B")] + [("A", "B")] * 3),
                 lambda: eng.les_moments(t, face="Z"),
                 lambda: eng.les_moments(t, mean=False, var=False),
                 lambda: eng.les_moments({"A": t["A"], "B": t["B"][:1]}),
                 lambda: eng.les_moments({"A": t["A"][..., ::2]}),
                 lambda: eng.les_moments({"A": t["A"].to(other)}),
                 lambda: eng.les_moments({"A": t["A"].cpu()}),
                 lambda: eng.les_moments({"A": t["A"]}, out={"mean": {"A": out8()[:, :7]}}),
                 lambda: eng.les_moments({"A": t["A"]}, out={"mean": {"A": out8().to(other)}}),
                 lambda: eng.les_moments({"A": t["A"], "B": t["B"]}, var=False, out={"mean": {"A": out8(), "B": torch.full((2, 12), POISON, dtype=eng.dtype, device=eng.device)[:, :8]}})):
        try:
            call()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    for call in (lambda: eng.les_moments(one_level),):
        try:
            call()
        except RuntimeError as e:                                # (the library's own refusal, as les_advance's)
            assert "ktot == 1" in str(e)
        else:
            raise AssertionError("a field of one level was not refused")
    _sync(eng)
    for k in fields:
        assert_bits("refused: " + k, t[k].cpu().numpy(), fields[k])


def check_same_as_k10_k6(eng):
    """``mean`` is K10's slab mean of the same fields; ``std`` of a QT field K6 has nudged is K6's own qt_std"""
    from tests.test_vnudge import make_les_fields
    dtype = np_of(eng)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    for ktot in (7, 64):
        fields = case((3, 8, 8, ktot), dtype, seed=ktot)
        t = {k: dev(v) for k, v in fields.items()}
        got, means = eng.les_moments(t, var=False), eng.slab_means(t)
        _sync(eng)
        for k in fields:
            assert_bits("mean of %s is K10's" % k, got["mean"][k].cpu().numpy(), means[k].cpu().numpy())
    n, itot, jtot, ktot = 3, 8, 8, 40
    fs = [make_les_fields(itot, jtot, ktot, seed=20 + i) for i in range(n)]
    stack = lambda k: dev(numpy.stack([f[k] for f in fs]).astype(dtype))                       # noqa: E731
    rng = numpy.random.default_rng(2)
    R = rng.normal(size=(n, itot, jtot))
    R -= R.sum(axis=(1, 2), keepdims=True) / (itot * jtot)
    qt = stack("qt")
    before = qt.clone()
    res = eng.variability_nudge(qt, stack("qsat"), dev(R), stack("ql_av"), stack("qt_av"), stack("ql_ref"))
    got = eng.les_moments({"QT": qt}, mean=False, var=False, std=True)
    _sync(eng)
    assert not torch.equal(before, qt)
    assert_bits("std of the nudged QT is K6's qt_std", got["std"]["QT"].cpu().numpy(), res["qt_std"].cpu().numpy())


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    fields = case((n, 2, 3, 40), np_of(one), seed=n, n_fields=3)
    pairs = (("A", "C"), ("C", "B"))
    want = pick(les_moments(fields, pairs, "C"), KINDS, pairs)
    for tag, eng, up in on_both(one, multi, n):
        t = {k: up(v) for k, v in fields.items()}
        got = eng.les_moments(t, pairs, std=True, face="C")
        multi.synchronize()
        same_results(tag, {kind: {key: host_of(v) for key, v in d.items()} for kind, d in got.items()}, want)
        for k in fields:
            assert qlr._same_host(host_of(t[k]), fields[k])
    return blocks_of(t["A"], multi, n)


def check_large_plane(eng):
    """ONE LES of 64 x 64 x 2 (4 096 rows: whole rounds of the long-plane launch) and of 33 x 31 x 5 (1 023 rows: the ragged
    tail of the load-ahead loop)"""
    for shape in ((1, 64, 64, 2), (1, 33, 31, 5)):
        fields = case(shape, np_of(eng), seed=shape[1], n_fields=2)
        Run(eng, fields, (("B", "A"),), "A").check("large plane %s" % (shape,))


def check_chain(eng):
    """the cases of the lane's walk (les_harness.chain_cases) for the 8 rows in flight of the 16-byte form and, at ktot 7 and with
    every field off the 16-byte grid, for the 32 of the other (nij = 1 ... 17 and 31 ... 33, 63 ... 65); a pair walks with half
    of either, the face field is in the pair and a field job of its own"""
    dtype = np_of(eng)
    long = (31, 32, 33, 63, 64, 65)
    for shape, lead in list(chain_cases(8, dtype)) + [c for c in chain_cases(32, dtype, long) if c[0][-1] == 7 or c[1]]:
        fields = case(shape, dtype, seed=9, n_fields=3)
        Run(eng, fields, (("A", "C"),), "C", leads={k: lead for k in fields}).check("chain %s lead %d" % (shape, lead))


BODIES = ("parity", "counts", "rows", "face", "special", "alignment", "refusals", "same_as_k10_k6", "large_plane", "chain")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (2, 7, 64, 65)]),
            ("counts", lambda: check_counts(eng)),
            ("rows", lambda: [check_rows(eng, k) for k in (7, 8)]),
            ("face", lambda: check_face(eng)),
            ("special", lambda: check_special(eng)),
            ("alignment", lambda: [check_alignment(eng, *a) for a in ((65, 0), (64, 0), (160, 1))]),
            ("refusals", lambda: check_refusals(eng)),
            ("same_as_k10_k6", lambda: check_same_as_k10_k6(eng)),
            ("large_plane", lambda: check_large_plane(eng)),
            ("chain", lambda: check_chain(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_moments (CPU suite) ------------------------------------------------------------------------
class MomentsOracleEngine(qlr.QtLocalOracleEngine):
    """tests/les_qt_local_ref.QtLocalOracleEngine with ``les_moments`` by the NumPy oracle above: the results written into the
    caller's tensors or new ones, as the HIP engine does"""

    def les_moments(self, fields, pairs=(), mean=True, var=True, std=False, face=None, out=None, **kw):
        pairs = [tuple(p) for p in pairs]
        kinds = [k for k, on in (("mean", mean), ("var", var), ("std", std)) if on]
        if not fields or (not kinds and not pairs) or any(a == b or a not in fields or b not in fields for a, b in pairs) or \
                (face is not None and face not in fields):
            raise ValueError("les_moments: bad fields, pairs, face or no output")
        if next(iter(fields.values())).shape[-1] == 1:
            raise RuntimeError("les_moments: ktot == 1")
        want = pick(les_moments({k: v.numpy() for k, v in fields.items()}, pairs, face), kinds, pairs)
        res = {}
        for kind, d in want.items():
            for key, v in d.items():
                t = (out or {}).get(kind, {}).get(key)
                if t is None:
                    t = torch.from_numpy(numpy.ascontiguousarray(v))
                else:
                    t.copy_(torch.from_numpy(v))
                res.setdefault(kind, {})[key] = t
        return res


# -- the host twin of models.DeviceLESEnsemble.get_statistics ----------------------------------------------------------------------
def twin_statistics(ens, w=None, names=None, pairs=None):
    """what ``get_statistics`` of an ensemble returns, from host copies of its fields by the oracle above: the fields of
    statistics.FIELDS it holds (``ens`` may be a host twin or the device ensemble itself), ``w`` the vertical wind at the upper
    faces or None, the pairs of statistics.PAIRS whose fields are present, TKE where U and V are"""
    names = list(st.FIELDS if names is None else names)
    f = ens.fields3d
    if getattr(ens, "thermo", False) or getattr(ens, "THERMO", False) or "QL" in f or ("QT" in f and "Qsat" in f):
        ens.get_fields_batched("QL")
    have = {}
    for k in st.FIELDS:
        if k == st.FACE:
            if w is not None:
                have[k] = numpy.asarray(w)
        elif k in f:
            have[k] = numpy.asarray(host_of(ens.get_fields_batched(k)))
    pairs = [tuple(p) for p in (st.PAIRS if pairs is None else pairs) if p[0] in have and p[1] in have]
    keep = [k for k in names if k in have]
    need = {k: have[k] for k in st.FIELDS if k in keep or any(k in p for p in pairs)}
    res = les_moments(need, pairs, st.FACE if st.FACE in need else None)
    out = {kind: {k: numpy.asarray(res[kind][k], dtype=numpy.float64) for k in keep} for kind in KINDS}
    out["cov"] = {p: numpy.asarray(res["cov"][p], dtype=numpy.float64) for p in pairs}
    if "U" in keep and "V" in keep:
        out["TKE"] = st.tke(out["var"])
    return out


def flat(stats):
    """a result of get_statistics as one dict of arrays (a record of a log)"""
    rec = {}
    for kind, d in stats.items():
        if kind == "TKE":
            rec["TKE"] = numpy.array(d)
        else:
            rec.update({"%s %s" % (kind, "-".join(key) if isinstance(key, tuple) else key): numpy.array(v) for key, v in d.items()})
    return rec


VARIANTS = qlr.VARIANTS


def ensemble_run(engine, n, calls=None, **kw):
    """a device ensemble as tests/les_qt_local_ref.ensemble_run makes it (``kw``: its modes), three steps and one constantT nudge
    before the last: after each of them the statistics are read twice, through the batched getter and through two rows, and
    compared with the twin's on host copies of the ensemble's own fields (every other test of the ensemble holds those equal
    to the host twins' bit for bit; W is the device's own: the twins' differs in its last bits).  ``calls``: the list a counting
    wrapper of ``les_moments`` appends to; ONE launch per engine that holds rows per change of the fields, none for a second
    read.  Returns the records."""
    log = []

    def launches():
        return None if calls is None else len(calls)

    def record(ens):
        before = launches()
        w = ens.get_vertical_wind_batched()
        dev = ens.get_statistics_batched()
        host = ens.get_statistics()
        mid = launches()
        again = ens.get_statistics()
        ens.get_statistics_batched(("U", "QT"), (("THL", "QT"),))
        want = twin_statistics(ens, None if w is None else host_of(w))
        rec, ref = flat(host), flat(want)
        assert set(rec) == set(ref) and "TKE" in rec and "var QL" in rec and ("cov W-THL" in rec) == (w is not None), sorted(rec)
        for k in ref:
            assert_bits("statistics %s" % k, rec[k], ref[k])
            assert rec[k].dtype == numpy.float64 and rec[k].shape == (ens.n, ens.nL)
        assert_bits("batched getter", host_of(dev["var"]["QT"]).astype(numpy.float64), host["var"]["QT"])
        for k, v in flat(again).items():
            assert_bits("second read %s" % k, v, rec[k])
        for i in sorted({0, ens.n - 1}):
            for k, v in flat(ens[i].get_statistics()).items():
                assert_bits("row %d %s" % (i, k), v, rec[k][i])
        if calls is not None:
            rows = [int(p.shape[0]) for p in getattr(ens.fields3d["QT"], "parts", [ens.fields3d["QT"]])]
            assert mid - before == sum(1 for r in rows if r > 0) and launches() == mid, (before, mid, launches(), rows)
        log.append(rec)
        return rec

    # qlr.ensemble_run owns the sequence; the statistics are read behind every step and behind the nudge it makes
    inner, nudge = models.DeviceLESEnsemble.evolve_model_batched, spcpl.variability_nudge_ensemble
    seen = []

    def step(self, t):
        if not seen:
            record(self)                                              # the attached fields, before the first step
            seen.append(self)
        inner(self, t)
        record(self)

    def nudged(ens, *a, **k):
        res = nudge(ens, *a, **k)
        record(ens)
        return res
    models.DeviceLESEnsemble.evolve_model_batched, spcpl.variability_nudge_ensemble = step, nudged
    try:
        ens, _ = qlr.ensemble_run(engine, n, True, kind=kw.pop("kind", None), **kw)
    finally:
        models.DeviceLESEnsemble.evolve_model_batched, spcpl.variability_nudge_ensemble = inner, nudge
    assert len(log) == 5
    return ens, log
