"""K7 (the standalone exner / interp / searchsorted / integral / interp_c / interp_rho / rms operators of spc_sputils.hpp) where a
workgroup owns a SLAB of several rows: the bodies of tests/test_sputils_slabs_gpu.py (each takes an engine: tools/mutation_control.py
--sputils hands them the engines of its mutant libraries) and, on the oracle-backed engine below, of tests/test_sputils_slabs_cpu.py.

su_rows (spc_sputils_host.hpp) caps the slab height at n_rows / (4 x compute units): on a whole card every launch of fewer than
2 048 rows runs one row per workgroup, and SuWalk's carry, the row index r > 0, the per-row LDS offsets and the partial last slab
are never exercised.  The bodies count ONE compute unit for their launches (SPC_CUS, read at every launch: counted_cus), so that
40 rows get the slabs that 10 000 get on the card, and every launch asks spc_sputils_describe_launch for the height it got and
asserts on it: no body passes at one row per workgroup.  Every result is compared bit for bit (gpu_util.assert_bits; array_equal
for the indices) with NumPy / the oracle's restatement of splib/sputils.py for float64 and tests/f32_ref.py for float32; every
device array is the leading part of a poisoned buffer (tests/les_harness.Poisoned), looked at after the launch."""
import collections
import contextlib
import warnings

import numpy
import torch

from oracle import spcpl_oracle as orc
from sp_coupler_amd import _abi
from tests import f32_ref
from tests.fake_engine import OracleEngine
from tests.gpu_util import assert_bits
from tests.les_harness import DTYPES, NP, Poisoned, counted_cus, np_of, run_bodies  # noqa: F401  (DTYPES, NP: for the tests)

Desc = collections.namedtuple("Desc", "name rb grid lds cus")
ES = {torch.float64: 8, torch.float32: 4}
NAN = float("nan")
IPOISON = -7                                  # of the int64 indices
CAP, CAP_C = 16 * 1024, 32 * 1024             # su_rows' LDS budgets: interp and searchsorted; interp_c
TARGET = 1100                                 # outputs per workgroup su_rows aims at
#: the instantiation names of every launch the bodies checked, per element size (check_coverage)
LAUNCHED = {8: set(), 4: set()}


def parse(text):
    name, rest = text.split(" ", 1)
    kv = dict(item.split("=") for item in rest.split())
    return Desc(name, int(kv["rb"]), int(kv["grid"]), int(kv["lds"]), int(kv["cus"]))


def _lib(eng):
    return getattr(eng, "lib", None) or _abi.load_library()


def su_pad(n):
    """entries of the NaN-padded LDS row of a table of n entries (spc_device.hpp: 2 p2 + 2, p2 the power-of-two floor of n)"""
    return 2 * (1 << (max(int(n), 1).bit_length() - 1)) + 2


# -- what a launch is described as ---------------------------------------------------------------------------------------------
def _pitch(a, pad):
    return 0 if a.ndim == 1 else a.shape[1] + pad


def describe_interp(eng, n, n_x, n_xp, px, pxp, pfp, po):
    a = _abi.InterpArgs(n, n_x, n_xp, px, pxp, pfp, po, 1, 1, 1, 1)           # dummy non-null pointers: never dereferenced
    return parse(_abi.sputils_describe_launch(_lib(eng), _abi.SPC_SU_INTERP, ES[eng.dtype], a))


def describe_searchsorted(eng, n, n_a, n_v, pa, pv, po):
    a = _abi.SearchsortedArgs(n, n_a, n_v, pa, pv, po, 1, 1, 1, 0, 0)
    return parse(_abi.sputils_describe_launch(_lib(eng), _abi.SPC_SU_SEARCHSORTED, ES[eng.dtype], a))


MODES = {"interp_c": 0, "interp_rho": 1, "integral": 2}


def describe_interp_c(eng, n, nG, nL, pZ, pz, pq, po, mode, weighted):
    a = _abi.InterpCArgs(n, nG, nL, pZ, pz, pq, po, 1, 1, 1, 1 if weighted else None, 1, MODES[mode], 0)
    return parse(_abi.sputils_describe_launch(_lib(eng), _abi.SPC_SU_INTERP_C, ES[eng.dtype], a))


def describe_op(eng, name, n, n_out, n_tab, shared_t):
    """the description of the operator ``name`` of OPS on contiguous rows: n_tab entries of xp / a, or cells of zh"""
    if name == "interp":
        return describe_interp(eng, n, n_out, n_tab, n_out, 0 if shared_t else n_tab, n_tab, n_out)
    if name.startswith("searchsorted"):
        return describe_searchsorted(eng, n, n_tab, n_out, 0 if shared_t else n_tab, n_out, n_out)
    mode = {"interp_c": "interp_c", "interp_rho": "interp_rho"}.get(name, "integral")
    return describe_interp_c(eng, n, n_out, n_tab + 1, n_out + 1, 0 if shared_t else n_tab + 1, n_tab, n_out, mode, name in ("interp_c", "integral_weighted"))


def describe_rms(eng, n_rows, n, pitch):
    return parse(_abi.sputils_describe_launch(_lib(eng), _abi.SPC_SU_RMS, ES[eng.dtype], None, n_rows, n, pitch))


# -- the oracles, row by row -----------------------------------------------------------------------------------------------------
def _row(a, r):
    return a[r] if a.ndim == 2 else a


def want_interp(x, xp, fp):
    n = fp.shape[0]
    one = numpy.interp if fp.dtype == numpy.float64 else f32_ref.interp
    with numpy.errstate(all="ignore"):
        return numpy.stack([one(_row(x, r), _row(xp, r), fp[r]) for r in range(n)]).astype(fp.dtype)


def want_searchsorted(a, v, side):
    n = max(t.shape[0] for t in (a, v) if t.ndim == 2)
    return numpy.stack([numpy.searchsorted(_row(a, r), _row(v, r), side=side) for r in range(n)]).astype(numpy.int64)


def want_interp_c(Zh, zh, q, rho, mode):
    """splib/sputils.py:173-197 per row; a None of integral() is NaN (what Q[i] = None stores), also behind interp_rho's division"""
    f64 = Zh.dtype == numpy.float64
    integral = orc.integral if f64 else f32_ref.integral
    out = numpy.zeros((Zh.shape[0], Zh.shape[1] - 1), dtype=Zh.dtype)
    with numpy.errstate(all="ignore"):
        for r in range(Zh.shape[0]):
            Z, z, w = Zh[r], _row(zh, r), (None if rho is None or mode == "interp_rho" else rho[r])
            for k in range(len(Z) - 1):
                if mode == "integral" or Z[k] < z[-1]:
                    v = integral(Z[k + 1], Z[k], z, q[r], w)
                    v = numpy.nan if v is None else v
                    out[r, k] = v / (Z[k] - Z[k + 1]) if mode == "interp_rho" else v
    return out


def want_rms(a):
    one = orc.rms if a.dtype == numpy.float64 else f32_ref.rms
    with numpy.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # (the mean of an empty row)
        return numpy.array([one(numpy.ascontiguousarray(row)) for row in a], dtype=a.dtype)


# -- one checked launch per call -------------------------------------------------------------------------------------------------
def _put(P, tag, a, pad):
    return P.put(tag, a, NAN) if a.ndim == 1 else P.rows(tag, a, NAN, pad=pad)


def _host(t):
    return t.cpu().numpy()


def _note(eng, d, min_rb):
    assert d.rb >= min_rb, ("slab height", d, min_rb)
    LAUNCHED[ES[eng.dtype]].add(d.name)
    return d


def run_interp(eng, x, xp, fp, pads=(0, 0, 0, 0), what="interp", min_rb=2):
    """eng.interp on poisoned, pitched device copies (pads: of x, xp, fp, out) against the oracle; returns its description"""
    n, n_xp = fp.shape
    n_x = x.shape[-1]
    assert (numpy.diff(xp, axis=-1) >= 0).all(), "the case's own table is not sorted"
    d = describe_interp(eng, n, n_x, n_xp, _pitch(x, pads[0]), _pitch(xp, pads[1]), n_xp + pads[2], n_x + pads[3])
    P = Poisoned(eng)
    xd, xpd, fpd = _put(P, "x", x, pads[0]), _put(P, "xp", xp, pads[1]), _put(P, "fp", fp, pads[2])
    out = P.rows("out", numpy.full((n, n_x), NAN, dtype=fp.dtype), NAN, pad=pads[3])
    eng.interp(xd, xpd, fpd, out=out)
    assert_bits("%s %s" % (what, (d,)), _host(out), want_interp(x, xp, fp))
    out.fill_(NAN)
    P.check_around(what)
    return _note(eng, d, min_rb)


def run_searchsorted(eng, a, v, side, pads=(0, 0, 0), what="searchsorted", min_rb=2):
    n = max(t.shape[0] for t in (a, v) if t.ndim == 2)
    n_a, n_v = a.shape[-1], v.shape[-1]
    assert (numpy.diff(a, axis=-1) >= 0).all(), "the case's own table is not sorted"
    d = describe_searchsorted(eng, n, n_a, n_v, _pitch(a, pads[0]), _pitch(v, pads[1]), n_v + pads[2])
    P = Poisoned(eng)
    ad, vd = _put(P, "a", a, pads[0]), _put(P, "v", v, pads[1])
    out = P.rows("out", numpy.full((n, n_v), IPOISON, dtype=numpy.int64), IPOISON, pad=pads[2])
    eng.searchsorted(ad, vd, side=side, out=out)
    got, want = _host(out), want_searchsorted(a, v, side)
    assert got.dtype == numpy.int64 and numpy.array_equal(got, want), (what, side, d, int((got != want).sum()))
    out.fill_(IPOISON)
    P.check_around(what)
    return _note(eng, d, min_rb)


def run_interp_c(eng, Zh, zh, q, rho, mode, pads=(0, 0, 0, 0), what="interp_c", min_rb=2):
    """eng.interp_c in ``mode``; pads: of Zh, zh, q and rho (one pitch), out"""
    n, nG = Zh.shape[0], Zh.shape[1] - 1
    nL = zh.shape[-1]
    weighted = rho is not None and mode != "interp_rho"
    d = describe_interp_c(eng, n, nG, nL, nG + 1 + pads[0], _pitch(zh, pads[1]), q.shape[1] + pads[2], nG + pads[3], mode, weighted)
    P = Poisoned(eng)
    Zd, zd, qd = _put(P, "Zh", Zh, pads[0]), _put(P, "zh", zh, pads[1]), _put(P, "q", q, pads[2])
    rd = _put(P, "rho", rho, pads[2]) if weighted else None
    out = P.rows("out", numpy.full((n, nG), NAN, dtype=Zh.dtype), NAN, pad=pads[3])
    eng.interp_c(Zd, zd, qd, rd, mode=mode, out=out)
    assert_bits("%s %s %s" % (what, mode, (d,)), _host(out), want_interp_c(Zh, zh, q, rho, mode))
    out.fill_(NAN)
    P.check_around(what)
    return _note(eng, d, min_rb)


#: the operators of the bodies: name -> launch(eng, rng, n, n_out, n_tab, **kw) of random rows; n_tab: the table (xp, a; the fine
#: grid's cells for the integrals), n_out: queries, keys or coarse layers
def _table(rng, dt, n, n_tab, shared=False):
    t = numpy.sort(rng.uniform(0, 1e4, size=(n, n_tab)), axis=1).astype(dt)
    return t[0].copy() if shared else t


def _queries(rng, dt, n, n_out, shared=False):
    x = rng.uniform(-300, 1.03e4, size=(n, n_out)).astype(dt)
    return x[0].copy() if shared else x


def op_interp(eng, rng, n, n_out, n_tab, shared_x=False, shared_t=False, pads=(0, 0, 0, 0), what="interp", min_rb=2):
    dt = np_of(eng)
    xp, fp, x = _table(rng, dt, n, n_tab, shared_t), rng.normal(size=(n, n_tab)).astype(dt), _queries(rng, dt, n, n_out, shared_x)
    if n_tab > 2:
        (x if x.ndim == 1 else x[:, 0])[...] = xp[n_tab // 2] if shared_t else (xp[0, n_tab // 2] if shared_x else xp[:, n_tab // 2])
    return run_interp(eng, x, xp, fp, pads, what, min_rb)


def op_searchsorted(side):
    def op(eng, rng, n, n_out, n_tab, shared_x=False, shared_t=False, pads=(0, 0, 0, 0), what="searchsorted", min_rb=2):
        dt = np_of(eng)
        a, v = _table(rng, dt, n, n_tab, shared_t), _queries(rng, dt, n, n_out, shared_x and not shared_t)
        if n_tab > 2:
            (v if v.ndim == 1 else v[:, 0])[...] = a[n_tab // 2] if shared_t else (a[0, n_tab // 2] if v.ndim == 1 else a[:, n_tab // 2])
        return run_searchsorted(eng, a, v, side, (pads[1], pads[0], pads[3]), "%s %s" % (what, side), min_rb)
    return op


def coarse_case(rng, dt, n, nG, nc, shared=False):
    """(Zh, zh, q, rho): a fine grid of nc cells per row (or one for all), coarse bounds descending from above its top (layers
    above the top stay zero) down to its first point exactly"""
    zh = numpy.cumsum(rng.uniform(0.5, 30, size=(n, nc + 1)), axis=1)
    za = zh[0] if shared else zh
    top = (za[-1] if shared else za[:, -1:]) * rng.uniform(0.7, 1.4, size=(n, 1))
    bot = za[0] if shared else za[:, :1]
    Zh = numpy.sort(rng.uniform(0, 1, size=(n, nG + 1)), axis=1)[:, ::-1] * (top - bot) + bot
    Zh = numpy.ascontiguousarray(Zh).astype(dt)
    za = za.astype(dt)
    Zh[:, -1] = za[0] if shared else za[:, 0]
    return Zh, za, rng.normal(size=(n, nc)).astype(dt), rng.uniform(0.4, 1.3, size=(n, nc)).astype(dt)


def op_coarse(mode, weighted):
    def op(eng, rng, n, n_out, n_tab, shared_x=False, shared_t=False, pads=(0, 0, 0, 0), what="interp_c", min_rb=2):
        Zh, zh, q, rho = coarse_case(rng, np_of(eng), n, n_out, max(n_tab, 1), shared_t)
        if mode == "interp_rho":
            q = rho
        return run_interp_c(eng, Zh, zh, q, rho if weighted else None, mode, pads, what, min_rb)
    return op


OPS = collections.OrderedDict([
    ("interp", op_interp), ("searchsorted_left", op_searchsorted("left")), ("searchsorted_right", op_searchsorted("right")),
    ("interp_c", op_coarse("interp_c", True)), ("interp_rho", op_coarse("interp_rho", False)),
    ("integral_weighted", op_coarse("integral", True)), ("integral", op_coarse("integral", False))])
COARSE = ("interp_c", "interp_rho", "integral_weighted", "integral")


def lds_elems(name, n_out, n_tab, shared_t):
    """(per row, fixed) LDS elements of the operator's slab, as its launcher counts them (n_tab: entries of xp / a, cells of zh)"""
    if name == "interp":
        return n_tab + (0 if shared_t else su_pad(n_tab)), su_pad(n_tab) if shared_t else 0
    if name.startswith("searchsorted"):
        return (0 if shared_t else su_pad(n_tab)), su_pad(n_tab) if shared_t else 0
    terms = 2 if name in ("interp_c", "integral_weighted") else 1
    return n_tab * terms + 2 * n_out + 1 + (0 if shared_t else su_pad(n_tab)), su_pad(n_tab) if shared_t else 0


# -- bodies ----------------------------------------------------------------------------------------------------------------------
#: per element size: the slab heights check_heights must see, per operator (worked out from su_rows' rule: see the body)
HEIGHTS = {
    8: {"interp": {1, 2, 3, 8, 9, 21, 64}, "searchsorted_left": {1, 2, 3, 8, 15, 64}, "searchsorted_right": {1, 2, 3, 8, 15, 64},
        "interp_c": {1, 2, 3, 12}, "interp_rho": {1, 2, 3, 17}, "integral_weighted": {1, 2, 3, 12}, "integral": {1, 2, 3, 17}},
    4: {"interp": {1, 2, 3, 8, 18, 43, 64}, "searchsorted_left": {1, 2, 3, 8, 31, 64}, "searchsorted_right": {1, 2, 3, 8, 31, 64},
        "interp_c": {1, 2, 3, 25}, "interp_rho": {1, 2, 3, 35}, "integral_weighted": {1, 2, 3, 25}, "integral": {1, 2, 3, 35}},
}


def check_heights(eng):
    """per operator: one row per workgroup (the control: 3 rows), slabs of 2 and 3 rows (8 and 13 rows with one compute unit), the
    height fit_rounds moves to from its first choice (91 sample points, 160 queries: 8 rows = exactly 5 rounds of 256 outputs,
    not the 7 of ceil(1100 / 160)), the largest height the LDS budget allows for a table of 91 entries (the next one does not
    fit: asserted from the description's own lds), and 64 (searchsorted with a shared a, interp with a table of 4 entries)"""
    es, rng = ES[eng.dtype], numpy.random.default_rng(31)
    with counted_cus(1):
        for name, op in OPS.items():
            coarse = name in COARSE
            seen = set()
            seen.add(op(eng, rng, 3, 160, 91, what="heights control", min_rb=1).rb)
            assert seen == {1}
            seen.add(op(eng, rng, 8, 160, 91, what="heights 2").rb)
            seen.add(op(eng, rng, 13, 160, 91, what="heights 3").rb)
            if not coarse:
                d = op(eng, rng, 265, 160, 91, what="heights fit_rounds")
                assert d.rb == 8 and -(-TARGET // 160) == 7, d
                seen.add(d.rb)
            for shared_t in ((False, True) if name == "interp" else (False,)):
                n_out = 4 if coarse else 7                      # few outputs per row: the first choice is 64, the LDS decides
                d = op(eng, rng, 265, n_out, 91, shared_t=shared_t, what="heights LDS")
                per_row, fixed = lds_elems(name, n_out, 91, shared_t)
                cap = CAP_C if coarse else CAP
                assert d.lds == (per_row * d.rb + fixed) * es <= cap < (per_row * (d.rb + 1) + fixed) * es and d.rb < 64, (name, d)
                seen.add(d.rb)
            if name == "interp":
                seen.add(op(eng, rng, 265, 5, 4, what="heights 64").rb)
            elif not coarse:
                seen.add(op(eng, rng, 265, 7, 91, shared_t=True, what="heights 64").rb)
            assert seen == HEIGHTS[es][name], (name, sorted(seen))


def check_last_slab(eng):
    """row counts that leave a last slab of one row, of rb - 1 rows and none partial, contiguous and pitched outputs: poison
    around every array and between the rows of the pitched ones (the run_* look)"""
    rng = numpy.random.default_rng(32)
    with counted_cus(1):
        for name, op in OPS.items():
            n_out, n_tab = (23, 40) if name in COARSE else (150, 91)
            R = op(eng, rng, 400, n_out, n_tab, what="last_slab height").rb
            assert 4 <= R <= 64, (name, R)
            for rows, left in ((4 * R + 1, 1), (5 * R - 1, R - 1), (5 * R, 0)):
                for pads in ((0, 0, 0, 0), (1, 2, 3, 5)):
                    d = op(eng, rng, rows, n_out, n_tab, pads=pads, what="last_slab %d rows" % rows)
                    assert d.rb == R and rows % R == left and d.grid == -(-rows // R), (name, d, rows)


#: where SuWalk changes behaviour: the reciprocal for n < 256 (exact only because 255 n < 2^16), n >= 256, dr of 0 and 1, di == 0
WALK = tuple(range(1, 41)) + (127, 128, 129, 254, 255, 256, 257, 300, 511, 512, 513)
#: both sides of each power of two from 2 to 1 024: the rows of su_stage_rows are su_pad(p2) entries long
TABLES = tuple(sorted({max(1, p + s) for p in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024) for s in (-1, 0, 1)}))
#: (operator, table) pairs of check_walk that the LDS budget of today leaves at one row per workgroup whatever the sharing (the
#: description says so; check_walk asks it): launched by tests/test_sputils_gpu.py's search-depth tests only.  Per element size.
ONE_ROW_TABLES = {
    8: {("interp", 512), ("interp", 513), ("interp", 1023), ("interp", 1024), ("interp", 1025), ("searchsorted_left", 1024),
        ("searchsorted_left", 1025), ("interp_c", 1023), ("interp_c", 1024), ("interp_c", 1025), ("integral", 1024), ("integral", 1025)},
    4: {("interp", 1024), ("interp", 1025)},
}


def check_walk(eng):
    """SuWalk at every count of outputs per row where it changes behaviour (n_x, n_v; nG for the layer-major walk, the staging
    of Zh and the row-major store of interp_c) and, for the staging walks over the padded rows, every table length on both
    sides of each power of two from 2 to 1 024 (n_xp, n_a, nL - 1) -- each at a slab height of at least 2"""
    es, rng = ES[eng.dtype], numpy.random.default_rng(33)
    with counted_cus(1):
        for n in WALK:
            for name in ("interp", "searchsorted_right", "interp_c", "integral"):
                rows = 13 if n > 4 else 41                       # (3 rows of a few outputs do not fill one round: 10 rows)
                OPS[name](eng, rng, rows, n, 37 if name in COARSE else 91, shared_x=n % 3 == 0, pads=(0, 0, 0, n % 2), what="walk n_out=%d" % n)
        one_row = set()
        for n_tab in TABLES:
            for name in ("interp", "searchsorted_left", "interp_c", "integral"):
                # per-row tables where two rows fit the operator's LDS budget, else one shared table, else nothing: asked of the
                # description, so a budget that grows launches the lengths it newly allows
                fits = [describe_op(eng, name, 9, 9, n_tab, shared).rb >= 2 for shared in (False, True)]
                if not any(fits):
                    one_row.add((name, n_tab))
                    continue
                OPS[name](eng, rng, 9, 9, n_tab, shared_t=not fits[0], what="walk n_tab=%d" % n_tab)
        assert one_row <= ONE_ROW_TABLES[es], sorted(one_row - ONE_ROW_TABLES[es])     # (no length lost to a budget that shrank)


def check_rows_differ(eng):
    """every row of a slab has its own table, values and queries (random rows: a wrong r shows): shared x, shared xp / a / zh,
    both shared, every array on a padded pitch, a different pad per array; interp_c with q and rho on one pitch and Zh and out on
    others"""
    rng = numpy.random.default_rng(34)
    with counted_cus(1):
        for name, op in OPS.items():
            for n_out, n_tab, some in ((160, 91, slice(None)), (19, 160, slice(1, None, 2))):
                for shared_x, shared_t, pads in ((True, False, (0, 0, 0, 0)), (False, True, (0, 0, 0, 0)), (True, True, (0, 0, 0, 0)),
                                                 (False, False, (2, 2, 2, 2)), (False, False, (1, 4, 2, 7)), (False, True, (5, 0, 1, 3)))[some]:
                    d = op(eng, rng, 29, n_out, n_tab, shared_x=shared_x, shared_t=shared_t, pads=pads, what="rows_differ")
                    assert d.rb >= 4, (name, d)


def _special_rows(R, rows):
    """the first, a middle and the last row of slab 1, and the rows of the partial last slab"""
    assert rows % R not in (0,) and rows >= 3 * R
    return [R, R + R // 2, 2 * R - 1] + list(range(rows - rows % R, rows))


def check_specials_in_the_slab(eng):
    """numpy.interp's and integral()'s special cases in the first, a middle and the last row of a slab and in the partial last
    slab (the integrals' six kinds of row: kind k in those rows of slab k, and all six in the partial last slab): NaN and +-inf x, exact hits on the table's first, last and a middle entry, x below and above it, a repeated sample
    point (zero dx: numpy's fallbacks), NaN and inf in fp, tables of 1 and 2 entries; for the integrals a coarse bound below the
    grid (None -> NaN), a layer that ends exactly on the grid's first and last point, a == b, a > b, layers wholly above the
    grid's top (whole waves that skip the integral) and a row whose fine grid is shallower than every coarse layer"""
    dt, rng = np_of(eng), numpy.random.default_rng(35)
    with counted_cus(1):
        for n_xp, n_x in ((91, 160), (2, 40), (1, 40), (5, 300)):
            for shared_t in (False, True):
                rows = 31
                xp, fp, x = _table(rng, dt, rows, n_xp), rng.normal(size=(rows, n_xp)).astype(dt), _queries(rng, dt, rows, n_x)
                R = describe_interp(eng, rows, n_x, n_xp, n_x, 0 if shared_t else n_xp, n_xp, n_x).rb
                assert 2 <= R and 3 * R <= rows and rows % R, (R, n_xp, n_x)
                m = max(1, 40 % n_xp)                                          # the repeated sample point: entries m - 1 and m
                for r in _special_rows(R, rows):
                    t = xp[0] if shared_t else xp[r]
                    x[r, :9] = [numpy.nan, numpy.inf, -numpy.inf, t[0], t[-1], t[n_xp // 2], t[0] - 1, t[-1] + 1, numpy.nextafter(t[-1], dt(0))]
                    if n_xp > 4:
                        if not shared_t:
                            xp[r, m] = xp[r, m - 1]                            # zero dx
                        x[r, 9:12] = [t[m - 1], (t[2] + t[3]) / 2, (t[n_xp - 2] + t[n_xp - 1]) / 2]
                        fp[r, 2], fp[r, n_xp - 2] = numpy.nan, numpy.inf
                        fp[r, m - 1] = fp[r, m]
                if shared_t and n_xp > 4:
                    xp[0, m] = xp[0, m - 1]
                t = xp[0].copy() if shared_t else xp
                d = run_interp(eng, x, t, fp, what="specials interp n_xp=%d" % n_xp)
                assert d.rb == R
                for side in ("left", "right"):
                    assert run_searchsorted(eng, t, x, side, what="specials searchsorted n_a=%d" % n_xp).rb >= 2
        for shared, mode, w in [(sh, m, w) for sh in (False, True) for m, w in (('interp_c', True), ('interp_rho', False), ('integral', True), ('integral', False))]:
            nG, nc = 23, 40
            # the height of THIS mode's slabs places the rows.  Six kinds of special row, each in the first, a middle and the last row of a full slab (kind k: slab k) and in the
            # partial last slab (its six rows): 6 R + 6 rows
            R = describe_interp_c(eng, 400, nG, nc + 1, nG + 1, 0 if shared else nc + 1, nc, nG, mode, w).rb
            rows = 6 * R + 6
            assert R >= 7 and describe_interp_c(eng, rows, nG, nc + 1, nG + 1, 0 if shared else nc + 1, nc, nG, mode, w).rb == R, R
            Zh, zh, q, rho = coarse_case(rng, dt, rows, nG, nc, shared)
            placed = set()
            for kind in range(6):
                for pos, r in (("first", kind * R), ("middle", kind * R + R // 2), ("last", kind * R + R - 1), ("partial", 6 * R + kind)):
                    z = zh if shared else zh[r]
                    low = numpy.sort(rng.uniform(z[0], z[-1], nG).astype(dt))[::-1]    # bounds inside the grid, descending
                    if kind == 0:
                        Zh[r, nG // 2] = z[0] - dt(3)                  # a bound below the grid: the two layers that touch it are None
                    elif kind == 1:
                        Zh[r, 0], Zh[r, 1:] = z[-1], low               # layers that end exactly on the grid's last and first point
                        Zh[r, -1] = z[0]
                    elif kind == 2:
                        Zh[r, 1:] = low
                        Zh[r, nG - 5] = Zh[r, nG - 6]                  # a == b, inside the grid
                        Zh[r, -1] = z[0]
                    elif kind == 3:
                        Zh[r, 1:] = low
                        Zh[r, nG - 8], Zh[r, nG - 7] = Zh[r, nG - 7], Zh[r, nG - 8]      # a > b in two layers, a < b between, inside the grid
                        Zh[r, -1] = z[0]
                    elif kind == 4:
                        Zh[r, :nG - 2] = z[-1] + numpy.arange(nG - 2, 0, -1).astype(dt)  # all but two layers wholly above the top
                        Zh[r, nG - 2], Zh[r, nG - 1] = (z[0] + z[-1]) / 2, z[0] + (z[-1] - z[0]) / 4
                    else:                                              # a fine grid shallower than every coarse layer
                        Zh[r] = z[0] + (z[-1] - z[0]) * (dt(1.5) * numpy.arange(nG, -1, -1).astype(dt))
                    assert r // R == (kind if pos != "partial" else 6) and r % R == {"first": 0, "middle": R // 2, "last": R - 1, "partial": kind}[pos]
                    placed.add((kind, pos))
            assert len(placed) == 24 and 0 < R // 2 < R - 1 and rows % R == 6
            with numpy.errstate(all="ignore"):
                c = want_interp_c(Zh, zh, q, rho, "interp_c")
                g = want_interp_c(Zh, zh, q, None, "integral")
            for kind, what in ((0, numpy.isnan(c)), (4, c == 0), (5, c == 0)):         # the cases are what they are meant to be
                for r in (kind * R, kind * R + R // 2, kind * R + R - 1, 6 * R + kind):
                    assert what[r].any() and (kind != 5 or what[r].all()), (kind, r)
            for r in (2 * R, 2 * R + R // 2, 3 * R - 1, 6 * R + 2):
                assert Zh[r, nG - 5] == Zh[r, nG - 6] and numpy.isfinite(g[r, 1:]).all(), r
            for r in (3 * R, 3 * R + R // 2, 4 * R - 1, 6 * R + 3):
                assert Zh[r, nG - 7] > Zh[r, nG - 8] and numpy.isfinite(g[r, 1:]).all(), r
            d = run_interp_c(eng, Zh, zh, rho if mode == "interp_rho" else q, rho if w else None, mode, what="specials %s" % mode)
            assert d.rb == R


RMS_ROWS = (1, 31, 32, 33, 65)
RMS_N = (0, 1, 7, 8, 9, 39, 40, 41, 128, 129, 248, 249, 488, 489, 968, 969, 1024, 1025, 8192, 8193, 20011)


def check_rms_groups(eng):
    """k_rms gives 8 lanes to a row and 32 rows to a workgroup: row counts around one and two workgroups (the dead groups walk row
    0), row lengths on both sides of numpy's leaf (8, 128) and of every depth of its pairwise recursion (248, 488, 968, 1 024),
    one chunk and more (8 192), a padded pitch; n == 0 is served (numpy's mean of nothing: NaN)"""
    dt, rng = np_of(eng), numpy.random.default_rng(36)
    names = set()
    for n in RMS_N:
        for n_rows in (RMS_ROWS if n <= 1025 else (33,)):
            for pad in ((0, 3) if n in (0, 41, 129, 1025) or n_rows == 33 else (0,)):
                a = (rng.normal(size=(n_rows, n)) * rng.uniform(1e-3, 1e3, size=(n_rows, 1))).astype(dt)
                d = describe_rms(eng, n_rows, n, n + pad)
                assert d.rb == 32 and d.grid == -(-n_rows // 32), d
                P = Poisoned(eng, tail_elems=64)
                ad = P.rows("a", a, NAN, pad=pad) if n else torch.empty((n_rows, 0), dtype=eng.dtype, device=eng.device)
                out = P.put("out", numpy.full(n_rows, 7.0, dtype=dt), 7.0)
                if pad and n:
                    assert ad.stride(0) == n + pad
                eng.rms(ad, out=out)
                assert_bits("rms %d x %d pad %d" % (n_rows, n, pad), _host(out), want_rms(a))
                out.fill_(7.0)
                P.check_around("rms")
                names.add(d.name)
    LAUNCHED[ES[eng.dtype]].update(names)
    assert len(names) == 5, sorted(names)                            # pd 0, 1, 2, 3 and the explicit stack


PLAIN_BYTES = 64 * 1024 * 1024


def check_plain_stores(eng):
    """one launch per operator that writes more than 64 MiB, i.e. with plain stores (wt=0 in its description): bit for bit the
    same rows launched in four parts (write-through stores, wt=1), and the oracle on the first and last 200 rows.  The only
    large case: about 70 MB per array, made and compared on the device.  (An engine on the host computes the ends only.)"""
    es, dt = ES[eng.dtype], np_of(eng)
    on_host = eng.device.type == "cpu"
    gen = torch.Generator(device=eng.device).manual_seed(37)
    rand = lambda *s: torch.rand(*s, generator=gen, device=eng.device, dtype=eng.dtype)      # noqa: E731
    ends = lambda t: numpy.concatenate([_host(t[:200]), _host(t[-200:])])                    # noqa: E731
    cut = lambda t, i, k: t if t.dim() == 1 else t[i:i + k]                                  # noqa: E731

    def both(what, fn, describe, n, oracle, *arrs):
        if on_host:
            full = torch.cat([fn(*[cut(a, 0, 200) for a in arrs]), fn(*[cut(a, n - 200, 200) for a in arrs])])
            got_ends = _host(full)
        else:
            full = fn(*arrs)
            k = -(-n // 4)
            parts = torch.cat([fn(*[cut(a, i, k) for a in arrs]) for i in range(0, n, k)])
            assert torch.equal(full.view(torch.int64 if es == 8 else torch.int32) if full.is_floating_point() else full,
                               parts.view(torch.int64 if es == 8 else torch.int32) if parts.is_floating_point() else parts), what
            got_ends = ends(full)
            del parts
        d, dk = describe(n), describe(-(-n // 4))
        assert d.name.endswith("wt=0>") and dk.name.endswith("wt=1>") and d.name[:-3] == dk.name[:-3] and d.rb >= 2 and dk.rb >= 2, (d, dk)
        want = oracle(*[(ends(a) if a.dim() == 2 else _host(a)) for a in arrs])
        if want.dtype == numpy.int64:
            assert numpy.array_equal(got_ends, want), what
        else:
            assert_bits(what, got_ends, want)
        LAUNCHED[es].update((d.name, dk.name))

    n_xp, n_x = 91, 160
    n = PLAIN_BYTES // (n_x * es) + 600
    xp = torch.sort(rand(n, n_xp) * 1e4, dim=1).values
    fp, x = rand(n, n_xp) - 0.5, rand(n, n_x) * 1.06e4 - 300
    both("plain interp", eng.interp, lambda k: describe_interp(eng, k, n_x, n_xp, n_x, n_xp, n_xp, n_x), n, want_interp, x, xp, fp)
    del fp
    m = PLAIN_BYTES // (n_x * 8) + 600
    for side in ("left", "right"):
        both("plain searchsorted " + side, lambda a, v: eng.searchsorted(a, v, side=side),
             lambda k: describe_searchsorted(eng, k, n_xp, n_x, n_xp, n_x, n_x), m, lambda a, v: want_searchsorted(a, v, side), xp[:m], x[:m])
    del xp, x
    nG, nc = 160, 91
    zh = torch.cumsum(rand(nc + 1) * 30 + 0.5, dim=0)
    frac = torch.sort(rand(n, nG + 1), dim=1, descending=True).values
    Zh = (frac * (zh[-1] * 1.2 - zh[0]) + zh[0]).contiguous()
    Zh[:, -1] = zh[0]
    q, rho = rand(n, nc) - 0.5, rand(n, nc) + 0.4
    del frac
    for mode, w in (("interp_c", True), ("integral", False)):
        both("plain " + mode, lambda Z, z, qq, rr: eng.interp_c(Z, z, qq, rr if w else None, mode=mode),
             lambda k: describe_interp_c(eng, k, nG, nc + 1, nG + 1, 0, nc, nG, mode, w), n,
             lambda Z, z, qq, rr: want_interp_c(Z, z, qq, rr if w else None, mode), Zh, zh, q, rho)
    assert describe_interp(eng, n, n_x, n_xp, n_x, n_xp, n_xp, n_x).cus == describe_rms(eng, 1, 1, 1).cus      # the card's own count


BODIES = ("heights", "last_slab", "walk", "rows_differ", "specials_in_the_slab", "rms_groups", "plain_stores")


def jobs(eng):
    return [("heights", lambda: check_heights(eng)), ("last_slab", lambda: check_last_slab(eng)), ("walk", lambda: check_walk(eng)),
            ("rows_differ", lambda: check_rows_differ(eng)), ("specials_in_the_slab", lambda: check_specials_in_the_slab(eng)),
            ("rms_groups", lambda: check_rms_groups(eng)), ("plain_stores", lambda: check_plain_stores(eng))]


def check_everything(eng):
    """every body above on one engine: what tools/mutation_control.py --sputils runs on a mutant library.  Returns the names of the
    bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


def reachable(es):
    """the instantiation names the shapes of the bodies reach, per element size.  The unrolled search depths (sl 7 ... 10) and sum
    depths (pd 1 ... 3) exist for double; the float twins run the run-time descent (sl 0) and the explicit stack (pd -1).  Plain
    stores (wt=0) are launched at one shape per operator.  Not here: sl=-1, tables beyond the LDS -- one row per workgroup
    whatever the launch (tests/test_sputils_gpu.py) -- and k_interp<f64,sl=10>, whose 16 KiB hold one row of 512 entries."""
    ty = "f64" if es == 8 else "f32"
    names = {"k_rms<%s,pd=%d,wt=1>" % (ty, pd) for pd in (0, 1, 2, 3, -1)}
    if es == 4:
        names |= {"k_%s<f32,sl=0,wt=%d>" % (k, wt) for k in ("interp", "searchsorted") for wt in (0, 1)}
        return names | {"k_interp_c<f32,pd=-1,sl=0,w=%d,wt=%d>" % (w, wt) for w in (0, 1) for wt in (0, 1)}
    names |= {"k_interp<f64,sl=%d,wt=1>" % sl for sl in (0, 7, 8, 9)} | {"k_searchsorted<f64,sl=%d,wt=1>" % sl for sl in (0, 7, 8, 9, 10)}
    names |= {"k_interp<f64,sl=7,wt=0>", "k_searchsorted<f64,sl=7,wt=0>"}
    for w in (0, 1):
        names |= {"k_interp_c<f64,pd=%d,sl=%d,w=%d,wt=1>" % (pd, sl, w) for pd, sl in ((1, 0), (1, 8), (2, 8), (2, 9), (3, 9), (3, 0))}
        names.add("k_interp_c<f64,pd=1,sl=0,w=%d,wt=0>" % w)
    return names | {"k_interp_c<f64,pd=-1,sl=0,w=0,wt=1>"}            # (integral without weights on 1 024 cells and more)


def check_coverage(eng):
    """behind check_everything: the names the bodies launched on engines of this element size are the reachable ones, so that a
    new SL, PD or WT instantiation cannot ship without a slab launch of it"""
    es = ES[eng.dtype]
    assert LAUNCHED[es] == reachable(es), (sorted(LAUNCHED[es] - reachable(es)), sorted(reachable(es) - LAUNCHED[es]))


# -- an oracle-backed engine with the K7 operators and out= (CPU suite) --------------------------------------------------------------
class SlabOracleEngine(OracleEngine):
    """tests/fake_engine.OracleEngine with ``out=`` on the K7 operators and, for float32, tests/f32_ref.py as the oracle: the
    bodies above run on it without a GPU -- which tests their own expectations (heights, cases, poison), not a kernel"""

    def __init__(self, dtype=torch.float64):
        self.dtype = dtype

    @staticmethod
    def _into(res, out):
        if out is None:
            return res
        out.copy_(res.reshape(out.shape))
        return out

    def interp(self, x, xp, fp, stream=None, out=None):
        return self._into(torch.from_numpy(want_interp(x.numpy(), xp.numpy(), fp.numpy())), out)

    def searchsorted(self, a, v, side="left", stream=None, out=None):
        return self._into(torch.from_numpy(want_searchsorted(a.numpy(), v.numpy(), side)), out)

    def interp_c(self, Zh, zh, q, rho=None, mode="interp_c", stream=None, out=None):
        return self._into(torch.from_numpy(want_interp_c(Zh.numpy(), zh.numpy(), q.numpy(), None if rho is None else rho.numpy(), mode)), out)

    def rms(self, a, stream=None, out=None):
        return self._into(torch.from_numpy(want_rms(a.numpy())), out)


@contextlib.contextmanager
def fresh_coverage():
    """LAUNCHED emptied for the duration (a test that asserts the coverage of ITS run)"""
    saved = {k: set(v) for k, v in LAUNCHED.items()}
    for v in LAUNCHED.values():
        v.clear()
    try:
        yield
    finally:
        for k, v in saved.items():
            LAUNCHED[k] |= v
