"""NumPy oracle of K21 (include/spc.h: spc_les_buoyancy_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_buoyancy_gpu.py (each takes an engine: tools/mutation_control.py --buoyancy hands them the engines of its mutant
libraries), the host twins of models.DeviceLESEnsemble's buoyancy mode and an oracle-backed engine with ``les_buoyancy`` for the
CPU suite.

The oracle spells the rule out one operation per NumPy call in the element type with dtype-typed scalars, vectorised over the
columns, a Python loop over k with two ``numpy.subtract`` per level for the chain, so nothing fuses.  Every device array of the
bodies is the LEADING part of a poisoned buffer (tests/les_harness.Poisoned); the bytes behind it (and in front of a view off
the 16-byte grid) are checked after the launch."""

import numpy
import torch

from sp_coupler_amd import _abi, models
from sp_coupler_amd import advection as adv
from sp_coupler_amd import buoyancy as buo
from tests import les_advect_ref as lar
from tests import les_micro_ref as lmr
from tests import les_radiate_ref as lrr
from tests import les_vadvect_ref as lvr
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, cols_table, ensemble_case, fill_args, host_of, np_of, on_both, run_bodies)

#: no neighbour at all, planes of two along one axis and along both (gx or gy +0), an odd plane, the flagship's, and one wider
#: than a wave along j
PLANES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (8, 8), (5, 33)]
#: no chain (1), one step (2), around one wave and eight chunks of the chain (63, 64, 65), the flagship's 160
KTOTS = [1, 2, 63, 64, 65, 160]
NS = [1, 2, 5]
ROWS = [1, 2, 3, 8, 9, 33]                                         # itot of the strip seams
OUT_FILL = -7.0
DT = 6.0


# -- the rule --------------------------------------------------------------------------------------------------------------
def hydrostatic(thl, qt, ql, t0, lex, s):
    """(phi [n x itot x jtot x ktot], psfc [n x itot x jtot]) of fields of dtype T (``ql`` may be None) and profiles [n x ktot]"""
    T = thl.dtype.type
    assert all(a.dtype == thl.dtype for a in (qt, t0, lex, s)) and (ql is None or ql.dtype == thl.dtype)
    c1, c2, one = T(buo.C1), T(buo.C2), T(1)
    P = lambda a: a[:, None, None, :]                                                       # noqa: E731
    ktot = thl.shape[3]
    with numpy.errstate(all="ignore"):
        if ql is None:
            e = numpy.zeros_like(thl)
        else:
            e = P(lex) * ql
        tl = thl + e
        a = c1 * qt
        m = one + a
        if ql is not None:
            w = c2 * ql
            m = m - w
        tv = tl * m
        d = tv - P(t0)
        b = d * P(s)
        assert b.dtype == thl.dtype
        phi = numpy.empty_like(thl)
        q = numpy.zeros(thl.shape[:3], dtype=thl.dtype)
        for k in range(ktot - 1, -1, -1):                          # sequential from the lid
            f = numpy.subtract(q, b[..., k])
            q = numpy.subtract(f, b[..., k])
            phi[..., k] = f
    return phi, q


def pressure_gradient(phi, u, v, hx, hy):
    """(the new u, the new v, amax [n]) of phi, u, v [n x itot x jtot x ktot] of dtype T and hx, hy [n]"""
    assert all(a.dtype == phi.dtype for a in (u, v, hx, hy))
    n = u.shape[0]
    with numpy.errstate(all="ignore"):
        gx = numpy.roll(phi, -1, axis=1) - numpy.roll(phi, 1, axis=1)
        gy = numpy.roll(phi, -1, axis=2) - numpy.roll(phi, 1, axis=2)
        du = hx[:, None, None, None] * gx
        dv = hy[:, None, None, None] * gy
        un = u - du
        vn = v - dv
        a = numpy.abs(du) + numpy.abs(dv)
        amax = a.reshape(n, -1).max(axis=1) if n else numpy.zeros(0, dtype=u.dtype)
    assert un.dtype == vn.dtype == amax.dtype == u.dtype
    return un, vn, amax


def les_buoyancy(thl, qt, ql, u, v, hx, hy, t0, lex, s):
    """(phi, psfc, the new u, the new v, amax), new arrays"""
    phi, psfc = hydrostatic(thl, qt, ql, t0, lex, s)
    un, vn, amax = pressure_gradient(phi, u, v, hx, hy)
    return phi, psfc, un, vn, amax


# -- inputs ------------------------------------------------------------------------------------------------------------------
def case(shape, dtype, seed=0, dt=DT):
    """dict of the arguments in ``dtype``: thl, qt, ql, u, v, hx, hy, t0, lex, s; another grid, pressure, mean state, hx and hy
    per LES; some cells hold liquid water and some hold none"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(9000 + seed + 7 * ktot + itot * jtot + 31 * n)
    rhobf, zh, zf, presf, _ = lrr.grid(n, ktot, rng)
    k = numpy.arange(ktot)
    thm = 290.0 + 10.0 * k / 160.0 + 0.5 * numpy.arange(n)[:, None]
    qtm = 8e-3 * numpy.exp(-k / 160.0) * (1.0 + 0.05 * numpy.arange(n))[:, None]
    qlm = numpy.where((k >= ktot // 3) & (k < ktot // 3 + max(1, ktot // 4)), 2e-4, 0.0) * numpy.ones((n, 1))
    t0, lex, s = buo.profiles(thm, qtm, qlm, presf, zh, zf=zf)
    thl = thm[:, None, None, :] + 0.5 * rng.standard_normal(shape)
    qt = qtm[:, None, None, :] * (1.0 + 0.05 * rng.standard_normal(shape))
    ql = numpy.maximum(qlm[:, None, None, :] + 2e-4 * rng.standard_normal(shape), 0.0)
    ql.flat[0], ql.flat[-1] = 0.0, 2e-4                            # (whatever the shape: a dry cell and a wet one)
    u = 5.0 + rng.standard_normal(shape)
    v = -2.0 + rng.standard_normal(shape)
    hx, hy = adv.coefficients(dt, 200.0 * (1.0 + 0.1 * numpy.arange(n)), 300.0 * (1.0 + 0.05 * numpy.arange(n)), n=n)
    c = dict(thl=thl, qt=qt, ql=ql, u=u, v=v, hx=hx, hy=hy, t0=t0, lex=lex, s=s)
    return {key: numpy.ascontiguousarray(a.astype(dtype)) for key, a in c.items()}


def oracle(c, ql=True):
    return les_buoyancy(c["thl"], c["qt"], c["ql"] if ql else None, c["u"], c["v"], c["hx"], c["hy"], c["t0"], c["lex"], c["s"])


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one call of ``eng.les_buoyancy`` with every array inside a poisoned buffer; ``check`` compares phi, psfc, u, v and amax
    with the oracle bit for bit (amax: a NaN where the oracle's is one), the read-only inputs with what was uploaded, and looks
    at the bytes around every array.  ``leads``: elements in front of (thl, qt, ql, phi; u and v take the first);
    ``pad``: elements between the rows of t0, lex and s (pitched profiles)"""

    def __init__(self, eng, c, leads=(0, 0, 0, 0), pad=0, ql=True, psfc=True, amax=True):
        self.eng, self.c, self.ql = eng, c, ql
        self.mem = Poisoned(eng)
        put, prof = self.mem.put, lambda tag, a: self.mem.rows(tag, a, 1e30, pad=pad)          # noqa: E731
        nan = float("nan")
        self.dthl, self.dqt = put("thl", c["thl"], nan, leads[0]), put("qt", c["qt"], nan, leads[1])
        self.dql = put("ql", c["ql"], nan, leads[2]) if ql else None
        self.du, self.dv = put("u", c["u"], nan, leads[0]), put("v", c["v"], nan, leads[0])
        self.dhx, self.dhy = put("hx", c["hx"], 1e30), put("hy", c["hy"], 1e30)
        self.dt0, self.dlex, self.ds = prof("t0", c["t0"]), prof("lex", c["lex"]), prof("s", c["s"])
        self.dphi = put("phi", numpy.full_like(c["thl"], OUT_FILL), 1e30, leads[3])
        self.dpsfc = put("psfc", numpy.full(c["thl"].shape[:3], OUT_FILL, dtype=c["thl"].dtype), 1e30) if psfc else None
        self.damax = put("amax", numpy.full_like(c["hx"], -5.0), 1e30) if amax else None
        self.got = eng.les_buoyancy(self.dthl, self.dqt, self.dql, self.du, self.dv, self.dhx, self.dhy, self.dt0, self.dlex, self.ds,
                                    self.dphi, psfc=self.dpsfc, amax=self.damax if amax else False)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        c = self.c
        phi, psfc, un, vn, amax = want = oracle(c, self.ql)
        assert_bits("%s phi" % what, self.dphi.cpu().numpy(), phi)
        assert_bits("%s u" % what, self.du.cpu().numpy(), un)
        assert_bits("%s v" % what, self.dv.cpu().numpy(), vn)
        if self.dpsfc is not None:
            assert_bits("%s psfc" % what, self.dpsfc.cpu().numpy(), psfc)
        if self.damax is None:
            assert self.got is None
        else:
            assert self.got is self.damax
            assert_bits("%s amax" % what, self.damax.cpu().numpy(), amax)
        for tag, t, a in (("thl", self.dthl, c["thl"]), ("qt", self.dqt, c["qt"]), ("ql", self.dql, c["ql"]), ("hx", self.dhx, c["hx"]),
                          ("hy", self.dhy, c["hy"]), ("t0", self.dt0, c["t0"]), ("lex", self.dlex, c["lex"]), ("s", self.ds, c["s"])):
            assert t is None or Poisoned.read_only(t, a), (what, tag, "read only")
        self.mem.check_around(what)
        return want


PTRS = ("thl", "qt", "ql", "u", "v", "hx", "hy", "t0", "lex", "s", "phi", "psfc", "amax")
INPUTS = ("thl", "qt", "ql", "hx", "hy", "t0", "lex", "s")
WRITTEN = ("phi", "u", "v", "psfc", "amax")


def raw_launch(eng, c, alias=None, extents=None, null=()):
    """spc_les_buoyancy_* itself: (rc, dict name -> host array of phi, u, v, psfc, amax).  ``alias``: (member, key) pairs that
    replace a pointer member by that of tensor ``key``; ``extents``: overrides of the scalar members; ``null``: members set to
    NULL"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    n, itot, jtot, ktot = c["thl"].shape
    t = {k: dev(c[k]) for k in ("thl", "qt", "ql", "u", "v", "hx", "hy", "t0", "lex", "s")}
    t["phi"] = dev(numpy.full_like(c["thl"], OUT_FILL))
    t["psfc"] = dev(numpy.full(c["thl"].shape[:3], OUT_FILL, dtype=c["thl"].dtype))
    t["amax"] = dev(numpy.full_like(c["hx"], -5.0))
    a = _abi.LesBuoyancyArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.pitch_prof, a.c1, a.c2 = n, itot, jtot, ktot, ktot, buo.C1, buo.C2
    fill_args(a, t, PTRS, alias, extents, null)
    rc = abi_call(eng, "spc_les_buoyancy", a)
    return rc, {k: t[k].cpu().numpy() for k in PTRS}


def derived_cols(ktot, esize):
    """the columns per workgroup that follow from the tile's pitch ktot | 1: the largest of 64 and 32 whose tile fits 64 KiB (two
    workgroups and more per CU), 16 where 16 columns fit the 160 KiB of a CU, else 0"""
    col = (ktot | 1) * esize
    return 64 if 64 * col <= 64 * 1024 else 32 if 32 * col <= 64 * 1024 else 16 if 16 * col <= 160 * 1024 else 0


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """phi, psfc, u, v and amax against the oracle with everything asked for and with no ql, psfc and amax; the answer is not the
    input where a cell has two different neighbours"""
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    assert (c["ql"] > 0).any() and (c["ql"] == 0).any() and (c["hx"] != c["hy"]).all()
    what = "n %d plane %s ktot %d" % (n, plane, ktot)
    phi, psfc, un, vn, amax = Run(eng, c).check(what)
    Run(eng, c, ql=False, psfc=False, amax=False).check(what + " bare")
    assert (amax >= 0).all() and not numpy.signbit(amax).any()
    if plane[0] > 2:
        assert (un != c["u"]).any() and (amax > 0).all()
    else:
        assert_bits("itot <= 2 keeps u", un, c["u"])
    if plane[1] > 2:
        assert (vn != c["v"]).any() and (amax > 0).all()
    else:
        assert_bits("jtot <= 2 keeps v", vn, c["v"])
    if max(plane) <= 2:
        assert_bits("amax of a plane without a gradient", amax, numpy.zeros_like(amax))


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 3 x 5: t0, lex, s, hx and hy differ per LES and hx from hy, so a wrong l or a swapped coefficient shows; then
    the same with pitched profiles"""
    for n in NS:
        for pad in (0, 3):
            c = case((n, 3, 5, ktot), np_of(eng), seed=1)
            assert (c["hx"] != c["hy"]).all()
            if n > 1:
                assert not numpy.array_equal(c["t0"][0], c["t0"][1]) and c["hx"][0] != c["hx"][1] and not numpy.array_equal(c["s"][0], c["s"][1])
            Run(eng, c, pad=pad).check("rows n %d ktot %d pad %d" % (n, ktot, pad))


def check_tiles(eng):
    """for every C of spc_les_buoyancy_cols_per_block: C - 1, C, C + 1 and 2 C + 1 columns, as one LES of 1 x cols columns (a
    tile ends inside a row), as cols LES of one column (l per lane) and as LES of 1 x 3 (a tile ends inside an LES); ktot on
    both sides of every change of C; 17 columns at the last supported ktot; the first unsupported ktot refused.  The thresholds
    the library reports are the ones that follow from the LDS and the pitch (derived_cols)."""
    dtype = np_of(eng)
    esize = numpy.dtype(dtype).itemsize
    first, changes, bad = table = cols_table(eng.buoyancy_cols_per_block)
    assert table == cols_table(lambda k: derived_cols(k, esize))
    assert sorted(first) == [16, 32, 64] and len(changes) == 2
    for C, k0 in first.items():
        ktot = 7 if C == 64 else k0
        assert eng.buoyancy_cols_per_block(ktot) == C
        for cols in (C - 1, C, C + 1, 2 * C + 1):
            shapes = [(1, 1, cols, ktot), (cols, 1, 1, ktot)] + ([(cols // 3, 1, 3, ktot)] if cols % 3 == 0 else [])
            for shape in shapes:
                Run(eng, case(shape, dtype, seed=3)).check("tiles %s C %d" % (shape, C))
    for ktot in changes:
        for k in (ktot - 1, ktot):
            Run(eng, case((2, 2, 3, k), dtype, seed=4)).check("change at ktot %d: %d" % (ktot, k))
    Run(eng, case((1, 1, 17, bad - 1), dtype, seed=5)).check("17 columns at the last ktot %d" % (bad - 1))
    rc, out = raw_launch(eng, case((1, 1, 2, bad), dtype, seed=5))
    assert rc == _abi.SPC_ERR_UNSUPPORTED and str(bad - 1).encode() in eng.lib.spc_last_error(), (rc, eng.lib.spc_last_error())
    assert (out["phi"] == OUT_FILL).all() and (out["psfc"] == OUT_FILL).all() and (out["amax"] == -5.0).all()
    return table


def strip_shapes(strip):
    """(n, itot, jtot, ktot) whose run jtot * ktot stands one below, at and one above a strip, for every itot of ROWS; the run as
    one level of many j once; and a launch of many workgroups, which walks more rows"""
    out = []
    for run in (strip - 1, strip, strip + 1):
        jtot = next(q for q in (5, 4, 3, 2, 1) if run % q == 0)
        out += [(2, itot, jtot, run // jtot) for itot in ROWS]
        out.append((2, 3, run, 1))
    out.append((lar.MANY, 33, 1, 1))
    return out


def check_strips(eng):
    """the seams of k_les_pgrad: the flat run of a row at the strip - 1, + 0, + 1 (the j neighbours of a cell lie in another
    workgroup or across the wrap), rows below, at and above what a workgroup walks"""
    strip, rows = eng.advect_strip(2, 8, 8, 160)
    assert strip >= 64 and 1 <= rows < 33
    for shape in strip_shapes(strip):
        Run(eng, case(shape, np_of(eng), seed=2)).check("strip %d x %d x %d x %d" % shape)
    return strip, rows


def check_outputs(eng):
    """with and without ql, psfc and amax: phi, u and v do not depend on psfc and amax, and what is not asked for is not written;
    the C entry point itself"""
    for ktot in (2, 65):
        c = case((2, 3, 4, ktot), np_of(eng), seed=6)
        for ql in (True, False):
            for psfc in (True, False):
                for amax in (True, False):
                    Run(eng, c, ql=ql, psfc=psfc, amax=amax).check("ql %s psfc %s amax %s ktot %d" % (ql, psfc, amax, ktot))
    assert (oracle(c)[0] != oracle(c, ql=False)[0]).any()
    rc, got = raw_launch(eng, c)
    assert rc == 0
    for tag, w in zip(("phi", "psfc", "u", "v", "amax"), oracle(c)):
        assert_bits("raw " + tag, got[tag], w)


def check_alignment(eng, leads, ktot=65, pad=0):
    """views off the 16-byte grid: all equally (the 16-byte mover with a head and a tail) or each on its own (single elements)"""
    c = case((3, 2, 3, ktot), np_of(eng), seed=sum(leads) + 10 * pad)
    Run(eng, c, leads=leads, pad=pad).check("leads %s pad %d ktot %d" % (leads, pad, ktot))


COLTILE_KTOTS = (1, 2, 7, 8, 9, 17)


def check_coltile(eng):
    """the cases of the column tile (spc_coltile.hpp) together: 3 LES of 3 x 5 (one partial tile that spans three LES, more than
    DIF_STAGE) and 6 of them (a whole 64-column tile that spans five LES, then a partial one); ktot 1, 2, 7, 8, 9 and 17, and at
    n = 3 the last ktot of every C and the first of the next; thl, qt, ql and phi led by 0 ... V - 1 elements, equally and each on its own (coltile_leads of les_radiate_ref);
    the bytes around every array are looked at by Run.check"""
    dtype = np_of(eng)
    V = 16 // numpy.dtype(dtype).itemsize
    for n in (3, 6):
        for ktot in COLTILE_KTOTS:
            for leads in lrr.coltile_leads(V, 4):
                Run(eng, case((n, 3, 5, ktot), dtype, seed=11 + sum(leads)), leads=leads).check("coltile n %d ktot %d leads %s" % (n, ktot, leads))
    first, changes, bad = cols_table(eng.buoyancy_cols_per_block)
    for ktot in [k for c in changes for k in (c - 1, c)] + [bad - 1]:
        for leads in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 0, 0)):
            Run(eng, case((3, 3, 5, ktot), dtype, seed=12), leads=leads).check("coltile C %d ktot %d leads %s" % (eng.buoyancy_cols_per_block(ktot), ktot, leads))


def uniform_case(dtype, shape=(2, 3, 4, 9)):
    """a state that is uniform on every level of every LES; some winds are -0.0"""
    c = case(shape, dtype, seed=7)
    for key in ("thl", "qt", "ql"):
        c[key][...] = c[key][:, :1, :1, :]
    c["u"][0, 0, 0, :] = -0.0
    c["v"][-1, -1, -1, ::2] = -0.0
    return c


NAN_CELL = (0, 2, 3, 4)                                            # (l, i, j, k) of the thl cell that holds the NaN


def nan_case(dtype, shape=(2, 5, 6, 7)):
    """(clean case, the same with a NaN in the thl cell NAN_CELL)"""
    c = case(shape, dtype, seed=8)
    s = dict(c, thl=c["thl"].copy())
    s["thl"][NAN_CELL] = numpy.nan
    return c, s


def nan_reach(shape):
    """boolean masks (phi, u, v) of the cells that the NaN of NAN_CELL reaches: its own column from its level down; the two
    i-neighbour columns of u and the two j-neighbour columns of v at those levels"""
    l, i, j, k = NAN_CELL
    phi, u, v = (numpy.zeros(shape, dtype=bool) for _ in range(3))
    phi[l, i, j, :k + 1] = True
    for d in (-1, 1):
        u[l, (i + d) % shape[1], j, :k + 1] = True
        v[l, i, (j + d) % shape[2], :k + 1] = True
    return phi, u, v


def check_nan_reach(clean, got, shape):
    """``got`` (phi, psfc, u, v, amax of the case with the NaN) is NaN exactly where nan_reach says and keeps the bits of
    ``clean`` everywhere else; amax of the NaN's LES is a NaN, the other LES's keeps its bits"""
    l, i, j, _ = NAN_CELL
    for tag, a, b, mask in zip(("phi", "u", "v"), (got[0], got[2], got[3]), (clean[0], clean[2], clean[3]), nan_reach(shape)):
        assert numpy.isnan(a[mask]).all() and not numpy.isnan(a[~mask]).any(), tag
        assert_bits("the other cells: " + tag, a[~mask], b[~mask])
    others = numpy.ones(shape[:3], dtype=bool)
    others[l, i, j] = False
    assert numpy.isnan(got[1][l, i, j])
    assert_bits("the other columns: psfc", got[1][others], clean[1][others])
    assert numpy.isnan(got[4][l]) and not numpy.isnan(got[4][1 - l])
    assert_bits("amax of the other LES", got[4][1 - l:2 - l], clean[4][1 - l:2 - l])


def check_special(eng):
    """the uniform state (every wind keeps its bits, -0.0 included, amax = +0, phi the same in every column) and the NaN's reach"""
    dtype = np_of(eng)
    c = uniform_case(dtype)
    phi, psfc, un, vn, amax = Run(eng, c).check("uniform")
    assert_bits("uniform: u", un, c["u"])
    assert_bits("uniform: v", vn, c["v"])
    assert_bits("uniform: amax", amax, numpy.zeros_like(amax))
    assert_bits("uniform: phi", phi, numpy.broadcast_to(phi[:, :1, :1, :], phi.shape))
    c, s = nan_case(dtype)
    clean = Run(eng, c).check("clean")
    r = Run(eng, s)
    r.check("nan")
    got = [t.cpu().numpy() for t in (r.dphi, r.dpsfc, r.du, r.dv, r.damax)]
    check_nan_reach(clean, got, c["thl"].shape)


def check_refusals(eng):
    """n = 0 is a no-op; pitch_prof < ktot, a NULL required pointer, and phi, u, v, psfc or amax equal to an input or to each other
    are refused by the library; the engine refuses the same aliases and bad shapes; no refused call writes"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=13)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731

    def untouched(out, but=()):
        for k in ("u", "v"):
            if k not in but:
                assert_bits("refused: " + k, out[k], c[k])
        assert all((out[k] == fill).all() for k, fill in (("phi", OUT_FILL), ("psfc", OUT_FILL), ("amax", -5.0)) if k not in but)
    rc, out = raw_launch(eng, c, extents=dict(n_les=0))
    assert rc == 0
    untouched(out)
    rc, out = raw_launch(eng, c, null=("ql", "psfc", "amax"))
    assert rc == 0 and (out["psfc"] == OUT_FILL).all() and (out["amax"] == -5.0).all()
    assert_bits("without ql", out["phi"], oracle(c, ql=False)[0])
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    bad = [(dict(extents=dict(pitch_prof=7)), b"pitch_prof")]
    bad += [(dict(alias=((out_, key),)), b"also an input") for out_ in WRITTEN for key in INPUTS]
    bad += [(dict(alias=((WRITTEN[y], WRITTEN[x]),)), b"same array") for x in range(5) for y in range(x + 1, 5)]
    bad += [(dict(null=(k,)), b"required pointer " + k.encode()) for k in ("thl", "qt", "u", "v", "phi", "hx", "hy", "t0", "lex", "s")]
    for kw, text in bad:
        rc, out = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        untouched(out, but=[m for m, _ in kw.get("alias", ())] + list(kw.get("null", ())))
    t = {k: dev(c[k]) for k in ("thl", "qt", "ql", "u", "v", "hx", "hy", "t0", "lex", "s")}
    phi, psfc = torch.empty_like(t["thl"]), torch.empty_like(t["thl"][..., 0])
    args = tuple(t[k] for k in ("thl", "qt", "ql", "u", "v", "hx", "hy", "t0", "lex", "s"))
    assert eng.les_buoyancy(*[x[:0] for x in args], phi[:0]) is not None
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    for call in (lambda: eng.les_buoyancy(*args, t["thl"]),
                 lambda: eng.les_buoyancy(*args, t["u"]),
                 lambda: eng.les_buoyancy(*args[:3], t["u"], t["u"], *args[5:], phi),
                 lambda: eng.les_buoyancy(*args[:3], t["qt"], *args[4:], phi),
                 lambda: eng.les_buoyancy(*args, phi, psfc=phi[..., 0]),
                 lambda: eng.les_buoyancy(*args, phi, psfc=psfc[:1]),
                 lambda: eng.les_buoyancy(*args, phi, amax=t["hx"]),
                 lambda: eng.les_buoyancy(*args[:7], t["t0"][:, :4], *args[8:], phi),
                 lambda: eng.les_buoyancy(*args[:5], t["hx"][:1], *args[6:], phi),
                 lambda: eng.les_buoyancy(*args, phi[..., ::2]),
                 lambda: eng.les_buoyancy(*args, phi.to(other)),
                 lambda: eng.les_buoyancy(t["thl"].cpu(), *args[1:], phi)):
        try:
            call()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    for k in ("thl", "qt", "ql", "u", "v"):
        assert_bits("refused: " + k, t[k].cpu().numpy(), c[k])


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    c = case((n, 3, 4, 40), np_of(one), seed=n)
    want = oracle(c)
    for tag, eng, up in on_both(one, multi, n):
        t = {k: up(c[k]) for k in ("thl", "qt", "ql", "u", "v", "hx", "hy", "t0", "lex", "s")}
        phi, psfc = up(numpy.full_like(c["thl"], OUT_FILL)), up(numpy.full(c["thl"].shape[:3], OUT_FILL, dtype=c["thl"].dtype))
        amax = eng.les_buoyancy(*[t[k] for k in ("thl", "qt", "ql", "u", "v", "hx", "hy", "t0", "lex", "s")], phi, psfc=psfc)
        multi.synchronize()
        for k, got, w in zip(("phi", "psfc", "u", "v", "amax"), (phi, psfc, t["u"], t["v"], amax), want):
            assert_bits("%s %s" % (tag, k), host_of(got), w)
    return blocks_of(t["u"], multi, n)


BODIES = ("parity", "rows", "tiles", "coltile", "strips", "outputs", "alignment", "special", "refusals")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (1, 2, 65)]),
            ("rows", lambda: [check_rows(eng, k) for k in (2, 65)]),
            ("tiles", lambda: check_tiles(eng)),
            ("coltile", lambda: check_coltile(eng)),
            ("strips", lambda: check_strips(eng)),
            ("outputs", lambda: check_outputs(eng)),
            ("alignment", lambda: [check_alignment(eng, *a) for a in (((1, 1, 1, 1), 65, 0), ((1, 0, 3, 2), 64, 0), ((3, 3, 3, 1), 7, 5))]),
            ("special", lambda: check_special(eng)),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_buoyancy (CPU suite) -----------------------------------------------------------------------
class BuoyancyOracleEngine(lrr.RadiateOracleEngine):
    """tests/les_radiate_ref.RadiateOracleEngine with ``les_buoyancy`` by the NumPy oracle above: u and v updated in place, phi
    and psfc written whole into the caller's tensors, as the HIP engine does"""

    def les_buoyancy(self, thl, qt, ql, u, v, hx, hy, t0, lex, s, phi, psfc=None, amax=True, **kw):
        want = amax is not None and amax is not False
        written = [t.data_ptr() for t in (phi, u, v, psfc, amax if want and amax is not True else None) if t is not None]
        read = {t.data_ptr() for t in (thl, qt, ql, hx, hy, t0, lex, s) if t is not None}
        if thl.shape[0] and (len(set(written)) != len(written) or set(written) & read):
            raise ValueError("phi, u, v, psfc or amax is an input or another of them")
        c = lambda t: numpy.ascontiguousarray(t.numpy())                                     # noqa: E731
        f, q, un, vn, am = les_buoyancy(thl.numpy(), qt.numpy(), None if ql is None else ql.numpy(), u.numpy(), v.numpy(), hx.numpy(), hy.numpy(),
                                        c(t0), c(lex), c(s))
        phi.copy_(torch.from_numpy(f))
        u.copy_(torch.from_numpy(un))
        v.copy_(torch.from_numpy(vn))
        if psfc is not None:
            psfc.copy_(torch.from_numpy(q))
        if not want:
            return None
        am = torch.from_numpy(am)
        return am if amax is True else amax.copy_(am)


# -- the host twins of models.DeviceLESEnsemble after enable_buoyancy() ----------------------------------------------------------
class _HostBuoyancy:
    """NumPy fields: the executable definition of what the advection of evolve_model_batched does after enable_buoyancy(): QL
    and the slab means of the stepped fields, the profiles of those means, K16's and K17's probes with the coefficients of the
    whole step, the substeps of the probes or of the gravity wave, whichever are more, then per substep K21 on the winds, K16
    and K17"""

    buoyancy_wave_speed = None
    buoyancy_wind_change = None
    _phi = None

    def enable_buoyancy(self, wave_speed=None):
        if not getattr(self, "advect_vertical", False) or self.advect_par is None:
            raise ValueError("the pressure force (K21) needs enable_advection(..., vertical=True)")
        self.buoyancy_wave_speed = buo.WAVE_SPEED if wave_speed is None else float(wave_speed)

    def _advect(self, dt):
        if self.buoyancy_wave_speed is None:
            return super()._advect(dt)
        f, p, par = self.fields3d, self.p, self.advect_par
        if self.THERMO:
            self._stale = True
            self._ensure_ql()
        elif "QL" in f or ("QT" in f and "Qsat" in f):
            f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
        self._slab_means()
        T = f["U"].dtype
        ql = f.get("QL")
        t0, lex, s = (a.astype(T) for a in buo.profiles(p["THL"], p["QT"], p["QL"] if ql is not None else None, p["presf"], self.zh_cache,
                                                        zf=self.zf_cache))
        g, r = (a.astype(T) for a in adv.vertical_profiles(self.water_path_weights()))
        hx, hy = (a.astype(T) for a in adv.coefficients(dt, par["dx"], par["dy"], n=self.n))
        c = float(lar.faces(f["U"], f["V"], hx, hy)[4].max())
        c = max(c, float(lvr.face_numbers(lvr.mass_flux(f["U"], f["V"], hx, hy, g), r)[2].max()))
        n_sub = adv.substeps(c, par["cfl"], par["max_substeps"])
        n_wave = buo.wave_substeps(dt, par["dx"], par["dy"], par["cfl"], self.buoyancy_wave_speed)
        if n_wave > par["max_substeps"]:
            raise RuntimeError("the pressure force (K21) needs %d substeps" % n_wave)
        n_sub = max(n_sub, n_wave)
        hx, hy = (a.astype(T) for a in adv.coefficients(dt / n_sub, par["dx"], par["dy"], n=self.n))
        worst = worst_z = worst_b = 0.0
        for _ in range(n_sub):
            self._phi, _, f["U"], f["V"], amax = les_buoyancy(f["THL"], f["QT"], ql, f["U"], f["V"], hx, hy, t0, lex, s)
            worst_b = max(worst_b, float(amax.max()))
            new, cmax = lar.les_advect({k: f[k] for k in self.KEYS if k in f}, f["U"], f["V"], hx, hy)
            f.update(new)
            worst = max(worst, float(cmax.max()))
            new, cmax, self._mtop = lvr.les_vadvect({k: f[k] for k in self.KEYS if k in f}, f["U"], f["V"], hx, hy, g, r)
            f.update(new)
            worst_z = max(worst_z, float(cmax.max()))
        self.advect_substeps, self.advect_courant, self.advect_courant_z, self._mtop_dt = n_sub, worst, worst_z, dt / n_sub
        self.buoyancy_wind_change = worst_b

    def get_pressure_batched(self):
        return self._phi


class HostBuoyancyLESEnsemble(_HostBuoyancy, lrr.HostRadiateLESEnsemble):
    """without enable_thermo(): QL = max(QT - Qsat, 0)"""


class HostThermoBuoyancyLESEnsemble(_HostBuoyancy, lrr.HostThermoRadiateLESEnsemble):
    """after enable_thermo(): K12's oracle gives the QL that K21 reads"""


VARIANTS = {"plain": dict(), "all": dict(diffuse=True, radiate=True, thermo=True, micro=True)}
DX = lvr.DX


def ensemble_run(engine, n, device, buoyancy=True, thermo=False, micro=False, diffuse=False, radiate=False, wave_speed=None, itot=4, jtot=5,
                 nL=20, steps=3):
    """an ensemble with attached U, V, THL, QT (and Qsat, or thermo; QR with the microphysics), enable_advection(vertical=True)
    and enable_buoyancy() (``buoyancy`` None: never called, and the host twin is the one of the K18 tests) through ``steps`` calls
    of evolve_model_batched and one variability nudge (constantT) before the last; after each of them every profile, the fields,
    the substeps, phi and the largest wind change.  Returns (ens, list of records)"""
    if device:
        cls = models.DeviceLESEnsemble
    elif buoyancy:
        cls = HostThermoBuoyancyLESEnsemble if thermo else HostBuoyancyLESEnsemble
    else:
        cls = lrr.HostThermoRadiateLESEnsemble if thermo else lrr.HostRadiateLESEnsemble

    def enable(ens):
        if buoyancy:
            ens.enable_buoyancy(**({} if wave_speed is None else {"wave_speed": wave_speed}))

    def record(ens, rec):
        lar.record_substeps(ens, rec, z=True)
        if buoyancy:
            record_pressure(ens, rec)

    def before(ens):
        assert not buoyancy or ens.get_pressure_batched() is None
    return ensemble_case(engine, n, cls, thermo=thermo, micro=micro, diffuse=diffuse, edit=lvr.raise_u, advection=dict(dx=DX, dy=1.5 * DX, vertical=True),
                         radiation=lrr.radiation_of(n, "f0", "f1") if radiate else None, enable=enable, record=record, before=before,
                         itot=itot, jtot=jtot, nL=nL, steps=steps)


def record_pressure(ens, rec):
    """phi (zeros before the first step) and the largest wind change of the last step into a record of ensemble_case"""
    phi = ens.get_pressure_batched()
    rec["phi"] = numpy.zeros(rec["field U"].shape) if phi is None else numpy.array(host_of(phi))
    rec["wind change"] = numpy.array([-1.0 if ens.buoyancy_wind_change is None else ens.buoyancy_wind_change])


def check_ensemble(one, engines, n, variant):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``: every profile, field and phi
    bit-equal after each step; the pressure force moves the winds: U of the twin's first step differs from the same run without
    enable_buoyancy(), whose device run is bit-equal to today's twin as well.  Returns the twin's substeps per step"""
    kw = VARIANTS[variant]
    host = ensemble_run(one, n, False, **kw)[1]
    plain = ensemble_run(one, n, False, buoyancy=None, **kw)[1]
    assert (host[1]["field U"] != plain[1]["field U"]).any() and (host[1]["phi"] != 0).any()
    assert 0 < host[1]["wind change"][0] and all(numpy.isfinite(r["wind change"][0]) for r in host)
    for engine in engines:
        lmr.same_logs(host, ensemble_run(engine, n, True, **kw)[1])
    lmr.same_logs(plain, ensemble_run(engines[0], n, True, buoyancy=None, **kw)[1])
    return [int(r["substeps"][0]) for r in host if r["substeps"][0] > 0]
