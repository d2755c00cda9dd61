"""NumPy oracle of K15 (include/spc.h: spc_les_diffuse_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_diffuse_gpu.py (each takes an engine: tools/mutation_control.py --diffuse hands them the engines of its mutant
libraries), the host twins of models.DeviceLESEnsemble's diffusion mode and an oracle-backed engine with ``les_diffuse`` for
the CPU suite.

The oracle spells the rule out one operation per NumPy call in the element type, vectorised over the columns, a Python loop
over k, so nothing fuses.  Every device array of the bodies is the LEADING part of a poisoned buffer
(tests/les_harness.Poisoned); the bytes behind it (and in front of a view off the 16-byte grid) are checked after the launch."""

import numpy
import torch

from sp_coupler_amd import _abi, models
from sp_coupler_amd import diffusion as df
from tests import les_micro_ref as lmr
from tests import les_thermo_ref as ltr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, WQ, WT, abi_call, blocks_of, ensemble_case, host_of, np_of, on_both, run_bodies)

#: tiles that hold many LES (1 x 1), tiles that straddle LES (3 x 5), a tile that is exactly one LES (8 x 8 at 64 columns per
#: workgroup), an LES of more than one tile plus a partial one (9 x 9)
PLANES = [(1, 1), (3, 5), (8, 8), (9, 9)]
#: no sweep at all (1), shorter than one chunk of 8 levels, one chunk and one more level (9), whole chunks plus 7, 0 and 1
#: levels (64, 65, 66 levels after level 0 -> 63, 64, 65), the flagship's 160 and an odd neighbour (pitch == ktot)
KTOTS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 160, 161]
NS = [1, 2, 5]
NAMES = ("U", "V", "THL", "QT")


# -- the rule --------------------------------------------------------------------------------------------------------------
def les_diffuse(x, a, m, cp, s0=None, flux=None):
    """the new field (a new array): x [n x itot x jtot x ktot] of dtype T, a, m, cp [n x ktot], s0 and flux [n] of the same T"""
    T = x.dtype
    assert all(p.dtype == T for p in (a, m, cp)) and (flux is None or (s0.dtype == T and flux.dtype == T))
    ktot = x.shape[-1]
    b = lambda p, k: p[:, k][:, None, None]                                              # noqa: E731
    y = numpy.empty_like(x)
    with numpy.errstate(all="ignore"):
        d = x[..., 0]
        if flux is not None:
            t = s0 * flux
            d = d + t[:, None, None]
        y[..., 0] = d * b(m, 0)
        for k in range(1, ktot):
            t = b(a, k) * y[..., k - 1]
            r = x[..., k] - t
            y[..., k] = r * b(m, k)
        for k in range(ktot - 2, -1, -1):
            t = b(cp, k) * y[..., k + 1]
            y[..., k] = y[..., k] - t
    assert y.dtype == T
    return y


# -- inputs ------------------------------------------------------------------------------------------------------------------
def grid(n, ktot, rng):
    """(zh, zf, rhobf, h_mix) of LES with layers of 20 ... 30 m, another density profile and another mixed layer per LES"""
    dz = 20.0 + 10.0 * rng.random((n, ktot))
    if ktot > 1:
        dz[:, -1] = dz[:, -2]
    zh = numpy.concatenate([numpy.zeros((n, 1)), numpy.cumsum(dz, axis=1)[:, :-1]], axis=1)
    zf = zh + 0.5 * dz
    rhobf = (1.0 + 0.3 * rng.random((n, 1))) * numpy.exp(-zf / (7000.0 + 3000.0 * rng.random((n, 1))))
    h_mix = 300.0 + 2000.0 * rng.random((n, 1))
    return zh, zf, rhobf, h_mix


def grid_profiles(n, ktot, dtype, rng, dt):
    """(a, m, cp, s0) in ``dtype`` by diffusion.profiles: rows that differ per LES"""
    zh, zf, rhobf, h_mix = grid(n, ktot, rng)
    return tuple(numpy.ascontiguousarray(p.astype(dtype)) for p in df.profiles(zh, zf, rhobf, dt, h_mix=h_mix))


def field_like(name, shape, dtype, rng):
    z = numpy.arange(shape[-1]) / 160.0
    if name == "QT":
        return (8e-3 * numpy.exp(-z) + 1e-3 * rng.random(shape)).astype(dtype)
    if name == "THL":
        return (290.0 + 10.0 * z + 0.5 * rng.standard_normal(shape)).astype(dtype)
    return (5.0 + 3.0 * z + rng.standard_normal(shape)).astype(dtype)


def case(shape, dtype, seed=0, dt=60.0, names=NAMES, fluxes=("THL", "QT")):
    """dict of the arguments: fields (dict name -> array), prof (a, m, cp, s0), flux (dict name -> [n])"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(5000 + seed + 7 * ktot + itot * jtot + 31 * n)
    prof = grid_profiles(n, ktot, dtype, rng, dt)
    fields = {k: field_like(k, shape, dtype, rng) for k in names}
    scale = {"THL": 0.2, "QT": 2e-4, "U": 0.1, "V": 0.1}
    flux = {k: (scale[k] * (0.25 + rng.random(n))).astype(dtype) for k in fluxes if k in names}
    return dict(fields=fields, prof=prof, flux=flux, dt=dt)


def oracle(c):
    a, m, cp, s0 = c["prof"]
    return {k: les_diffuse(x, a, m, cp, s0 if k in c["flux"] else None, c["flux"].get(k)) for k, x in c["fields"].items()}


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one launch through ``eng.les_diffuse`` with every array inside a poisoned buffer; ``check`` compares the fields with the
    oracle bit for bit, the profiles, s0 and the fluxes with what was uploaded, and looks at the bytes around every array"""

    def __init__(self, eng, c, lead=0, pad=0, lead_rows=0, with_s0=True):
        self.eng, self.c, self.pad = eng, c, pad
        first = next(iter(c["fields"].values()))
        dtype, (n, ktot) = first.dtype, (first.shape[0], first.shape[-1])
        self.mem = Poisoned(eng)
        put = self.mem.put
        rows = lambda tag, a, poison, lead: self.mem.rows(tag, a, poison, lead, pad)        # noqa: E731
        self.dev = {k: put(k, x, float("nan"), lead) for k, x in c["fields"].items()}
        self.dprof = [rows("prof %d" % i, a, 1e30, lead_rows) for i, a in enumerate(c["prof"][:3])]
        self.ds0 = put("s0", c["prof"][3], 1e30, lead_rows) if with_s0 else None
        self.dflux = {k: put("flux " + k, v, 1e30, lead_rows) for k, v in c["flux"].items()}
        self.got = eng.les_diffuse(self.dev, *self.dprof, s0=self.ds0, flux=self.dflux)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        c = self.c
        want = oracle(c)
        assert self.got is None
        for k in c["fields"]:
            assert_bits("%s %s" % (what, k), self.dev[k].cpu().numpy(), want[k])
        same = Poisoned.read_only
        for t, a in zip(self.dprof, c["prof"]):
            assert same(t, a), (what, "a profile", "read only")
        assert self.ds0 is None or same(self.ds0, c["prof"][3]), (what, "s0", "read only")
        for k, t in self.dflux.items():
            assert same(t, c["flux"][k]), (what, "flux " + k, "read only")
        self.mem.check_around(what)
        return want


def raw_launch(eng, c, names=None, flux=None, s0=True, alias=None):
    """spc_les_diffuse_* itself: (rc, dict name -> host array).  ``flux``: the names whose flux is passed (default: all of the
    case); ``s0`` False: NULL; ``alias``: (slot, tensor key) pairs that replace fields[slot] by another argument's pointer"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    names = list(c["fields"]) if names is None else list(names)
    first = c["fields"][names[0]]
    n, itot, jtot, ktot = first.shape
    t = {k: dev(c["fields"][k]) for k in names}
    t.update({k: dev(a) for k, a in zip(("a", "m", "cp", "s0"), c["prof"])})
    fl = {k: dev(v) for k, v in c["flux"].items() if k in names and (flux is None or k in flux)}
    g = _abi.LesDiffuseArgs()
    g.n_les, g.itot, g.jtot, g.ktot, g.n_fields, g.pitch_prof = n, itot, jtot, ktot, len(names), ktot
    g.a, g.m, g.cp = t["a"].data_ptr(), t["m"].data_ptr(), t["cp"].data_ptr()
    if s0:
        g.s0 = t["s0"].data_ptr()
    for f, k in enumerate(names):
        g.fields[f] = t[k].data_ptr()
        if k in fl:
            g.flux[f] = fl[k].data_ptr()
    for slot, key in (alias or ()):
        g.fields[slot] = t[key].data_ptr()
    rc = abi_call(eng, "spc_les_diffuse", g)
    return rc, {k: t[k].cpu().numpy() for k in names}


def boundaries(cols_of):
    """from ``cols_of(ktot)`` (spc_les_diffuse_cols_per_block): [(ktot, C)] of the last ktot of each C and the first of the next,
    the largest supported ktot, and one above it (C == 0)"""
    out, k = [], 1
    c = cols_of(1)
    assert c == 64
    while c:
        lo, hi = k, 1 << 20                                       # the last ktot with cols_of == c: the choice is monotone
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if cols_of(mid) == c else (lo, mid)
        out.append((lo, c))
        k = lo + 1
        c = cols_of(k)
        assert c in (0, 16, 32) and c < out[-1][1]
        out.append((k, c))
    return out


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """four fields, THL and QT with a flux, against the oracle; the answer is not the input"""
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    want = Run(eng, c).check("n %d plane %s ktot %d" % (n, plane, ktot))
    assert all((want[k] != c["fields"][k]).any() for k in (NAMES if ktot > 1 else ("THL", "QT")))       # (one level: only a flux changes it)
    assert (want["THL"][..., 0] > c["fields"]["THL"][..., 0]).any()


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 3 x 5: the coefficient rows differ per LES (another density and another mixed layer), so a wrong l shows"""
    for n in NS:
        c = case((n, 3, 5, ktot), np_of(eng), seed=1)
        if n > 1 and ktot > 1:
            assert not numpy.array_equal(c["prof"][1][0], c["prof"][1][1])
        Run(eng, c).check("rows n %d ktot %d" % (n, ktot))


def check_boundaries(eng):
    """every boundary of spc_les_diffuse_cols_per_block at plane 3 x 5, n = 2: the last ktot of each C, the first of the next,
    the largest supported one, and one above it, which is refused with a text that names the limit"""
    bounds = boundaries(eng.diffuse_cols_per_block)
    assert [c for _, c in bounds] == [64, 32, 32, 16, 16, 0], bounds
    for ktot, cols in bounds:
        c = case((2, 3, 5, ktot), np_of(eng), seed=2, names=("THL", "QT"))
        if cols:
            Run(eng, c).check("boundary ktot %d C %d" % (ktot, cols))
            continue
        try:
            Run(eng, c)
        except _abi.SpcError as e:
            assert e.code == _abi.SPC_ERR_UNSUPPORTED and str(ktot - 1) in str(e), str(e)
        else:
            raise AssertionError("ktot %d was not refused" % ktot)
    return bounds


def check_tiles(eng, ktot):
    """column counts C q + r, r in {0, 1, C - 1}: as one LES of 1 x (C q + r) columns and as C q + r LES of one column (l per lane)"""
    C = eng.diffuse_cols_per_block(ktot)
    for cols in (1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 3 * C - 1):
        for shape in ((1, 1, cols, ktot), (cols, 1, 1, ktot)):
            Run(eng, case(shape, np_of(eng), seed=3, names=("THL",))).check("tiles %s C %d" % (shape, C))


def check_fields(eng):
    """1 to 4 fields; each flux NULL on its own; all NULL with s0 NULL; a flux for U as well"""
    dtype = np_of(eng)
    for nf in (1, 2, 3, 4):
        Run(eng, case((2, 3, 5, 64), dtype, seed=4, names=NAMES[-nf:])).check("%d fields" % nf)
    for fluxes in (("THL",), ("QT",), (), ("U", "V", "THL", "QT")):
        Run(eng, case((2, 3, 5, 65), dtype, seed=5, fluxes=fluxes)).check("fluxes %s" % (fluxes,))
    Run(eng, case((2, 3, 5, 65), dtype, seed=5, fluxes=()), with_s0=False).check("no flux, no s0")
    c = case((2, 3, 5, 9), dtype, seed=6)
    want = oracle(dict(c, flux={"QT": c["flux"]["QT"]}))
    rc, got = raw_launch(eng, c, flux=("QT",))
    assert rc == 0
    for k in NAMES:
        assert_bits("raw %s" % k, got[k], want[k])


def check_alignment(eng, lead, lead_rows, pad, ktot=65):
    """views one (or more) elements off the 16-byte grid and pitched profiles"""
    c = case((3, 3, 5, ktot), np_of(eng), seed=lead + 10 * lead_rows + 100 * pad)
    Run(eng, c, lead=lead, lead_rows=lead_rows, pad=pad).check("lead %d %d pad %d ktot %d" % (lead, lead_rows, pad, ktot))


COLTILE_KTOTS = (1, 2, 7, 8, 9, 17)


def check_coltile(eng):
    """the cases of the column tile (spc_coltile.hpp) together: 3 LES of 3 x 5 (one partial tile that spans three LES, more than
    DIF_STAGE) and 6 of them (a whole 64-column tile that spans five LES, then a partial one); ktot 1, 2, 7, 8, 9 and 17, and at
    n = 3 the last ktot of every C and the first of the next; every field 0 ... V - 1 elements off the 16-byte grid (V elements are 16 bytes);
    the bytes around every array are looked at by Run.check"""
    dtype = np_of(eng)
    V = 16 // numpy.dtype(dtype).itemsize
    for n in (3, 6):
        for ktot in COLTILE_KTOTS:
            for lead in range(V):
                Run(eng, case((n, 3, 5, ktot), dtype, seed=11 + lead), lead=lead).check("coltile n %d ktot %d lead %d" % (n, ktot, lead))
    for ktot, cols in boundaries(eng.diffuse_cols_per_block):
        for lead in (0, 1) if cols else ():
            Run(eng, case((3, 3, 5, ktot), dtype, seed=12, names=("THL", "QT")), lead=lead).check("coltile C %d ktot %d lead %d" % (cols, ktot, lead))


def check_long_step(eng):
    """dt = 3600: |a| in the hundreds"""
    for ktot in (7, 160):
        c = case((2, 3, 5, ktot), np_of(eng), seed=7, dt=3600.0)
        assert numpy.abs(c["prof"][0]).max() > 50
        Run(eng, c).check("dt 3600 ktot %d" % ktot)


def special_case(dtype, ktot):
    """(clean case, the same with -0.0, NaN, +inf and -inf planted in one column each of THL, columns (l, i, j))"""
    c = case((3, 3, 5, ktot), dtype, seed=8)
    s = dict(c, fields={k: v.copy() for k, v in c["fields"].items()})
    x = s["fields"]["THL"]
    planted = {(0, 0, 1): -0.0, (1, 1, 2): numpy.nan, (1, 2, 4): numpy.inf, (2, 0, 0): -numpy.inf}
    for (l, i, j), v in planted.items():
        x[l, i, j, ktot // 2] = v
    x[0, 2, 2, :] = -0.0
    return c, s, list(planted) + [(0, 2, 2)]


def identity_case(dtype, ktot):
    """a = 0, m = 1, cp = 0, no flux, positive THL and QT with -0.0 at level 0 of a column and at every other level of another:
    every bit is kept.  (A -0.0 keeps its sign where the levels next to it are not negative: 0 * negative is -0.0, and
    -0.0 - -0.0 is +0.0 -- the recurrence's arithmetic, in the oracle and in the kernel alike.)"""
    c = case((3, 3, 5, ktot), dtype, seed=10, names=("THL", "QT"), fluxes=())
    a, m, cp, s0 = c["prof"]
    c["prof"] = (numpy.zeros_like(a), numpy.ones_like(m), numpy.zeros_like(cp), s0)
    c["fields"]["QT"][:, 0, 0, ::2] = -0.0
    c["fields"]["THL"][:, 1, 1, 0] = -0.0
    return c


def check_special(eng):
    """-0.0, NaN and +-inf planted in single columns: they spread through their column as the oracle says, and the bits of every
    other column equal a run without them; the identity coefficients keep every bit, -0.0 included"""
    dtype = np_of(eng)
    for ktot in (7, 64):
        c, s, cols = special_case(dtype, ktot)
        clean = Run(eng, c).check("clean ktot %d" % ktot)
        r = Run(eng, s)
        want = r.check("special ktot %d" % ktot)
        got = r.dev["THL"].cpu().numpy()
        others = numpy.ones(got.shape[:3], dtype=bool)
        for col in cols:
            others[col] = False
        assert_bits("the other columns", got[others], clean["THL"][others])
        assert numpy.isnan(want["THL"][1, 1, 2]).all() and not numpy.isfinite(want["THL"][1, 2, 4]).any()
        r = Run(eng, identity_case(dtype, ktot))
        r.check("identity ktot %d" % ktot)
        for k, v in r.c["fields"].items():
            assert_bits("identity keeps " + k, r.dev[k].cpu().numpy(), v)


def check_refusals(eng):
    """n = 0 is a no-op; two equal fields, a field that is a profile and a flux without s0 are refused by the library and by
    the engine, and no refused call touches anything"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=9)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    t = {k: dev(v) for k, v in c["fields"].items()}
    a, m, cp, s0 = (dev(p) for p in c["prof"])
    fl = {k: dev(v) for k, v in c["flux"].items()}
    assert eng.les_diffuse({k: v[:0] for k, v in t.items()}, a[:0], m[:0], cp[:0], s0=s0[:0], flux={k: v[:0] for k, v in fl.items()}) is None
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    for kw, text in ((dict(alias=((1, "U"),)), b"same field"), (dict(alias=((2, "m"),)), b"also a profile"), (dict(s0=False), b"without s0")):
        rc, got = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        for k in NAMES:
            assert_bits("refused: " + k, got[k], c["fields"][k])
    prof_like = a.view(2, 1, 1, 8)
    for bad in (lambda: eng.les_diffuse({"U": t["U"], "V": t["U"]}, a, m, cp),
                lambda: eng.les_diffuse({"U": prof_like}, a, m, cp),
                lambda: eng.les_diffuse(t, a, m, cp, flux=fl),                                # a flux without s0
                lambda: eng.les_diffuse(t, a, m, cp, s0=s0, flux={"QR": fl["QT"]}),
                lambda: eng.les_diffuse({}, a, m, cp),
                lambda: eng.les_diffuse(dict(t, QR=t["QT"].clone()), a, m, cp),              # five fields
                lambda: eng.les_diffuse(t, a, m[:, :4], cp),
                lambda: eng.les_diffuse(t, a, m, cp, s0=s0[:1], flux=fl),
                lambda: eng.les_diffuse({"U": t["U"][..., ::2]}, a, m, cp),
                lambda: eng.les_diffuse({"U": t["U"].to(torch.float64 if eng.dtype == torch.float32 else torch.float32)}, a, m, cp),
                lambda: eng.les_diffuse({"U": t["U"].cpu()}, a, m, cp)):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    for k in NAMES:
        assert_bits("refused: " + k, t[k].cpu().numpy(), c["fields"][k])


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    c = case((n, 3, 5, 40), np_of(one), seed=n)
    want = oracle(c)
    for tag, eng, up in on_both(one, multi, n):
        t = {k: up(v) for k, v in c["fields"].items()}
        a, m, cp, s0 = (up(p) for p in c["prof"])
        assert eng.les_diffuse(t, a, m, cp, s0=s0, flux={k: up(v) for k, v in c["flux"].items()}) is None
        multi.synchronize()
        for k in NAMES:
            assert_bits("%s %s" % (tag, k), host_of(t[k]), want[k])
    return blocks_of(t["QT"], multi, n)


BODIES = ("parity", "rows", "boundaries", "tiles", "coltile", "fields", "alignment", "long_step", "special", "refusals")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (1, 2, 9, 64, 65, 160)]),
            ("rows", lambda: [check_rows(eng, k) for k in (1, 7, 160)]),
            ("boundaries", lambda: check_boundaries(eng)),
            ("tiles", lambda: [check_tiles(eng, k) for k in (7, 300)]),
            ("coltile", lambda: check_coltile(eng)),
            ("fields", lambda: check_fields(eng)),
            ("alignment", lambda: [check_alignment(eng, *a) for a in ((1, 0, 0), (0, 1, 0), (0, 0, 3), (3, 1, 5))]),
            ("long_step", lambda: check_long_step(eng)),
            ("special", lambda: check_special(eng)),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_diffuse (CPU suite) ----------------------------------------------------------------------
class DiffuseOracleEngine(lmr.MicroOracleEngine):
    """tests/les_micro_ref.MicroOracleEngine with ``les_diffuse`` by the NumPy oracle above: the fields written in place, as
    the HIP engine does"""

    def les_diffuse(self, fields, a, m, cp, s0=None, flux=None, **kw):
        flux = {k: v for k, v in (flux or {}).items() if v is not None}
        if flux and s0 is None:
            raise ValueError("a flux needs s0")
        if len({t.data_ptr() for t in fields.values()}) != len(fields):
            raise ValueError("a field is another field")
        for k, t in fields.items():
            r = les_diffuse(t.numpy(), a.numpy(), m.numpy(), cp.numpy(), s0.numpy() if k in flux else None, flux[k].numpy() if k in flux else None)
            t.copy_(torch.from_numpy(r))


# -- the host twins of models.DeviceLESEnsemble after enable_diffusion() -------------------------------------------------------
class _HostDiffuse:
    """NumPy fields: the executable definition of what evolve_model_batched does after enable_diffusion(), plain, after
    enable_thermo() (THERMO) and with enable_microphysics() on top of either"""

    THERMO = False
    diffuse_par = None

    def enable_diffusion(self, k_max=None, h_mix=None, k_bg=None):
        if not any(k in self.fields3d for k in NAMES):
            raise ValueError("the diffusion (K15) needs one of the fields U, V, THL, QT")
        self.diffuse_par = {"k_max": df.K_MAX if k_max is None else k_max, "h_mix": df.H_MIX if h_mix is None else h_mix,
                            "k_bg": df.K_BG if k_bg is None else k_bg}

    def evolve_model_batched(self, t):
        from sp_coupler_amd import thermo
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        if self.diffuse_par is None:
            return super().evolve_model_batched(t)
        f, p = self.fields3d, self.p
        self._step(dt, NAMES)
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        a, m, cp, s0 = (self._r(x) for x in df.profiles(self.zh_cache, self.zf_cache, p["Rhobf"], dt, **self.diffuse_par))
        for key, slot in (("U", None), ("V", None), ("THL", "wt"), ("QT", "wq")):
            if key in f:
                flux = self._r(numpy.asarray(self.tend[slot], dtype=numpy.float64).reshape(self.n)) if slot in self.tend else None
                f[key] = les_diffuse(f[key], a, m, cp, s0 if flux is not None else None, flux)
        if self.THERMO:
            self._stale = True
            self._ensure_ql()
        elif "QL" in f or ("QT" in f and "Qsat" in f):
            f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
        self._slab_means()
        if self.micro_par is not None and self.THERMO:
            presf = numpy.asarray(p["presf"], dtype=numpy.float64)
            self._micro_step(dt, ltr.les_thermo(f["THL"], f["QT"], self._r(presf), self._r(thermo.exner(presf)), self.n_iter)["temp"])
            self._stale = True
            self._ensure_ql()
        elif self.micro_par is not None:
            self._micro_step(dt, None)
            f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
            p["QL"] = self._w(slab_ref.slab_means(f["QL"]))
        p["QL_ice"] = numpy.minimum(p["QL_ice"], p["QL"])
        if not self.THERMO:
            p["T"] = p["THL"] * (p["presf"] / 1e5) ** (287.04 / 1004.) + 2.53e6 * p["QL"] / 1004.
        if self.micro_par is None:
            p["Rain"] = p["Rain"] + 1e-6 * dt
        self.model_time = float(t)


class HostDiffuseLESEnsemble(_HostDiffuse, lmr.HostMicroLESEnsemble):
    """without enable_thermo(): QL = max(QT - Qsat, 0) of the diffused QT (and again after the microphysics)"""


class HostThermoDiffuseLESEnsemble(_HostDiffuse, lmr.HostThermoMicroLESEnsemble):
    """after enable_thermo(): K12's oracle on the diffused THL and QT (and again after the microphysics)"""

    THERMO = True


WT, WQ = 0.12, 6e-5                                               # K m/s and kg/kg m/s: the surface fluxes of the ensemble runs


def ensemble_run(engine, n, thermo, device, micro=False, diffuse=True, itot=4, jtot=5, nL=20, steps=3):
    """an ensemble with attached U, V, THL, QT (and Qsat, or thermo; QR with the microphysics) through ``steps`` calls of
    evolve_model_batched with non-zero wt and wq and one variability nudge (constantT) before the last; after each of them
    every profile and the fields.  Returns (ens, list of records)"""
    def record(ens, rec):
        rec["TWP"] = numpy.array(host_of(ens.get_water_paths_batched(("TWP",))["TWP"]))
    return ensemble_case(engine, n, models.DeviceLESEnsemble if device else (HostThermoDiffuseLESEnsemble if thermo else HostDiffuseLESEnsemble),
                         thermo=thermo, micro=micro, diffuse=diffuse, record=record, itot=itot, jtot=jtot, nL=nL, steps=steps)


def check_ensemble(one, engines, n, thermo, micro=False, **kw):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``; the fluxes reach level 0: p["THL"]
    there differs from the same run without enable_diffusion()"""
    host = ensemble_run(one, n, thermo, False, micro=micro, **kw)[1]
    plain = ensemble_run(one, n, thermo, False, micro=micro, diffuse=False, **kw)[1]
    assert (host[-1]["p THL"][:, 0] != plain[-1]["p THL"][:, 0]).all() and (host[1]["p THL"][:, 0] != plain[1]["p THL"][:, 0]).all()
    assert not numpy.array_equal(host[1]["field U"], plain[1]["field U"])
    for engine in engines:
        lmr.same_logs(host, ensemble_run(engine, n, thermo, True, micro=micro, **kw)[1])
    return host
