"""What the test modules of the LES kernels (tests/les_*_ref.py, tests/*_edges.py) share, one copy of each idiom: the poisoned
buffers of a ``Run``, the call of a C entry point, the loop over a module's bodies that tools/mutation_control.py runs on a
mutant library, the two uploads of ``check_multi`` and the ensemble run that the twins and models.DeviceLESEnsemble are
compared on.  A module supplies what is particular to its kernel: the oracle, ``case``, ``Run``'s call and comparison, its
bodies, and ``BODIES`` with ``jobs``."""
import contextlib
import ctypes
import os

import numpy
import torch

from sp_coupler_amd import models, spcpl
from tests.test_vnudge import make_les_fields

NP = {torch.float64: numpy.float64, torch.float32: numpy.float32}
DTYPES = (torch.float64, torch.float32)
TAIL_ROWS = 4


def np_of(eng):
    return NP[eng.dtype]


def f32_of(engine_cls):
    """the float32 form of an oracle-backed engine class (tests/fake_engine.OracleEngine has ``dtype`` as a class attribute)"""
    return type(engine_cls.__name__ + "F32", (engine_cls,), {"dtype": torch.float32, "__doc__": engine_cls.__doc__})


def twin_kw(cls, engine):
    """the arguments of ``cls.for_gcm`` that give a host twin the dtype of ``engine``; none for the device ensemble, which takes it
    from its engine"""
    return {} if cls is models.DeviceLESEnsemble else {"dtype": np_of(engine)}


def host_of(t):
    return t if isinstance(t, numpy.ndarray) else models.DeviceLESEnsemble._host(t)


# -- poisoned buffers ------------------------------------------------------------------------------------------------------
def with_tail(eng, a, poison, lead=0, tail_elems=None):
    """``a`` on the device as a view of a larger buffer: ``lead`` elements of poison in front, then the array, then a poisoned
    tail of at least TAIL_ROWS rows (at least one LES).  Returns (view, buffer)."""
    a = numpy.ascontiguousarray(a)
    row = int(numpy.prod(a.shape[1:])) if a.ndim > 1 else 1
    tail = tail_elems if tail_elems is not None else max(row, TAIL_ROWS * int(a.shape[-1]))
    buf = torch.full((lead + a.size + tail,), poison, dtype=torch.from_numpy(a).dtype, device=eng.device)
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a).to(eng.device))
    return view, buf


class Poisoned:
    """the device arrays of one launch, each the leading part of a poisoned buffer (with_tail); ``check_around`` looks at the
    bytes around every array and between the rows of the pitched ones, in the order they were put"""

    def __init__(self, eng, tail_elems=None):
        self.eng, self.tail_elems = eng, tail_elems
        self.bufs, self.width = {}, {}

    def put(self, tag, a, poison, lead=0):
        view, buf = with_tail(self.eng, a, poison, lead=lead, tail_elems=self.tail_elems)
        self.bufs[tag] = (view, buf, lead, poison)
        return view

    def rows(self, tag, a, poison, lead=0, pad=0):
        """``a`` [n x width] with ``pad`` elements of poison behind every row: the view [:, :width] of the pitched array"""
        n, width = a.shape
        wide = numpy.full((n, width + pad), poison, dtype=a.dtype)
        wide[:, :width] = a
        self.width[tag] = width
        return self.put(tag, wide, poison, lead)[:, :width]

    def check_around(self, what):
        for tag, (view, buf, lead, poison) in self.bufs.items():
            clean = lambda x: bool((torch.isnan(x) if poison != poison else x == poison).all())       # noqa: E731
            assert clean(torch.cat([buf[:lead], buf[lead + view.numel():]])), (what, tag, "written around the array")
            if tag in self.width:
                assert clean(view[:, self.width[tag]:]), (what, tag, "written between the rows")

    @staticmethod
    def read_only(t, a):
        """the device tensor ``t`` holds the bytes of the host array ``a``"""
        return numpy.array_equal(numpy.ascontiguousarray(t.cpu().numpy()).view(numpy.uint8), numpy.ascontiguousarray(a).view(numpy.uint8))


# -- the C entry points ------------------------------------------------------------------------------------------------------
def fill_args(a, tensors, members=None, alias=None, extents=None, null=()):
    """the pointer members of the argument struct ``a`` from ``tensors`` (``members``: default every key); then ``alias``:
    (member, key) pairs that replace a pointer member by that of tensor ``key``; then ``extents``: overrides of the scalar
    members; then ``null``: members set to NULL"""
    for k in (tensors if members is None else members):
        setattr(a, k, tensors[k].data_ptr())
    for member, key in (alias or ()):
        setattr(a, member, tensors[key].data_ptr())
    for key, val in (extents or {}).items():
        setattr(a, key, val)
    for key in null:
        setattr(a, key, None)


def abi_call(eng, stem, a):
    """``stem``_f32 or ``stem``_f64 of the engine's library, by its dtype, on its device and the current stream; synchronised.
    Returns rc"""
    fn = getattr(eng.lib, "%s_%s" % (stem, "f32" if eng.dtype == torch.float32 else "f64"))
    with torch.cuda.device(eng.device):
        rc = fn(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
    torch.cuda.synchronize(eng.device)
    return rc


@contextlib.contextmanager
def counted_cus(n):
    """the library counts ``n`` compute units for the duration (SPC_CUS, read at every launch): with 1 a launch of a few rows
    gets what thousands get on a whole card -- K14's kernels for MANY waves (tests/les_micro_ref.py), K7's slabs of several rows
    (tests/sputils_slabs.py)"""
    old = os.environ.get("SPC_CUS")
    os.environ["SPC_CUS"] = str(n)
    try:
        yield
    finally:
        if old is None:
            del os.environ["SPC_CUS"]
        else:
            os.environ["SPC_CUS"] = old


# -- bodies ------------------------------------------------------------------------------------------------------------------
def run_bodies(bodies, jobs):
    """the names of the ``jobs`` [(name, callable)] that failed (AssertionError; anything else propagates), in the order they
    ran; the jobs are the module's ``bodies``, all of them, in that order"""
    assert [name for name, _ in jobs] == list(bodies), ([name for name, _ in jobs], list(bodies))
    failed = []
    for name, job in jobs:
        try:
            job()
        except AssertionError:
            failed.append(name)
    return failed


def chain_cases(U, dtype, nijs=None):
    """(shape, lead) of the cases that hold the walk of a slab-chain lane (spc_chain.hpp; K10, K11, K12, K14, K20) in batches of
    U rows together: n_les = 2, planes 1 x nij for every nij = 1 ... 2 U + 1 (``nijs``: others) -- the tail alone, one whole
    batch with no successor, a batch that has a successor and one that has none, a batch with a tail behind it --, each at ktot 8
    (16-byte accesses in both dtypes: four and two lanes per LES), at ktot 7 (one element per lane) and at ktot 8 with every array
    ``lead`` = 1 element off the 16-byte grid (one element per lane at an even ktot); then n_les = 5, ktot = 7 V with a batch and a
    tail, on and off the grid: 35 and 35 V lanes, so a wave holds lanes of several LES and lanes past the last chain"""
    V = 16 // numpy.dtype(dtype).itemsize
    for nij in (range(1, 2 * U + 2) if nijs is None else nijs):
        for ktot, lead in ((8, 0), (7, 0), (8, 1)):
            yield (2, 1, nij, ktot), lead
    for lead in (0, 1):
        yield (5, 1, U + 1, 7 * V), lead


def cols_table(cols_of, top=3000):
    """(dict C -> the smallest ktot with that many columns per workgroup, the ktot at which the count changes, the first
    unsupported ktot) of ``cols_of(ktot)``"""
    first, changes, last = {}, [], None
    for ktot in range(1, top):
        C = cols_of(ktot)
        if C != last and last is not None:
            changes.append(ktot)
        last = C
        if C == 0:
            return first, changes[:-1], ktot
        first.setdefault(C, ktot)
    raise AssertionError("no unsupported ktot below %d" % top)


def on_both(one, multi, n):
    """(tag, engine, upload of a host array) of "one" engine and of the "multi" engine with Sharded blocks of ``n`` rows"""
    yield "one", one, lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(one.device)
    yield "multi", multi, lambda a: multi.to_devices(numpy.ascontiguousarray(a), rows=n)


def blocks_of(sharded, multi, n):
    """the rows of every part of a Sharded: one block per engine, ``n`` rows in all"""
    blocks = [int(p.shape[0]) for p in sharded.parts]
    assert sum(blocks) == n and len(blocks) == len(multi.engines)
    return blocks


# -- the tables of tools/mutation_control.py, without a GPU ------------------------------------------------------------------
def check_mutant_table(table, sources, module, count=8):
    """``table`` against the tree: numbered 1 ... ``count``; every edit in one of the files ``sources`` and applied exactly as
    often as it states (mutation_control.patched raises otherwise); every patched file changed; every guard a body of ``module``"""
    from tools import mutation_control as mc
    assert sorted(table) == list(range(1, count + 1))
    for n, (what, guard, edits) in table.items():
        assert what and edits and callable(guard) and all(e[0] in sources for e in edits), n
        mod, name = guard.__name__.split(".", 1)
        assert "tests." + mod == module.__name__ and name in module.BODIES and hasattr(module, "check_" + name), (n, guard.__name__)
        for fname, text in mc.patched(n, table=table).items():
            with open(os.path.join(mc.CSRC, fname)) as f:
                assert text != f.read(), (n, fname)


def check_library_names(table, name):
    """no two mutants of the tables of the registry, the *_EQUIVALENT ones included, share a library; mutant 2 of ``table``
    builds ``name``"""
    from tools import mutation_control as mc
    tables = [t.table for t in mc.TABLES] + [t.equivalent for t in mc.TABLES if t.equivalent]
    libs = [mc.lib_of(n, t) for t in tables for n in t]
    assert len(set(libs)) == len(libs) and mc.lib_of(2, table).endswith(name)


def check_jobs_are_bodies(module):
    """check_everything runs each name of BODIES, in that order (a body left out would guard nothing)"""
    assert [name for name, _ in module.jobs(None)] == list(module.BODIES)


# -- the ensemble run ----------------------------------------------------------------------------------------------------------
WT, WQ = 0.12, 6e-5                                               # K m/s and kg/kg m/s: the surface fluxes of the ensemble runs


def ensemble_case(engine, n, cls, thermo=False, micro=False, diffuse=False, edit=None, advection=None, radiation=None, enable=None,
                  forcings=None, record=None, before=None, itot=4, jtot=5, nL=20, steps=3):
    """an ensemble of class ``cls`` with attached U, V, THL, QT (and Qsat, or thermo; QR with the microphysics) through ``steps``
    calls of evolve_model_batched with non-zero wt and wq and one variability nudge (constantT) before the last; after each of
    them every profile and the fields; a twin takes the dtype of ``engine`` (np_of), the engine its nudge runs on.  The hooks of a module: ``edit(fields)`` on the host fields; ``advection`` and
    ``radiation``: the arguments of enable_advection and enable_radiation (None: never called); ``enable(ens)`` behind them;
    ``forcings(rng, stack)``: more arguments of set_forcings_batched; ``record(ens, rec)``: more entries of a record;
    ``before(ens)``: what holds before the first step.  Returns (ens, list of records)"""
    spcpl.set_engine(engine)
    fs = [make_les_fields(itot, jtot, nL, seed=60 + (i % 7)) for i in range(n)]
    stack = lambda k: numpy.stack([f[k] for f in fs])                                      # noqa: E731
    gcm = models.BatchedSyntheticGCM(n + 4, 19, 21)
    ens = cls.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=21, itot=itot, jtot=jtot, **twin_kw(cls, engine))
    rng = numpy.random.default_rng(n + 100)
    fields = {"Qsat": stack("qsat"), "QT": stack("qt"), "THL": stack("thl"), "U": 5.0 + rng.standard_normal((n, itot, jtot, nL)),
              "V": -2.0 + rng.standard_normal((n, itot, jtot, nL))}
    if thermo:
        del fields["Qsat"]
        fields["THL"] = fields["THL"] - 25.0                      # cells between t_dn and t_up: ice and water
        fields["QT"] = fields["QT"] * 0.35
        fields["QT"][:, 2, 1, :] *= 2.0                           # one column K12 finds cloudy whatever the profile
    if edit:
        edit(fields)
    if micro:
        fields["QR"] = numpy.random.default_rng(n).random((n, itot, jtot, nL)) * 1e-5
    ens.attach_fields({k: v.copy() for k, v in fields.items()})
    ens.p["presf"] = stack("presf")
    ens.ql_ref = stack("ql_ref")
    ens.model_time = 900.0
    if thermo:
        ens.enable_thermo()
    if diffuse:
        ens.enable_diffusion()
    if micro:
        ens.enable_microphysics(qc0=1e-4, v_fall=0.05)           # (layers of the synthetic grid in 900 s: part of the rain stays)
    if advection is not None:
        ens.enable_advection(**advection)
    if radiation is not None:
        ens.enable_radiation(**radiation)
    if enable:
        enable(ens)
    rng = numpy.random.default_rng(5)
    forced = dict(THL=rng.normal(0, 2e-4, (n, nL)), QT=rng.normal(0, 2e-7, (n, nL)), U=rng.normal(0, 1e-4, (n, nL)),
                  WT_surf=WT * (0.5 + rng.random(n)), WQ_surf=WQ * (0.5 + rng.random(n)))
    if forcings:
        forced.update(forcings(rng, stack))
    ens.set_forcings_batched(**forced)
    log = []

    def rec():
        prof = {k: numpy.empty((n, nL)) for k in ("U", "V", "THL", "QT", "QL")}
        ens.get_profiles_batched(tuple(prof), prof)
        r = {"p " + k: numpy.array(v) for k, v in ens.p.items()}
        r.update({"got " + k: v for k, v in prof.items()})
        r.update({"field " + k: numpy.array(host_of(ens.get_fields_batched(k))) for k in ("U", "V", "QT", "THL", "QL") + (("QR",) if micro else ())})
        if record:
            record(ens, r)
        log.append(r)
    if before:
        before(ens)
    rec()
    for step in range(steps):
        if step == steps - 1:
            numpy.random.seed(11)
            spcpl.variability_nudge_ensemble(ens, 900.0, True, write=False)
            rec()
        ens.evolve_model_batched(1800.0 + 900.0 * step)
        rec()
    return ens, log
