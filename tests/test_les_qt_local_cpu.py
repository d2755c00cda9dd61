"""K19 without a GPU: the ABI of spc_les_qt_local_*, the refusals the library makes on the host, the NumPy oracle of
tests/les_qt_local_ref.py against a second statement of the rule and against what the rule promises (the classes of levels, the
slab mean of qt, the direction the cloud water moves in), qt_forcing.increments, and models.DeviceLESEnsemble's
enable_qt_forcing() on an oracle-backed engine against its host twins, alone, beside every other mode and under the coupler."""
import ctypes
import math
import os
import subprocess

import numpy
import pytest
import torch

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import qt_forcing as qf
from tests import les_qt_local_ref as qlr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {numpy.float64: 2.0 ** -52, numpy.float32: 2.0 ** -23}
SHAPES = [(3,) + p + (k,) for p in qlr.PLANES for k in (1, 2, 7, 20, 65)]
NPS = [numpy.float64, numpy.float32]


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    return _abi.load_library()


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


# -- the ABI -------------------------------------------------------------------------------------------------------------------
def test_struct_layout_of_the_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror; the ABI version has not moved"""
    cls, cname = _abi.LesQtLocalArgs, "spc_les_qt_local_args"
    fields = ["n_les", "itot", "jtot", "ktot", "split", "qt", "ql", "a", "qtm", "pitch_prof", "count", "pitch_count"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_ABI_VERSION);']
    want = [ctypes.sizeof(cls), 4]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


def _args(n=4, itot=8, jtot=8, ktot=20, split=0, pitch_prof=None, pitch_count=None, **ptrs):
    a = _abi.LesQtLocalArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.split = n, itot, jtot, ktot, split
    a.pitch_prof = ktot if pitch_prof is None else pitch_prof
    a.pitch_count = ktot if pitch_count is None else pitch_count
    for i, k in enumerate(qlr.PTRS):                              # distinct, 16-byte aligned, never dereferenced
        setattr(a, k, ptrs.get(k, 4096 * (i + 1)))
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_qt_local_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    for k in qlr.PTRS:
        assert call(**{k: None}) == (E, b"required pointer %s is NULL" % k.encode())
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    rc, text = call(itot=4096, jtot=4097)
    assert rc == E and b"2^24" in text
    rc, text = call(itot=1 << 20, jtot=1 << 20)
    assert rc == E and b"2^24" in text
    rc, text = call(pitch_prof=19)
    assert rc == E and b"pitch_prof" in text
    rc, text = call(pitch_count=19)
    assert rc == E and b"pitch_count" in text
    rc, text = call(split=-1)
    assert rc == E and b"split" in text
    rc, text = call(ql=4096)
    assert rc == E and b"same array" in text
    rc, text = call(qt=4100 if sfx == "f64" else 4098)
    assert rc == E and b"not aligned" in text
    rc, text = call(count=4096 * 5 + 2)
    assert rc == E and b"not aligned" in text
    rc, text = call(n=1 << 40, ktot=3)
    assert rc == U and b"too many workgroups" in text
    assert fn(ctypes.byref(_args(n=0, **{k: None for k in qlr.PTRS})), None) == 0       # an empty ensemble is a no-op
    assert lib.spc_abi_version() == 4


def test_the_split_the_library_chooses(lib):
    """1 where the fused launch fills the card or a plane is small, else parts of at least 64 rows up to ~1 024 workgroups; the
    element size changes nothing; bad arguments give 0"""
    f = lib.spc_les_qt_local_split
    for esize in (4, 8):
        assert f(256, 8, 8, 160, esize) == 1 and f(1024, 64, 64, 160, esize) == 1
        assert f(16, 64, 64, 160, esize) == 22 and f(1, 64, 64, 160, esize) == 64 and f(1, 128, 128, 160, esize) == 256
        assert f(3, 8, 8, 160, esize) == 1 and f(3, 17, 5, 7, esize) == 1 and f(2, 16, 16, 70, esize) == 4
        assert f(0, 8, 8, 160, esize) == 0 and f(4, 0, 8, 160, esize) == 0 and f(4, 8, 8, 0, esize) == 0 and f(4, 4097, 4097, 9, esize) == 0
    assert f(4, 8, 8, 160, 2) == 0


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    assert callable(Engine.les_qt_local) and callable(MultiDeviceEngine.les_qt_local) and callable(Engine.qt_local_split)
    assert not hasattr(qlr.lrr.RadiateOracleEngine, "les_qt_local")


# -- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_equals_the_vectorised_statement(shape, dtype):
    for seed in (0, 3):
        c = qlr.case(shape, dtype, seed=seed)
        new, count = qlr.oracle(c)
        new2, count2 = qlr.les_qt_local_vectorised(c["qt"], c["ql"], c["a"], c["qtm"])
        assert new.dtype == c["qt"].dtype and count.dtype == numpy.int32
        assert_bits("qt", new, new2)
        assert numpy.array_equal(count, count2)
    c, _ = qlr.skipped_case(dtype)
    assert_bits("special values", qlr.oracle(c)[0], qlr.les_qt_local_vectorised(c["qt"], c["ql"], c["a"], c["qtm"])[0])


@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("plane", [(2, 3), (8, 8), (17, 5)])
def test_every_class_of_level_is_in_a_case(plane, dtype):
    """what the builder plants is there (it asserts so itself); the random levels add both mixed classes many times over"""
    for ktot in (7, 20, 160):
        c = qlr.case((3,) + plane + (ktot,), dtype)
        have = qlr.classes(c["qt"], c["ql"], c["a"], c["qtm"])
        assert set(qlr.CLASSES) <= set(have.ravel())
        assert numpy.signbit(c["a"][have == "negzero"]).all() and not numpy.signbit(c["a"][have == "zero"]).any()
        if ktot >= 20:
            assert (have == "pos_mixed").sum() > 3 and (have == "neg_mixed").sum() > 3


def test_a_plane_of_one_cell_never_changes():
    for dtype in NPS:
        c = qlr.case((3, 1, 1, 20), dtype)
        new, count = qlr.oracle(c)
        assert numpy.array_equal(new.view(numpy.uint8), c["qt"].view(numpy.uint8)) and set(count.ravel()) <= {0, 1} and count.any()


@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("plane", [(2, 3), (8, 8), (17, 5)])
def test_the_slab_mean_of_qt_is_conserved(plane, dtype):
    """every cell is rounded once when its share is added (half an ulp of qt at most) and the two shares carry the rounding of
    their quotients (an ulp of the share): the mean of a plane moves by less than 2 ulp of its largest cell"""
    c = qlr.case((3,) + plane + (20,), dtype)
    new, count = qlr.oracle(c)
    N = plane[0] * plane[1]
    worst = 0.0
    for l in range(3):
        for k in range(20):
            old_sum = math.fsum(float(x) for x in c["qt"][l, :, :, k].ravel())
            new_sum = math.fsum(float(x) for x in new[l, :, :, k].ravel())
            drift = abs(new_sum - old_sum) / N
            bound = 2.0 * EPS[dtype] * float(numpy.abs(c["qt"][l, :, :, k]).max())
            assert drift <= bound, (l, k, drift, bound)
            worst = max(worst, drift)
    mixed = (count > 0) & (count < N)
    assert mixed.sum() > 6 and (worst > 0 or dtype is numpy.float64)


@pytest.mark.parametrize("plane", [(2, 3), (8, 8), (17, 5)])
def test_the_cloud_water_moves_with_the_sign_of_a(plane):
    """the rule moves moisture from the drier cells to the moister ones (a > 0) or from the cloudy ones to the rest (a < 0).
    With shares that are small against the spread of qt, as in the case (|a| of 1e-5 ... 3e-5, a spread of 2e-4), no cell that
    receives overtakes one that gives, and max(qt - qsat, 0) is convex: on every mixed level of the case the slab mean of the
    cloud water does not move against a (beyond the rounding of a sum of N cells), and on the planted mixed levels and on every
    mixed level with a < 0 it moves with it.  (Large shares can break this: DESIGN.md 7.3.)"""
    c = qlr.case((3,) + plane + (20,), numpy.float64)
    new, count = qlr.oracle(c)
    N = plane[0] * plane[1]
    qs = c["qsat"][:, None, None, :]
    before = numpy.maximum(c["qt"] - qs, 0.0).mean(axis=(1, 2))
    after = numpy.maximum(new - qs, 0.0).mean(axis=(1, 2))
    assert_bits("ql is the cloud water of qt", numpy.maximum(c["qt"] - qs, 0.0), c["ql"])
    moved = (after - before) * numpy.sign(numpy.nan_to_num(c["a"]))
    mixed = (count > 0) & (count < N)
    assert (moved[mixed] >= -N * 2.0 ** -52 * 8e-3).all() and not moved[~mixed].any()
    assert (moved[mixed & (c["a"] < 0)] > 0).all()
    inv = {v: k for k, v in c["planted"].items()}
    assert moved[inv["pos_mixed"]] > 0 and moved[inv["neg_mixed"]] > 0


def test_increments():
    rng = numpy.random.default_rng(0)
    f_ql, ql_ref, ql_mean = rng.normal(0, 1e-8, (3, 5)), rng.random((3, 5)) * 1e-4, rng.random((3, 5)) * 1e-4
    a = qf.increments("local", f_ql, ql_ref, ql_mean, 60.0)
    assert a.dtype == numpy.float64 and numpy.array_equal(a, f_ql * 60.0)
    assert numpy.array_equal(qf.increments("local", f_ql.astype(numpy.float32), None, None, 60), f_ql.astype(numpy.float32).astype(numpy.float64) * 60.0)
    s = qf.increments("strong", f_ql, ql_ref, ql_mean, 60.0)
    assert s.dtype == numpy.float64 and numpy.array_equal(s, ql_ref - ql_mean)
    assert numpy.array_equal(qf.increments("strong", None, ql_ref, ql_mean, 1e9), s)            # no dt in it: the whole gap
    assert qf.KINDS == ("local", "strong")
    for bad in ("sp", "variance", None, "LOCAL"):
        with pytest.raises(ValueError, match="kind"):
            qf.increments(bad, f_ql, ql_ref, ql_mean, 60.0)


# -- the ensemble ------------------------------------------------------------------------------------------------------------
KERNELS = ("les_qt_local", "les_radiate", "les_thermo", "les_microphysics", "les_diffuse", "les_advect", "les_vadvect", "les_advance")


def _counted(engine, calls):
    for name in KERNELS:
        inner = getattr(engine, name)
        setattr(engine, name, lambda *a, _n=name, _f=inner, **kw: (calls.append(_n), _f(*a, **kw))[1])
    return engine


@pytest.mark.parametrize("kind", qf.KINDS)
@pytest.mark.parametrize("variant", list(qlr.VARIANTS))
def test_ensemble_on_one_engine_equals_the_host_twin(variant, kind):
    """every profile, field and the counts bit-equal to the twin after each of three steps and the nudge; ONE K19 launch per
    step, directly after the step and before K16 / K17 / K15 / K18 / K14"""
    qlr.check_ensemble(qlr.QtLocalOracleEngine(), [qlr.QtLocalOracleEngine()], 4, variant, kind)
    calls = []
    qlr.ensemble_run(_counted(qlr.QtLocalOracleEngine(), calls), 4, True, kind=kind, **qlr.VARIANTS[variant])
    assert calls.count("les_qt_local") == 3
    if variant == "plain":
        assert calls == ["les_qt_local"] * 3
    else:
        at = [i for i, k in enumerate(calls) if k == "les_qt_local"] + [len(calls)]
        for lo, hi in zip(at[:-1], at[1:]):
            step = calls[lo:hi]
            physics = [k for k in step if k not in ("les_qt_local", "les_thermo")]
            assert physics[0] == "les_advect" and physics.index("les_diffuse") < physics.index("les_radiate") < physics.index("les_microphysics")
            assert calls[lo - 1] == "les_thermo"                  # (K12 made the QL that K19 reads)


def test_step_order_of_the_twin():
    """the twin applies the rule to the STEPPED QT with the QL and the means of the stepped fields, before anything else acts"""
    ens, log = qlr.ensemble_run(qlr.QtLocalOracleEngine(), 3, False, kind="local", steps=1)
    before, after = log[1], log[2]                               # (log[1]: after the nudge that precedes the last step)
    dt = 900.0
    qt = before["field QT"] + (ens.tend["QT"] * dt)[:, None, None, :]
    ql = numpy.maximum(qt - numpy.stack([qlr.make_les_fields(4, 5, 20, seed=60 + i)["qsat"] for i in range(3)]), 0.0)
    a = qf.increments("local", ens.tend["QL"], None, None, dt)
    new, count = qlr.les_qt_local(qt, ql, numpy.ascontiguousarray(a), slab_ref.slab_means(qt))
    assert_bits("QT", after["field QT"], new)
    assert numpy.array_equal(after["counts"], count)
    assert_bits("p QT", after["p QT"], slab_ref.slab_means(new))


@pytest.mark.parametrize("kind", qf.KINDS)
def test_ensemble_as_row_blocks_with_an_empty_device(kind):
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(qlr.QtLocalOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    qlr.check_ensemble(qlr.QtLocalOracleEngine(), [multi], 2, "all", kind)
    assert calls.count("les_qt_local") == 6                        # blocks 1 + 1 + 0: two devices, three steps


@pytest.mark.parametrize("variant", list(qlr.VARIANTS))
def test_without_enable_qt_forcing_nothing_changes(variant):
    """enable_qt_forcing never called: three steps bit-equal to the ensemble of the K18 tests' engine, which has no
    les_qt_local at all, on the same inputs (the cloud-water forcing handed over all the same), and no K19 launch"""
    calls = []
    new = qlr.ensemble_run(_counted(qlr.QtLocalOracleEngine(), calls), 4, True, kind=None, **qlr.VARIANTS[variant])[1]
    old = qlr.ensemble_run(qlr.lrr.RadiateOracleEngine(), 4, True, kind=None, **qlr.VARIANTS[variant])[1]
    qlr.lmr.same_logs(old, new)
    assert "les_qt_local" not in calls


def _small(eng, n=2, nL=6):
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(n, nL=nL)
    return models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)


def _fields(rng, names=("THL", "QT", "Qsat")):
    base = {"THL": 290.0, "QT": 9e-3, "Qsat": 8.7e-3}
    return {k: base[k] * (1.0 + 0.05 * rng.random((2, 2, 3, 6))) for k in names}


def test_enable_qt_forcing_needs_a_kind_qt_and_cloud_water():
    eng = qlr.QtLocalOracleEngine()
    rng = numpy.random.default_rng(1)
    ens = _small(eng)
    ens.attach_fields(_fields(rng, ("THL", "Qsat")))
    with pytest.raises(ValueError, match="QT field"):
        ens.enable_qt_forcing("local")
    ens = _small(eng)
    ens.attach_fields(_fields(rng, ("THL", "QT")))
    with pytest.raises(ValueError, match="Qsat"):
        ens.enable_qt_forcing("strong")
    ens.enable_thermo()
    ens.enable_qt_forcing("strong")
    ens = _small(eng)
    ens.attach_fields(_fields(rng))
    for bad in ("sp", "variance", None):
        with pytest.raises(ValueError, match="one of"):
            ens.enable_qt_forcing(bad)
    assert ens.qt_forcing_kind is None and ens.get_qt_forcing_counts_batched() is None
    old = models.DeviceLESEnsemble(ens.grid_indices, ens.zf_cache, ens.zh_cache, ens.p, itot=2, jtot=3, engine=qlr.lrr.RadiateOracleEngine())
    old.attach_fields(_fields(rng))
    with pytest.raises(ValueError, match="les_qt_local"):
        old.enable_qt_forcing("local")
    # no launch before the forcing the kind reads was handed over; the counts tensor is written again, not made again
    ens.enable_qt_forcing("local")
    t = float(ens.model_time)
    ens.evolve_model_batched(t + 100.0)
    assert ens.get_qt_forcing_counts_batched() is None
    ens.set_forcings_batched(QL=numpy.full((2, 6), 1e-8))
    ens.evolve_model_batched(t + 200.0)
    counts = ens.get_qt_forcing_counts_batched()
    assert tuple(counts.shape) == (2, 6) and counts.dtype == torch.int32
    ens.evolve_model_batched(t + 300.0)
    assert ens.get_qt_forcing_counts_batched() is counts
    ens.enable_qt_forcing("local")
    assert ens.get_qt_forcing_counts_batched() is counts         # the same kind again changes nothing
    ens.enable_qt_forcing("strong")
    assert ens.qt_forcing_kind == "strong" and ens.get_qt_forcing_counts_batched() is None


# -- the coupler ---------------------------------------------------------------------------------------------------------------
def test_the_coupler_enables_the_mode_of_an_ensemble_that_offers_it():
    """spcpl._ensemble_forcings with qt_forcing 'local' / 'strong': the device ensemble and its twin are switched to that kind
    and agree bit for bit; QT moves inside the mixed planes only, its slab mean follows the 'sp' run, the cloud water moves with
    the forcing"""
    dev = qlr.check_coupler(qlr.QtLocalOracleEngine(), models.DeviceLESEnsemble)
    host = qlr.check_coupler(qlr.QtLocalOracleEngine(), qlr.HostQtLocalLESEnsemble)
    for kind in ("sp",) + qf.KINDS:
        for a, b in zip(host[kind], dev[kind]):
            assert set(a) == set(b)
            for k in a:
                assert_bits("%s %s" % (kind, k), b[k], a[k])


def test_an_ensemble_without_the_method_behaves_as_before():
    """'local' and 'strong' on an ensemble that does not offer enable_qt_forcing: what 'sp' does, bit for bit"""
    def run(qt_forcing):
        spcpl.set_engine(qlr.QtLocalOracleEngine())
        gcm = models.BatchedSyntheticGCM(11, 19, 3)
        ens = slab_ref.HostFieldLESEnsemble.for_gcm(gcm, numpy.arange(1, 9, 2), nL=24, seed=4, itot=4, jtot=4)
        rng = numpy.random.default_rng(8)
        ens.attach_fields({"Qsat": ens.p["QT"][:, None, None, :] * (1.0 + 2e-3 * rng.normal(size=(4, 4, 4, 24)))})
        cpl = qlr.driver.Coupler(gcm, ens, cplsurf=True, qt_forcing=qt_forcing)
        numpy.random.seed(42)
        cpl.init_les_state()
        cpl.run_spinup(900.0, 1)
        cpl.step()
        return ens
    assert not hasattr(slab_ref.HostFieldLESEnsemble, "enable_qt_forcing")
    sp = run("sp")
    for kind in qf.KINDS:
        other = run(kind)
        for k in ("QT", "QL", "THL"):
            assert_bits(kind + " " + k, other.fields3d[k], sp.fields3d[k])
        for k in sp.p:
            assert_bits(kind + " p " + k, other.p[k], sp.p[k])


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", qf.KINDS)
@pytest.mark.parametrize("variant", list(qlr.VARIANTS))
def test_float32_ensemble_on_one_engine_equals_the_host_twin(variant, kind):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    qlr.check_ensemble(f32_of(qlr.QtLocalOracleEngine)(), [f32_of(qlr.QtLocalOracleEngine)()], 4, variant, kind)
    calls = []
    qlr.ensemble_run(_counted(f32_of(qlr.QtLocalOracleEngine)(), calls), 4, True, kind=kind, **qlr.VARIANTS[variant])
    assert calls.count("les_qt_local") == 3
    if variant == "plain":
        assert calls == ["les_qt_local"] * 3
    else:
        at = [i for i, k in enumerate(calls) if k == "les_qt_local"] + [len(calls)]
        for lo, hi in zip(at[:-1], at[1:]):
            step = calls[lo:hi]
            physics = [k for k in step if k not in ("les_qt_local", "les_thermo")]
            assert physics[0] == "les_advect" and physics.index("les_diffuse") < physics.index("les_radiate") < physics.index("les_microphysics")
            assert calls[lo - 1] == "les_thermo"                  # (K12 made the QL that K19 reads)


@pytest.mark.parametrize("kind", qf.KINDS)
def test_float32_ensemble_as_row_blocks_with_an_empty_device(kind):
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(qlr.QtLocalOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    qlr.check_ensemble(f32_of(qlr.QtLocalOracleEngine)(), [multi], 2, "all", kind)
    assert calls.count("les_qt_local") == 6                        # blocks 1 + 1 + 0: two devices, three steps
