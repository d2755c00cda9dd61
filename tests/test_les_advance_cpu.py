"""K11 without a GPU: the struct layout of spc_les_advance_args, the host-side refusals of spc_les_advance_*, the NumPy oracle
of tests/les_advance_ref.py against answers worked out by hand, and models.DeviceLESEnsemble's fused step on an oracle-backed
engine against its host twin."""
import ctypes
import os
import subprocess

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from tests import device_fields_multi as dfm
from tests import les_advance_ref as lar
from tests import slab_ref
from tests.fake_engine import OracleEngine
from tools import mutation_control as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_struct_layout_of_the_advance_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.LesAdvanceArgs, "spc_les_advance_args"
    fields = ["n_les", "itot", "jtot", "ktot", "n_fields", "fields", "tend", "mean", "pitch_tend", "pitch_mean", "dt", "sat_field",
              "reserved", "qsat", "ql", "ql_mean"]
    assert [f[0] for f in cls._fields_] == fields and _abi.ADVANCE_MAX_FIELDS == 8
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_ADVANCE_MAX_FIELDS);', 'printf("%d\\n", SPC_ABI_VERSION);']
    want = [ctypes.sizeof(cls), 8, 4]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


def _args(n=4, itot=8, jtot=8, ktot=20, nf=3, pitch_tend=20, pitch_mean=20, sat=2, ptr=64, qsat=4096, ql=8192, ql_mean=64, dt=900.0):
    a = _abi.LesAdvanceArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields = n, itot, jtot, ktot, nf
    a.pitch_tend, a.pitch_mean, a.dt, a.sat_field = pitch_tend, pitch_mean, dt, sat
    for f in range(max(0, min(nf, _abi.ADVANCE_MAX_FIELDS))):
        a.fields[f] = None if ptr is None else ptr * (f + 1)                 # distinct, 16-byte aligned, never dereferenced
        a.tend[f], a.mean[f] = ptr, ptr
    a.qsat, a.ql, a.ql_mean = qsat, ql, ql_mean
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_advance_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_advance_" + sfx)
    assert lib.spc_abi_version() == 4

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    assert call(ptr=None) == (E, b"required pointer fields[f] is NULL")
    for nf in (0, -1, 9):
        rc, text = call(nf=nf, sat=-1)
        assert rc == E and b"field count" in text and b"1 ... 8" in text
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    rc, text = call(itot=65536, jtot=32768)
    assert rc == U and b"2^31 - 1 points per plane" in text
    for bad in (dict(pitch_tend=19), dict(pitch_mean=19)):
        rc, text = call(**bad)
        assert rc == E and b"pitch" in text and b"smaller than ktot" in text
    for s in (-2, 3, 8):
        rc, text = call(sat=s)
        assert rc == E and b"sat_field" in text and b"-1 ... 2" in text
    assert call(qsat=None) == (E, b"required pointer qsat is NULL")
    assert call(qsat=None, sat=-1, n=0)[0] == 0                              # qsat is not looked at without sat_field
    for alias in (dict(ql=64), dict(ql=128), dict(ql=4096)):                 # fields[0], fields[1], qsat
        rc, text = call(**alias)
        assert rc == E and b"ql is also a field or qsat" in text
    rc, text = call(qsat=192)
    assert rc == E and b"qsat is also a field" in text
    rc, text = call(n=1 << 40, ktot=3, pitch_tend=3, pitch_mean=3)
    assert rc == U and b"too many workgroups" in text
    rc, text = call(ktot=1, pitch_tend=1, pitch_mean=1)
    assert rc == U and b"ktot == 1" in text
    assert call(n=0, ptr=None, qsat=None) == (0, lib.spc_last_error())      # an empty ensemble is a no-op
    assert call(n=0)[0] == 0


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_answers_worked_out_by_hand(dtype):
    T = dtype
    x = numpy.array([[[[1.0, -0.0, 3.0]], [[2.0, -0.0, 5.0]]]], dtype=T)                      # n=1, itot=2, jtot=1, ktot=3
    tend = numpy.array([[0.5, -0.0, 0.1]], dtype=T)
    new, q, means = lar.les_advance({"QT": x}, {"QT": tend}, 2.0, qsat=numpy.array([[[[3.0, 0.0, 3.1]], [[2.5, 0.0, T(5.0) + T(0.1) * T(2.0)]]]], dtype=T), sat="QT")
    inc2 = T(0.1) * T(2.0)
    assert numpy.array_equal(new["QT"][0, :, 0, 0], [2.0, 3.0]) and numpy.signbit(new["QT"][0, :, 0, 1]).all()
    assert numpy.array_equal(new["QT"][0, :, 0, 2], [T(3.0) + inc2, T(5.0) + inc2])
    assert numpy.array_equal(means["QT"][0], [T(5.0) / T(2), 0.0, ((T(3.0) + inc2) + (T(5.0) + inc2)) / T(2)])
    assert not numpy.signbit(means["QT"][0, 1])                                               # the sum starts from +0.0
    # d = [2-3, 3-2.5 | -0.0-0.0, -0.0-0.0 | 3.2-3.1, 0]: negative -> +0, -0.0 -> +0.0, positive kept
    assert numpy.array_equal(q[0, :, 0, 0], [0.0, 0.5]) and not numpy.signbit(q[0, :, 0, :2]).any()
    assert q[0, 0, 0, 2] == (T(3.0) + inc2) - T(3.1) > 0 and q[0, 1, 0, 2] == 0
    assert numpy.array_equal(means["QL"][0, :2], [0.25, 0.0])
    assert not numpy.array_equal(means["QT"], lar.mean_rows(x))                                 # the mean is of the UPDATED field
    assert numpy.array_equal(lar.les_advance({"QT": x}, {}, 2.0)[0]["QT"], x) and numpy.signbit(lar.les_advance({"QT": x}, {}, 2.0)[0]["QT"][0, 0, 0, 1])


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_on_the_special_inputs_of_the_gpu_test(dtype):
    """what tests/test_les_advance_gpu.py compares the kernel with is not trivial: -0.0 and NaN arrive where it says"""
    fields, tend, qsat = lar.special_case(dtype)
    new, q, means = lar.les_advance(fields, tend, 900.0, qsat, "QT")
    with numpy.errstate(invalid="ignore"):
        d = new["QT"] - qsat
    assert numpy.signbit(d[:, :, :, 0]).all() and (d[:, :, :, 0] == 0).all()                   # d == -0.0 is reached
    assert (d[:, :, :, 1:3] == 0).all() and not numpy.signbit(d[:, :, :, 1:3]).any()           # and d == +0.0
    assert (q[:, :, :, :3] == 0).all() and not numpy.signbit(q[:, :, :, :3]).any()             # both give +0.0
    assert numpy.isnan(q[:, 1, 2, 3]).all() and numpy.isnan(q[:, 2, 2, 4]).all() and numpy.isnan(q[:, :, :, 8]).all()
    assert (q[:, :, :, 5:7] == 0).all() and (d[:, :, :, 5] < 0).all() and numpy.isinf(d[:, :, :, 6]).all()
    assert numpy.isnan(means["QL"][:, [3, 4, 8]]).all() and numpy.isfinite(means["QL"][:, [0, 1, 2, 5, 6, 7, 9, 10, 11]]).all()
    assert numpy.isnan(means["THL"][:, 7]).all() and numpy.isfinite(means["THL"][:, [6, 8]]).all()
    assert numpy.signbit(new["QT"][:, :, :, 0]).all() and numpy.signbit(new["THL"][:, :, :, 1]).all()      # -0.0 + -0.0
    assert (q[:, :, :, 9:] > 0).all()
    # numpy.maximum gives the rule's answer on every one of these inputs (the host twin uses it)
    with numpy.errstate(invalid="ignore"):
        mx = numpy.maximum(d, dtype(0.0))
    num = ~numpy.isnan(q)
    assert numpy.array_equal(mx, q, equal_nan=True) and numpy.array_equal(numpy.signbit(mx)[num], numpy.signbit(q)[num])


def test_oracle_mean_is_numpy_mean_and_the_cases_cover_the_look_ahead():
    rng = numpy.random.default_rng(1)
    f = rng.standard_normal((3, 5, 7, 33))
    assert numpy.array_equal(lar.mean_rows(f), slab_ref.slab_means(f))
    nij = sorted(i * j for i, j in lar.PLANES)
    assert nij == list(range(1, 18))
    assert {x % 8 for x in nij} == set(range(8)) and {8, 16} <= set(nij) and {4, 8, 12, 16} <= set(nij)
    assert [s for s in lar.SHAPES] == [(1, 1, 1, 2), (3, 3, 3, 5), (2, 5, 7, 64), (2, 4, 4, 66), (1, 9, 1, 130), (2, 8, 8, 160)]
    for shape in lar.SHAPES[1:]:                                   # dropping the last row of a plane changes every mean
        fields, tend, qsat = lar.case(shape, numpy.float64)
        new, q, means = lar.les_advance(fields, tend, 900.0, qsat, "QT")
        for k, v in new.items():
            rows = v.reshape(shape[0], -1, shape[-1])
            short = numpy.stack([slab_ref.sequential_mean(r[:-1, None, :]) * (rows.shape[1] - 1) / rows.shape[1] for r in rows])
            assert (short != means[k]).all(), (shape, k)


def test_engine_and_multi_engine_have_the_method_and_the_fake_engines_do_not():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    import inspect
    sig = inspect.signature(Engine.les_advance)
    assert list(sig.parameters) == ["self", "fields", "tend", "dt", "qsat", "sat", "ql", "means", "ql_mean", "stream"]
    assert sig.parameters["ql_mean"].default is True and sig.parameters["sat"].default is None
    assert callable(MultiDeviceEngine.les_advance) and not hasattr(OracleEngine, "les_advance")
    assert models.DeviceLESEnsemble.fused_advance is True


# -- the ensemble: fused step on an oracle-backed engine == unfused step == host twin -----------------------------------------
def _counted(engine, calls):
    inner = engine.les_advance

    def les_advance(*a, **kw):
        calls.append(int(next(iter(a[0].values())).shape[0]))
        return inner(*a, **kw)
    engine.les_advance = les_advance
    return engine


def _compare_logs(a, b):
    assert len(a) == len(b)
    for step, (x, y) in enumerate(zip(a, b)):
        assert x["time"] == y["time"] and set(x["tend"]) == set(y["tend"]) and set(x["prof"]) == set(y["prof"])
        for k in x["tend"]:
            assert numpy.array_equal(x["tend"][k], y["tend"][k], equal_nan=True), (step, "tendency", k)
        for k in x["prof"]:
            assert numpy.array_equal(x["prof"][k], y["prof"][k], equal_nan=True), (step, "profile", k)


def test_closed_loop_fused_unfused_and_host_twin_give_the_same_bits(monkeypatch):
    n, nG, nL, itot, jtot, steps = 5, 19, 40, 6, 5, 3
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)      # the fused path at the sizes of a test
    host, log_h, s_h = dfm._loop(OracleEngine(), slab_ref.HostFieldLESEnsemble, n, nG, nL, itot, jtot, steps)
    calls = []
    fused, log_f, s_f = dfm._loop(_counted(lar.AdvanceOracleEngine(), calls), models.DeviceLESEnsemble, n, nG, nL, itot, jtot, steps)
    assert calls and set(calls) == {n}                            # the fused path was taken, all LES in one call
    taken = len(calls)
    plain, log_p, s_p = dfm._loop(OracleEngine(), models.DeviceLESEnsemble, n, nG, nL, itot, jtot, steps)       # no such method
    monkeypatch.setattr(models.DeviceLESEnsemble, "fused_advance", False)
    off, log_o, s_o = dfm._loop(_counted(lar.AdvanceOracleEngine(), calls), models.DeviceLESEnsemble, n, nG, nL, itot, jtot, steps)
    assert len(calls) == taken                                    # switched off: not called again
    for ens, log, state in ((fused, log_f, s_f), (plain, log_p, s_p), (off, log_o, s_o)):
        dfm.same_state(state, s_h)
        _compare_logs(log_h, log)
        for k in ("U", "V", "THL", "QT", "QL", "Qsat"):
            assert numpy.array_equal(dfm.host_of(ens.fields3d[k]), host.fields3d[k]), k
    assert not numpy.array_equal(log_f[-1]["prof"]["QT"], log_f[0]["prof"]["QT"]) and (log_f[-1]["prof"]["QL"] > 0).any()


def test_closed_loop_fused_in_row_blocks_with_an_empty_device(monkeypatch):
    from sp_coupler_amd.multi import MultiDeviceEngine
    from sp_coupler_amd.transfer import Sharded
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    n, nG, nL, itot, jtot, steps = 2, 19, 40, 6, 5, 2
    host, log_h, s_h = dfm._loop(OracleEngine(), slab_ref.HostFieldLESEnsemble, n, nG, nL, itot, jtot, steps)
    calls = []
    multi = MultiDeviceEngine([_counted(lar.AdvanceOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    dev, log_d, s_d = dfm._loop(multi, models.DeviceLESEnsemble, n, nG, nL, itot, jtot, steps)
    assert calls and set(calls) == {1}                            # blocks 1 + 1 + 0: the empty device is skipped
    dfm.same_state(s_d, s_h)
    _compare_logs(log_h, log_d)
    for k in ("U", "V", "THL", "QT", "QL", "Qsat"):
        assert isinstance(dev.fields3d[k], Sharded) and numpy.array_equal(dfm.host_of(dev.fields3d[k]), host.fields3d[k]), k
    mixed = MultiDeviceEngine([lar.AdvanceOracleEngine(), OracleEngine()], min_cols_per_device=1)          # one engine without the method
    _, log_m, _ = dfm._loop(mixed, models.DeviceLESEnsemble, n, nG, nL, itot, jtot, steps)
    _compare_logs(log_h, log_m)


def test_launches_of_few_les_keep_the_unfused_path(monkeypatch):
    """below FUSED_MIN_LES LES per launch (the measured threshold) the step is torch ops + K10; at it, K11"""
    assert models.DeviceLESEnsemble.FUSED_MIN_LES == 128
    n, nG, nL, itot, jtot = 5, 19, 40, 3, 2
    calls = []
    for limit, taken in ((n + 1, False), (n, True)):
        monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", limit)
        del calls[:]
        dfm._loop(_counted(lar.AdvanceOracleEngine(), calls), models.DeviceLESEnsemble, n, nG, nL, itot, jtot, 1)
        assert bool(calls) == taken, (limit, calls)


def test_one_level_les_keep_the_unfused_path(monkeypatch):
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    calls = []
    eng = _counted(lar.AdvanceOracleEngine(), calls)
    spcpl.set_engine(eng)
    gcm = models.BatchedSyntheticGCM(6, 19, 3)
    ens = models.DeviceLESEnsemble.for_gcm(gcm, [1, 2], nL=1, seed=4, itot=3, jtot=3, engine=eng)
    rng = numpy.random.default_rng(2)
    qt = rng.random((2, 3, 3, 1)) * 1e-2
    ens.attach_fields({"QT": qt.copy(), "Qsat": numpy.full_like(qt, 5e-3)})
    ens.tend["QT"] = numpy.full((2, 1), 1e-6)
    ens.evolve_model_batched(ens.model_time + 100.0)
    assert not calls
    want = qt + (numpy.full((2, 1), 1e-6) * 100.0)[:, None, None, :]
    assert numpy.array_equal(ens.fields3d["QT"].numpy(), want)
    assert numpy.array_equal(ens.p["QL"], slab_ref.slab_means(numpy.maximum(want - 5e-3, 0.0)))


# -- the mutant table of K11 ----------------------------------------------------------------------------------------------
def test_advance_mutants_apply_to_the_tree_and_name_their_guards():
    assert sorted(mc.MUTANTS) == list(range(1, 36))                 # K11's table is kept apart
    assert sorted(mc.ADVANCE_MUTANTS) == list(range(1, len(mc.ADVANCE_MUTANTS) + 1)) and len(mc.ADVANCE_MUTANTS) >= 6
    for n, (what, guard, edits) in mc.ADVANCE_MUTANTS.items():
        assert what and callable(guard) and all(e[0] == mc.ADVANCE for e in edits), n
        assert guard.__name__.split(".", 1)[1] in lar.BODIES and hasattr(lar, "check_" + guard.__name__.split(".", 1)[1]), guard.__name__
        files = mc.patched(n, table=mc.ADVANCE_MUTANTS)
        for name, text in files.items():
            with open(os.path.join(mc.CSRC, name)) as f:
                assert text != f.read(), (n, name)


def test_the_chain_cases_on_the_oracle_backed_engine():
    """the oracle alone handles every case of the chain body, none skipped; its plumbing runs without a GPU"""
    lar.check_chain(lar.AdvanceOracleEngine())
    assert "chain" in lar.BODIES
