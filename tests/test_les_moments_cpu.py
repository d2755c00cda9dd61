"""K20 without a GPU: the ABI of spc_les_moments_*, the refusals the library makes on the host, the NumPy oracle of
tests/les_moments_ref.py against the vectorised NumPy statement (ndarray.mean / var / std) and against what the special cases
promise, statistics.tke, and models.DeviceLESEnsemble's get_statistics() on an oracle-backed engine against the twin: alone,
beside every other mode, as row blocks with an empty device, and its cache."""
import ctypes
import os
import subprocess

import numpy
import pytest
import torch

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import statistics as st
from tests import les_moments_ref as mr
from tests import les_qt_local_ref as qlr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPS = [numpy.float64, numpy.float32]
SHAPES = [(3,) + p + (k,) for p in mr.PLANES for k in mr.KTOTS] + [(1, 64, 64, 2), (1, 33, 31, 5)]


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
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror; the two limits; the ABI version has not moved"""
    cls, cname = _abi.LesMomentsArgs, "spc_les_moments_args"
    fields = ["n_les", "itot", "jtot", "ktot", "n_fields", "n_pairs", "face_field", "fields", "pair_a", "pair_b", "mean", "var", "std", "cov",
              "pitch_out"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_ABI_VERSION);',
             'printf("%d\\n", SPC_MOMENTS_MAX_FIELDS);', 'printf("%d\\n", SPC_MOMENTS_MAX_PAIRS);']
    want = [ctypes.sizeof(cls), 4, _abi.MOMENTS_MAX_FIELDS, _abi.MOMENTS_MAX_PAIRS]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and _abi.MOMENTS_MAX_FIELDS == 8 and _abi.MOMENTS_MAX_PAIRS == 8 and len(st.FIELDS) <= 8 and len(st.PAIRS) <= 8


def _args(n=4, itot=8, jtot=8, ktot=20, n_fields=3, pairs=((0, 2), (1, 0)), face=1, pitch=None, kinds=mr.KINDS, esize=8):
    """distinct pointers on the 16-byte grid, never dereferenced"""
    a = _abi.LesMomentsArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.n_pairs, a.face_field = n, itot, jtot, ktot, n_fields, len(pairs), face
    a.pitch_out = ktot if pitch is None else pitch
    at = 4096
    for f in range(max(0, min(n_fields, 8))):
        a.fields[f] = at
        at += 4096
        for kind in kinds:
            getattr(a, kind)[f] = at
            at += 4096
    for q, (pa, pb) in enumerate(pairs[:8]):
        a.pair_a[q], a.pair_b[q], a.cov[q] = pa, pb, at
        at += 4096
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_moments_" + sfx)

    def call(edit=None, **kw):
        a = _args(**kw)
        if edit:
            edit(a)
        return fn(ctypes.byref(a), None), lib.spc_last_error()

    def put(member, i, value):
        def edit(a):
            getattr(a, member)[i] = value
        return edit
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    rc, text = call(ktot=1)
    assert rc == U and b"ktot == 1" in text
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    for bad in (dict(itot=4096, jtot=4097), dict(itot=1 << 20, jtot=1 << 20)):
        rc, text = call(**bad)
        assert rc == E and b"2^24" in text
    assert call(itot=4096, jtot=4096, n=1 << 40)[0] == U           # (2^24 itself is allowed; the grid is what fails here)
    rc, text = call(pitch=19)
    assert rc == E and b"pitch_out" in text
    for bad in (0, 9, -1):
        rc, text = call(n_fields=bad, pairs=(), face=-1)
        assert rc == E and b"field count" in text
    rc, text = call(edit=lambda a: setattr(a, "n_pairs", 9))
    assert rc == E and b"pair count" in text
    rc, text = call(edit=lambda a: setattr(a, "n_pairs", -1))
    assert rc == E and b"pair count" in text
    for face in (3, -2, 8):
        rc, text = call(face=face)
        assert rc == E and b"face_field" in text
    for pairs, which in ((((0, 3),), b"pair 0"), (((0, 1), (-1, 0)), b"pair 1"), (((2, 2),), b"pair 0"), (((0, 1), (1, 0), (1, 8)), b"pair 2")):
        rc, text = call(pairs=pairs)
        assert rc == E and which in text
    rc, text = call(edit=put("fields", 1, None))
    assert (rc, text) == (E, b"required pointer fields[f] is NULL")
    rc, text = call(kinds=(), pairs=())
    assert rc == E and b"no output" in text
    rc, text = call(kinds=(), edit=lambda a: [put("cov", q, None)(a) for q in range(2)])
    assert rc == E and b"no output" in text
    for member, i, other in (("mean", 0, ("fields", 2)), ("cov", 1, ("fields", 0)), ("var", 1, ("std", 1)), ("cov", 0, ("mean", 2)), ("std", 2, ("cov", 1))):
        rc, text = call(edit=lambda a, m=member, i=i, o=other: put(m, i, getattr(a, o[0])[o[1]])(a))
        assert rc == E and b"same array" in text, (member, i, other)
    rc, text = call(edit=put("fields", 0, 4100 if sfx == "f64" else 4098))
    assert rc == E and b"not aligned" in text
    rc, text = call(edit=put("cov", 0, 4096 * 100 + 2))
    assert rc == E and b"not aligned" in text
    rc, text = call(n=1 << 40, ktot=3)
    assert rc == U and b"too many workgroups" in text
    empty = _args(n=0, kinds=(), pairs=())
    for f in range(3):
        empty.fields[f] = None
    assert fn(ctypes.byref(empty), None) == 0                      # an empty ensemble is a no-op, whatever its pointers
    assert lib.spc_abi_version() == 4


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    assert callable(Engine.les_moments) and callable(MultiDeviceEngine.les_moments)
    assert not hasattr(qlr.QtLocalOracleEngine, "les_moments")


# -- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_equals_the_vectorised_statement(shape, dtype):
    """the literal loop == ndarray.mean / var / std and the mean of the product of the deviations, with the face average"""
    fields = mr.case(shape, dtype)
    for face in ("C", None):
        a, b = mr.les_moments(fields, mr.PAIRS3, face), mr.les_moments_vectorised(fields, mr.PAIRS3, face)
        assert all(v.dtype == dtype for d in b.values() for v in d.values())
        mr.same_results("face %s" % face, a, b)


@pytest.mark.parametrize("dtype", NPS)
def test_special_values_are_in_their_cases_and_numpy_agrees(dtype):
    cases = mr.special_cases(dtype)
    assert numpy.isnan(cases["nan"][0]["A"]).sum() == 1 and numpy.isnan(cases["nan"][0]["C"]).sum() == 1
    assert numpy.isinf(cases["inf"][0]["B"]).sum() == 1 and numpy.isinf(cases["inf"][0]["A"]).sum() == 1
    zero = cases["zeros"][0]
    assert numpy.signbit(zero["A"][0, :, :, 3]).all() and not zero["A"][0, :, :, 3].any() and numpy.signbit(zero["C"][..., :2]).all()
    assert (zero["B"][1, :, :, 5] == 287.25).all()
    big = cases["big"][0]["A"]
    assert (numpy.abs(big - 1e5) < 0.1).all() and (big != big.ravel()[0]).any()
    for name, (fields, pairs, face) in cases.items():
        mr.same_results(name, mr.les_moments(fields, pairs, face), mr.les_moments_vectorised(fields, pairs, face))
    # what a contracted product or a one-pass formula would give on the big case is not what the rule gives
    f, T = cases["big"][0], dtype
    res = mr.les_moments(f, cases["big"][1])
    x = f["A"].astype(numpy.float64)
    one_pass = ((x * x).mean(axis=(1, 2)).astype(T) - (res["mean"]["A"] * res["mean"]["A"])).astype(T)
    assert not numpy.array_equal(one_pass, res["var"]["A"])
    exact = x.var(axis=(1, 2))
    rel = numpy.abs(res["var"]["A"].astype(numpy.float64) - exact) / exact
    assert rel.max() < (0.5 if dtype is numpy.float32 else 1e-6)    # (float32: the cells themselves are rounded to 2^-7)


def test_tke_and_the_tables():
    var = {"U": numpy.float32([[1.0, 2.0]]), "V": numpy.float32([[0.5, 0.25]]), "W": numpy.float32([[0.25, 0.0]])}
    t = st.tke(var)
    assert t.dtype == numpy.float64 and numpy.array_equal(t, [[0.875, 1.125]])
    del var["W"]
    assert numpy.array_equal(st.tke(var), [[0.75, 1.125]])
    assert st.FIELDS == ("U", "V", "W", "THL", "QT", "QL", "QR") and st.FACE == "W"
    assert st.PAIRS == (("W", "THL"), ("W", "QT"), ("U", "W"), ("V", "W"), ("THL", "QT"))


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    inner = engine.les_moments
    engine.les_moments = lambda fields, *a, **kw: (calls.append((id(engine), sorted(fields))), inner(fields, *a, **kw))[1]
    return engine


@pytest.mark.parametrize("variant", list(mr.VARIANTS))
def test_ensemble_on_one_engine_equals_the_twin(variant):
    """after the attach, each of three steps and the nudge: every statistic bit-equal to the twin's, ONE launch per change, none
    for a second read, the rows equal to the batched getter (asserted inside); with vertical advection W and its fluxes appear"""
    calls = []
    ens, log = mr.ensemble_run(_counted(mr.MomentsOracleEngine(), calls), 4, calls, **mr.VARIANTS[variant])
    assert len(calls) == 5
    assert ("cov W-THL" in log[-1]) == (variant == "all") and ("var W" in log[0]) is False
    assert not numpy.array_equal(log[1]["var QT"], log[2]["var QT"]) and (log[-1]["TKE"] > 0).all()
    if variant == "all":
        assert calls[-1][1] == ["QL", "QR", "QT", "THL", "U", "V", "W"] and log[-1]["cov W-QT"].any()


def test_ensemble_as_row_blocks_with_an_empty_device():
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(mr.MomentsOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    one = mr.ensemble_run(mr.MomentsOracleEngine(), 2, **mr.VARIANTS["all"])[1]
    log = mr.ensemble_run(multi, 2, calls, **mr.VARIANTS["all"])[1]
    assert len(calls) == 10                                        # blocks 1 + 1 + 0: two devices, five changes
    qlr.lmr.same_logs(one, log)


def _small(eng, n=2, nL=6, names=("U", "V", "THL", "QT", "Qsat")):
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(n, nL=nL)
    ens = models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)
    rng = numpy.random.default_rng(1)
    base = {"U": 5.0, "V": -2.0, "THL": 290.0, "QT": 9e-3, "Qsat": 8.7e-3, "QR": 1e-5}
    ens.attach_fields({k: base[k] * (1.0 + 0.05 * rng.random((n, 2, 3, nL))) for k in names})
    return ens


def test_every_change_of_a_field_launches_again_and_nothing_else_does():
    calls = []
    eng = _counted(mr.MomentsOracleEngine(), calls)
    ens = _small(eng)

    def reads():
        before = len(calls)
        ens.get_statistics()
        first = len(calls) - before
        ens.get_statistics_batched()
        ens[1].get_statistics()
        ens.get_statistics(("QT",), ())
        assert len(calls) - before == first
        return first
    assert reads() == 1 and reads() == 0
    # what changes no field: profiles, water paths, forcings handed over, the cloud fraction
    out = {k: numpy.empty((2, 6)) for k in ("QT", "QL")}
    ens.get_profiles_batched(("QT", "QL"), out)
    ens.get_water_paths_batched(("LWP", "TWP"))
    ens.set_forcings_batched(QT=numpy.full((2, 6), 1e-8), THL=numpy.full((2, 6), 1e-4))
    ens.get_cloudfraction_batched(numpy.full((2, 3), 2, dtype=numpy.int32), numpy.empty((2, 3)))
    assert reads() == 0
    # what does
    t = float(ens.model_time)
    ens.evolve_model_batched(t + 100.0)
    assert reads() == 1
    ens.set_fields_batched("QT", ens.get_fields_batched("QT"))
    assert reads() == 1
    numpy.random.seed(3)
    ens.ql_ref = numpy.full((2, 6), 1e-4)
    spcpl.variability_nudge_ensemble(ens, 900.0, True, write=False)
    assert reads() == 1
    for enable in ("enable_thermo", "enable_diffusion", "enable_microphysics", "enable_radiation",
                   lambda: ens.enable_advection(dx=5e4, dy=5e4, vertical=True), lambda: ens.enable_qt_forcing("local")):
        (enable if callable(enable) else getattr(ens, enable))()
        t += 100.0
        ens.evolve_model_batched(t)
        assert reads() == 1, enable
    got = ens.get_statistics()
    assert set(got["var"]) == set(st.FIELDS) and set(got["cov"]) == set(st.PAIRS) and "TKE" in got
    # only what is missing is launched: a new name, a new pair
    ens.evolve_model_batched(t + 100.0)
    before = len(calls)
    a = ens.get_statistics_batched(("QT",), ())
    assert list(a["mean"]) == ["QT"] and a["cov"] == {} and calls[-1][1] == ["QT"]
    b = ens.get_statistics_batched(("QT", "U"), (("U", "QT"),))
    assert calls[-1][1] == ["QT", "U"] and list(b["cov"]) == [("U", "QT")] and len(calls) - before == 2
    assert b["var"]["QT"] is a["var"]["QT"]
    want = mr.twin_statistics(ens, models.DeviceLESEnsemble._host(ens.get_vertical_wind_batched()), ("QT", "U"), (("U", "QT"),))
    for k, v in mr.flat(ens.get_statistics(("QT", "U"), (("U", "QT"),))).items():
        assert_bits(k, v, mr.flat(want)[k])


def test_names_without_a_field_and_engines_without_the_kernel():
    ens = _small(mr.MomentsOracleEngine(), names=("THL", "QT"))
    got = ens.get_statistics()
    assert sorted(got["var"]) == ["QT", "THL"] and list(got["cov"]) == [("THL", "QT")] and "TKE" not in got
    assert sorted(ens.get_statistics(("U", "QT", "W"))["mean"]) == ["QT"]
    with pytest.raises(KeyError, match="holds no field"):
        ens.get_statistics(("U", "QR"))
    with pytest.raises(KeyError, match="no statistics of"):
        ens.get_statistics(("T",))
    old = _small(qlr.QtLocalOracleEngine())
    with pytest.raises(ValueError, match="les_moments"):
        old.get_statistics_batched()
    with pytest.raises(ValueError, match="les_moments"):
        old[0].get_statistics()
    # ... and every other path of such an ensemble is what it was: the same steps on both engines, bit for bit
    new = _small(mr.MomentsOracleEngine())
    for e in (old, new):
        e.set_forcings_batched(QT=numpy.full((2, 6), 1e-8), THL=numpy.full((2, 6), 1e-4))
        e.evolve_model_batched(float(e.model_time) + 100.0)
    new.get_statistics()
    for k in ("U", "V", "THL", "QT", "QL"):
        assert_bits(k, models.DeviceLESEnsemble._host(new.get_fields_batched(k)), models.DeviceLESEnsemble._host(old.get_fields_batched(k)))
        assert_bits("p " + k, new.p[k], old.p[k])


def test_the_chain_cases_on_the_oracle_backed_engine():
    """the oracle alone handles every case of the chain body, none skipped; its plumbing runs without a GPU"""
    mr.check_chain(mr.MomentsOracleEngine())
    assert "chain" in mr.BODIES


# -- the same on float32 engines -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(mr.VARIANTS))
def test_float32_ensemble_on_one_engine_equals_the_twin(variant):
    """test_ensemble_on_one_engine_equals_the_twin on a float32 engine: the statistics are K20's float32 results, widened exactly"""
    calls = []
    ens, log = mr.ensemble_run(_counted(f32_of(mr.MomentsOracleEngine)(), calls), 4, calls, **mr.VARIANTS[variant])
    assert len(calls) == 5 and all(t.dtype == torch.float32 for t in ens.get_statistics_batched()["var"].values())
    assert ("cov W-THL" in log[-1]) == (variant == "all") and ("var W" in log[0]) is False
    assert not numpy.array_equal(log[1]["var QT"], log[2]["var QT"]) and (log[-1]["TKE"] > 0).all()
    assert all(numpy.array_equal(v, v.astype(numpy.float32)) for k, v in log[-1].items() if k != "TKE")


def test_float32_ensemble_as_row_blocks_with_an_empty_device():
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(mr.MomentsOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    one = mr.ensemble_run(f32_of(mr.MomentsOracleEngine)(), 2, **mr.VARIANTS["all"])[1]
    log = mr.ensemble_run(multi, 2, calls, **mr.VARIANTS["all"])[1]
    assert len(calls) == 10
    qlr.lmr.same_logs(one, log)
