"""K13 without a GPU: the NumPy oracle of tests/les_water_paths_ref.py against per-row ndarray.sum() and against the k loop, the
inputs of the GPU bodies, the struct layout of spc_water_path_args and the host-side refusals of spc_les_water_paths_*, and the
water-path methods of models.DeviceLESEnsemble on oracle-backed engines against their host twin."""
import ctypes
import os
import subprocess

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from tests import les_water_paths_ref as wpr
from tests.les_harness import f32_of
from tools import mutation_control as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = [numpy.float64, numpy.float32]


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


# -- the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("ktot", wpr.KTOTS)
def test_oracle_is_the_pairwise_row_sum_and_not_the_k_loop(ktot, dtype):
    """(field * w).sum(axis=3) equals ndarray.sum() of every row on its own, bit for bit, and from ktot = 8 on the inputs of the
    GPU bodies give another result when summed in order: the pairwise requirement is not vacuous"""
    for nf_seed in (0, 1):
        fields, w = wpr.case((3, 3, 5, ktot), dtype, 1, seed=nf_seed)
        want = wpr.water_paths(fields[0], w)
        assert want.dtype == dtype and want.shape == (3, 3, 5)
        assert numpy.array_equal(want, wpr.per_row_sum(fields[0], w))
        seq = wpr.sequential(fields[0], w)
        if ktot < 8:
            assert numpy.array_equal(want, seq)
        else:
            assert not numpy.array_equal(want, seq)
            assert (want != seq).mean() > (0.2 if ktot > 9 else 0.02)
            scale = numpy.abs(fields[0] * w[:, None, None, :]).sum(axis=3).astype(numpy.float64)
            assert (numpy.abs(want.astype(numpy.float64) - seq) <= ktot * numpy.finfo(dtype).eps * scale).all()


@pytest.mark.parametrize("dtype", DT)
def test_the_product_is_rounded_before_the_sum(dtype):
    """x = 1 + 2^-p: x * x = 1 + 2^(1-p) + 2^-2p exactly, which rounds to 1 + 2^(1-p); (x * x) + (-1) is then 2^(1-p), where an
    fma of the exact product would keep the 2^-2p"""
    p = 27 if dtype == numpy.float64 else 12
    x = dtype(1 + 2.0 ** -p)
    f = numpy.zeros((1, 1, 1, 2), dtype)
    f[0, 0, 0] = [x, -1.0]
    w = numpy.array([[x, 1.0]], dtype)
    assert wpr.water_paths(f, w)[0, 0, 0] == dtype(2.0 ** (1 - p))
    assert numpy.longdouble(x) * numpy.longdouble(x) - 1 != numpy.longdouble(2.0 ** (1 - p))


@pytest.mark.parametrize("dtype", DT)
def test_cloud_inputs_reach_what_they_name(dtype):
    q, w = wpr.cloud_case(dtype, 40)
    top = wpr.cloud_top(q)
    assert top.dtype == numpy.int32 and top.shape == (3, 3, 5)
    assert (top[0] == -1).all() and (top[1] >= 0).all() and top[2, 0].tolist() == [0, 39, -1, -1, -1]
    cover = wpr.cover_of(top, dtype)
    assert cover.dtype == dtype and cover[0] == 0 and cover[1] == 1 and cover[2] == dtype(int((top[2] >= 0).sum())) / dtype(15)
    wp = wpr.water_paths(q, w)
    assert numpy.isnan(wp[2, 0, 2]) and wp[0, 0, 0] == 0 and not numpy.signbit(wp[0, 0, 0]) and wp[2, 0, 4] < 0
    # by hand
    f = numpy.array([[[[0.0, 2.0, -0.0, numpy.nan, 3.0, 0.0]]]], dtype)
    assert wpr.cloud_top(f)[0, 0, 0] == 4 and wpr.cloud_top(-f)[0, 0, 0] == -1


# -- ABI ---------------------------------------------------------------------------------------------------------------------
def test_struct_layout_of_the_water_path_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.WaterPathArgs, "SpcWaterPathArgs"
    fields = ["n_les", "itot", "jtot", "ktot", "n_fields", "fields", "out", "w", "pitch_w", "cloud_field", "reserved", "top", "cover"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_WP_MAX_FIELDS);']
    want = [ctypes.sizeof(cls), _abi.WP_MAX_FIELDS]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(spc_water_path_args, %s));' % f)
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and _abi.WP_MAX_FIELDS == 4


def _args(n=4, itot=8, jtot=8, ktot=20, n_fields=2, pitch_w=20, cloud_field=-1, **ptr):
    a = _abi.WaterPathArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.pitch_w, a.cloud_field = n, itot, jtot, ktot, n_fields, pitch_w, cloud_field
    for f in range(max(0, min(n_fields, 4))):                    # distinct, 16-byte aligned, never dereferenced
        a.fields[f] = ptr.get("fields%d" % f, 4096 * (f + 1))
        a.out[f] = ptr.get("out%d" % f, 4096 * (f + 9))
    a.w = ptr.get("w", 4096 * 20)
    a.top, a.cover = ptr.get("top", None), ptr.get("cover", None)
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_water_path_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_water_paths_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    for name in ("fields0", "fields1", "out0", "out1", "w"):
        rc, text = call(**{name: None})
        assert rc == E and b"required pointer" in text and b"is NULL" in text, (name, text)
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    rc, text = call(itot=65536, jtot=32768)
    assert rc == U and b"2^31 - 1 points per plane" in text
    for bad in (0, 5, -1):
        rc, text = call(n_fields=bad)
        assert rc == E and b"field count" in text
    rc, text = call(pitch_w=19)
    assert rc == E and b"pitch_w" in text and b"smaller than ktot" in text
    rc, text = call(ktot=8193, pitch_w=8193)
    assert rc == U and b"8192" in text
    for bad in (2, -2):
        rc, text = call(cloud_field=bad)
        assert rc == E and b"cloud_field" in text
    for bad in (dict(out0=4096), dict(out1=4096 * 9), dict(out0=4096 * 20), dict(cloud_field=0, top=4096 * 9), dict(cloud_field=0, cover=4096),
                dict(cloud_field=1, top=4096 * 30, cover=4096 * 30)):
        rc, text = call(**bad)
        assert rc == E and (b"an output is" in text or b"top or cover is" in text), (bad, text)
    rc, text = call(fields0=4097)
    assert rc == E and b"not aligned" in text
    assert call(n=0, fields0=None, out0=None, w=None) == (0, lib.spc_last_error())          # an empty ensemble: no launch


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    from tests.fake_engine import OracleEngine
    assert callable(Engine.les_water_paths) and callable(MultiDeviceEngine.les_water_paths) and not hasattr(OracleEngine, "les_water_paths")


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    inner = engine.les_water_paths
    engine.les_water_paths = lambda fields, *a, **kw: (calls.append((tuple(fields), int(next(iter(fields.values())).shape[0]))), inner(fields, *a, **kw))[1]
    return engine


@pytest.mark.parametrize("thermo", [False, True])
def test_ensemble_on_one_engine_equals_the_host_twin(thermo):
    calls = []
    wpr.check_ensemble(wpr.WaterPathOracleEngine(), [_counted(wpr.WaterPathOracleEngine(), calls)], 4, thermo)
    assert calls == [(("LWP", "TWP", "RWP"), 4)] * 3              # one launch per state of the fields: everything else is cached


@pytest.mark.parametrize("thermo", [False, True])
def test_ensemble_as_row_blocks_with_an_empty_device(thermo):
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(wpr.WaterPathOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    wpr.check_ensemble(wpr.WaterPathOracleEngine(), [multi], 2, thermo)
    assert calls == [(("LWP", "TWP", "RWP"), 1)] * 6              # blocks 1 + 1 + 0: the device without rows launches nothing


def test_names_without_a_field_and_the_cache():
    calls = []
    eng = _counted(wpr.WaterPathOracleEngine(), calls)
    ens, log = wpr.ensemble_run(eng, 3, False, True, with_qr=False)
    host = wpr.ensemble_run(wpr.WaterPathOracleEngine(), 3, False, False, with_qr=False)[1]
    wpr.same_logs(host, log, with_qr=False)
    assert all("RWP" not in rec for rec in log)
    with pytest.raises(KeyError):
        ens.get_water_paths_batched(("RWP",))
    with pytest.raises(KeyError):
        ens.get_water_paths_batched(("LWP", "IWP"))
    with pytest.raises(NotImplementedError):
        ens[0].get_field("QT")
    del calls[:]
    a = ens.get_water_paths_batched(("TWP",))
    b = ens.get_water_paths_batched(("LWP", "TWP"), cloud_cover=True)
    assert calls == [] and a["TWP"] is b["TWP"] and list(b) == ["LWP", "TWP", "top", "cover"]
    assert ens[1].get_field("LWP").shape == (4, 5) and calls == []
    ens.set_fields_batched("QT", ens.get_fields_batched("QT") * 2.0)
    c = ens.get_water_paths_batched(("TWP",))
    assert calls == [(("TWP",), 3)] and numpy.array_equal(c["TWP"].numpy(), 2.0 * a["TWP"].numpy())
    ens.set_fields_batched("QT", ens.get_fields_batched("QT") * 1.0)   # the cache dropped, nothing fetched: LWP is not cached
    del calls[:]
    g = ens.get_water_paths_batched(("TWP",), cloud_cover=True)
    assert calls == [(("LWP", "TWP"), 3)] and list(g) == ["TWP", "top", "cover"]
    fresh = wpr.ensemble_run(_counted(wpr.WaterPathOracleEngine(), []), 3, False, True, with_qr=False)[0]
    fresh.evolve_model_batched(2700.0)
    assert list(fresh.get_water_paths_batched(("TWP",), cloud_cover=True)) == ["TWP", "top", "cover"]
    ens.set_fields_batched("QT", ens.get_fields_batched("QT") * 1.0)
    c = ens.get_water_paths_batched(("TWP",))
    del calls[:]
    calls.append(None)
    lwp = ens.get_water_paths_batched(("LWP",))["LWP"]
    d = ens.get_water_paths_batched(("TWP",), cloud_cover=True)    # the cover was dropped with the cache: the cloud pass walks QL
    assert calls[1:] == [(("LWP",), 3), (("LWP",), 3)] and d["TWP"] is c["TWP"]
    assert ens.get_water_paths_batched(("LWP",))["LWP"] is lwp      # ... and writes LWP again into the tensor a caller may hold
    before = lwp.numpy().copy()
    ens.p["Rhobf"] = ens.p["Rhobf"] * 2.0                          # other weights: nothing cached is handed out
    del calls[:]
    e = ens.get_water_paths_batched(("LWP", "TWP"), cloud_cover=True)
    assert calls == [(("LWP", "TWP"), 3)] and numpy.array_equal(e["LWP"].numpy(), 2.0 * before) and numpy.array_equal(e["cover"].numpy(), d["cover"].numpy())
    w = ens.water_path_weights()
    zh = numpy.asarray(ens.zh_cache)
    assert numpy.array_equal(w[:, :-1], ens.p["Rhobf"][:, :-1] * (zh[1:] - zh[:-1])) and numpy.array_equal(w[:, -1], ens.p["Rhobf"][:, -1] * (zh[-1] - zh[-2]))


# -- mutants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thermo", [False, True])
def test_ensemble_against_the_oracle_on_its_own_fields(thermo):
    """the body of the GPU file's dtype cases, on the oracle-backed engine (float64)"""
    wpr.check_ensemble_dtype(wpr.WaterPathOracleEngine(), 4, thermo)


def test_few_rows_inputs_are_what_they_name():
    class Eng(wpr.WaterPathOracleEngine):
        pass
    wpr.check_few_rows(Eng())


def test_water_path_mutants_apply_to_the_tree_and_name_their_guards():
    table = mc.WATERPATH_MUTANTS
    assert sorted(table) == list(range(1, len(table) + 1)) and len(table) >= 6
    for n, (what, guard, edits) in table.items():
        assert what and edits and callable(guard) and all(e[0] == mc.WATERPATH for e in edits), n
        mod, name = guard.__name__.split(".", 1)
        assert mod == "les_water_paths_ref" and name in wpr.BODIES and hasattr(wpr, "check_" + name), (n, guard.__name__)
        files = mc.patched(n, table=table)
        for fname, text in files.items():
            with open(os.path.join(mc.CSRC, fname)) as f:
                assert text != f.read(), (n, fname)
    libs = [mc.lib_of(n, t) for t in (mc.MUTANTS, mc.ADVANCE_MUTANTS, mc.THERMO_MUTANTS, mc.WATERPATH_MUTANTS) for n in t]
    assert len(set(libs)) == len(libs) and mc.lib_of(2, table).endswith("libspc_waterpath_mutant2.so")


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("thermo", [False, True])
def test_float32_ensemble_on_one_engine_equals_the_host_twin(thermo):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    calls = []
    wpr.check_ensemble(f32_of(wpr.WaterPathOracleEngine)(), [_counted(f32_of(wpr.WaterPathOracleEngine)(), calls)], 4, thermo)
    assert calls == [(("LWP", "TWP", "RWP"), 4)] * 3              # one launch per state of the fields: everything else is cached


@pytest.mark.parametrize("thermo", [False, True])
def test_float32_ensemble_as_row_blocks_with_an_empty_device(thermo):
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(wpr.WaterPathOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    wpr.check_ensemble(f32_of(wpr.WaterPathOracleEngine)(), [multi], 2, thermo)
    assert calls == [(("LWP", "TWP", "RWP"), 1)] * 6              # blocks 1 + 1 + 0: the device without rows launches nothing
