"""float32 variability nudge, the parts a CPU can check: the scalar restatements of NumPy's float32 reductions
(tests/vnudge_f32_ref.py), the dtypes of the restatement's intermediates (the contract table of INTEGRATION.md "float32"),
the C ABI of spc_variability_nudge_f32 without a device, and the host logic (chunk sizing by element size, R uploaded as
float64, float32 results handed back) through a CPU stand-in engine."""
import ctypes

import numpy
import pytest
import torch

import __graft_entry__ as ge
from oracle import vnudge_oracle as vo
from sp_coupler_amd import _abi
from tests import vnudge_f32_ref as v32
from tests.test_vnudge import FieldLES, make_les_fields


def test_npsum32_restatement_equals_float32_ndarray_sum_bit_for_bit():
    rng = numpy.random.default_rng(11)
    for n in list(range(1, 301)) + [4096, 8464, 34000]:          # 8464 = 92 x 92: two 8192 chunks; 34 000 = 200 x 170
        a = (rng.normal(size=n) * 10.0 ** rng.integers(-4, 4, size=n)).astype(numpy.float32)
        got = v32.npsum32_restated(a)
        assert got.dtype == numpy.float32 and a.sum().dtype == numpy.float32
        assert got.tobytes() == a.sum().tobytes(), n
    b = numpy.maximum(rng.normal(size=(92, 92)) * 1.3 - 0.2, 0).astype(numpy.float32)   # get_ql_diff's expression class
    assert v32.npsum32_restated(b).tobytes() == b.sum().tobytes()


@pytest.mark.parametrize("shape", [(9, 7), (64, 64), (92, 92), (200, 170)])
def test_std32_restatement_equals_float32_std_bit_for_bit(shape):
    rng = numpy.random.default_rng(shape[0])
    f = (8e-3 + 1e-3 * rng.normal(size=shape + (3,))).astype(numpy.float32)
    want = f.std(axis=(0, 1))
    assert want.dtype == numpy.float32
    for k in range(3):
        assert v32.std32_restated(f[:, :, k]).tobytes() == want[k].tobytes(), (shape, k)


@pytest.mark.parametrize("constantT", [False, True])
def test_restatement_intermediates_have_the_contract_dtypes(constantT):
    f = make_les_fields(16, 12, 40, seed=3)
    numpy.random.seed(42)
    R = vo.make_R(16, 12)
    types = {}
    r = v32.variability_nudge(f["qt"], f["qsat"], f["ql_av"], f["qt_av"], f["presf"], f["ql_ref"], R, 900.0, constantT,
                              thl=f["thl"], ql=f["ql"], types=types)
    assert r["error"] is None
    st = r["status"]
    assert (st & 1).any() and (st & 2).any() and (st & 4).any() and (st == 0).any()      # every branch exercised
    f32, f64 = numpy.dtype(numpy.float32), numpy.dtype(numpy.float64)
    assert types["get_ql_diff"] == f32 and types["barely_unsaturated"] == f32 and types["qt_std"] == f32
    assert types["get_ql_diff_additive"] == f64 and types["beta"] == f64
    assert types["dQT_multiplicative"] == f64 and types["dQT_additive"] == f64 and types["qt"] == f32
    if constantT:
        assert types["dTHL"] == f32 and r["thl"].dtype == f32
    assert r["alpha"].dtype == f64 and r["a"].dtype == f64
    # and it is the float32 evaluation: close to the float64 oracle, not equal to it
    r64 = vo.variability_nudge(f["qt"].astype(numpy.float32), f["qsat"].astype(numpy.float32), f["ql_av"].astype(numpy.float32),
                               f["qt_av"].astype(numpy.float32), f["presf"].astype(numpy.float32),
                               f["ql_ref"].astype(numpy.float32), R, 900.0, constantT,
                               thl=f["thl"].astype(numpy.float32), ql=f["ql"].astype(numpy.float32))
    assert numpy.allclose(r["qt"], r64["qt"], rtol=1e-5, atol=1e-9) and not numpy.array_equal(r["beta"], r64["beta"])


# ---- C ABI without a device -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    return _abi.load_library()


def test_f32_nudge_symbols_exported_and_bound(lib):
    for name in ("spc_variability_nudge_f32", "spc_vnudge_workspace_bytes_f32"):
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name


def test_f32_workspace_is_half_the_f64_one(lib):
    for ext in ((1, 64, 64, 160), (7, 9, 7, 23), (256, 128, 128, 12), (0, 5, 5, 5)):
        b64, b32 = lib.spc_vnudge_workspace_bytes(*ext), lib.spc_vnudge_workspace_bytes_f32(*ext)
        assert b64 >= 0 and b32 * 2 == b64, ext
    assert lib.spc_vnudge_workspace_bytes_f32(1, 0, 5, 5) == _abi.SPC_ERR_INVALID_ARGUMENT
    assert b"bad extents" in lib.spc_last_error()


def test_f32_nudge_rejects_null_pointers_and_bad_extents(lib):
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    assert lib.spc_variability_nudge_f32(None, None) == E and b"NULL" in lib.spc_last_error()
    a = _abi.VnudgeArgs()
    a.n_cols, a.itot, a.jtot, a.ktot = 1, 0, 4, 4
    assert lib.spc_variability_nudge_f32(ctypes.byref(a), None) == E and b"bad extents" in lib.spc_last_error()
    a.itot = 4
    assert lib.spc_variability_nudge_f32(ctypes.byref(a), None) == E and b"qt" in lib.spc_last_error()
    buf = ctypes.create_string_buffer(64)
    for name in ("qt", "qsat", "R", "ql_av", "qt_av", "ql_ref", "beta", "a_add", "qt_std", "status"):
        setattr(a, name, ctypes.cast(buf, ctypes.c_void_p).value)
    a.constantT = 1                                       # constantT needs thl, ql and presf
    assert lib.spc_variability_nudge_f32(ctypes.byref(a), None) == E and b"thl" in lib.spc_last_error()


# ---- host logic through a CPU stand-in engine ---------------------------------------------------------------------------
class F32NudgeEngine:
    """CPU stand-in with the interface Engine.variability_nudge has on a float32 engine: float32 fields and profiles, a
    float64 R (asserted: R is never rounded), results beta / a float64, qt_std float32; qt / thl updated in place.  Each
    column through tests/vnudge_f32_ref.py."""
    device, dtype, stream = torch.device("cpu"), torch.float32, None

    def __init__(self):
        self.launches = 0

    def on_stream(self):
        import contextlib
        return contextlib.nullcontext()

    def variability_nudge(self, qt, qsat, R, ql_av, qt_av, ql_ref, presf=None, thl=None, ql=None, constantT=False, stream=None):
        for name, t in (("qt", qt), ("qsat", qsat), ("ql_av", ql_av), ("qt_av", qt_av), ("ql_ref", ql_ref), ("presf", presf)):
            assert t.dtype == torch.float32, name
        assert R.dtype == torch.float64, "R must reach the nudge in float64"
        self.launches += 1
        n, ktot = int(qt.shape[0]), int(qt.shape[3])
        res = dict(beta=torch.empty(n, ktot, dtype=torch.float64), a=torch.empty(n, ktot, dtype=torch.float64),
                   qt_std=torch.empty(n, ktot, dtype=torch.float32), status=torch.empty(n, ktot, dtype=torch.int32))
        for c in range(n):
            r = v32.variability_nudge(qt[c].numpy(), qsat[c].numpy(), ql_av[c].numpy(), qt_av[c].numpy(), presf[c].numpy(),
                                      ql_ref[c].numpy(), R[c].numpy(), 900.0, constantT,
                                      thl=None if thl is None else thl[c].numpy(), ql=None if ql is None else ql[c].numpy())
            qt[c] = torch.from_numpy(r["qt"])
            if constantT:
                thl[c] = torch.from_numpy(r["thl"])
            for k in ("beta", "a", "qt_std", "status"):
                res[k][c] = torch.from_numpy(numpy.asarray(r[k]))
        return res


def test_f32_nudge_in_chunks_gives_the_bits_of_one_launch_host_logic(monkeypatch):
    """5 LES in chunks of 2 (three launches) against one launch, on the float32 stand-in: same bits, float32 QT / THL handed
    to the model, float64 beta / alpha / a, float32 qt_std -- and equal to the restatement per LES"""
    from sp_coupler_amd import spcpl
    runs = []
    try:
        for limit in (32767, 2):
            eng = F32NudgeEngine()
            spcpl.set_engine(eng)
            monkeypatch.setattr(spcpl, "VN_MAX_COLS", limit)
            fs = [make_les_fields(8, 8, 24, seed=70 + i) for i in range(5)]
            les = [FieldLES(f, f["ql_ref"], i + 1) for i, f in enumerate(fs)]
            numpy.random.seed(3)
            out = spcpl.variability_nudge_batched(les, 900.0, constantT=True, write=False)
            assert eng.launches == (1 if limit > 5 else 3)
            runs.append((out, [m.fields.QT for m in les], [m.fields.THL for m in les], fs))
    finally:
        spcpl.set_engine(None)
    (o1, q1, t1, fs), (o2, q2, t2, _) = runs
    numpy.random.seed(3)
    for i in range(5):
        assert q1[i].dtype == numpy.float32 and t1[i].dtype == numpy.float32
        assert o1[i]["beta"].dtype == numpy.float64 and o1[i]["a"].dtype == numpy.float64
        assert o1[i]["qt_std"].dtype == numpy.float32 and o1[i]["alpha"].dtype == numpy.float64
        for k in ("beta", "alpha", "qt_std", "a", "status"):
            assert numpy.array_equal(o1[i][k], o2[i][k]), (i, k)
        assert numpy.array_equal(q1[i], q2[i]) and numpy.array_equal(t1[i], t2[i]), i
        f = fs[i]
        r = v32.variability_nudge(f["qt"], f["qsat"], f["ql_av"], f["qt_av"], f["presf"], f["ql_ref"], vo.make_R(8, 8), 900.0,
                                  True, thl=f["thl"], ql=f["ql"])
        assert numpy.array_equal(q1[i], r["qt"]) and numpy.array_equal(o1[i]["beta"], r["beta"])
    assert any((o["status"] != 0).any() for o in o1)


def test_chunk_sizing_counts_four_byte_fields_on_a_float32_engine(monkeypatch):
    """_vnudge_chunk: fields and workspace at the engine's element size (the library's f32 workspace query), R at 8 bytes"""
    from sp_coupler_amd import spcpl

    class Lib:
        @staticmethod
        def spc_vnudge_workspace_bytes(n, i, j, k):
            return n * 2 * i * j * k * 8

        @staticmethod
        def spc_vnudge_workspace_bytes_f32(n, i, j, k):
            return n * 2 * i * j * k * 4

    class Eng:
        device, lib = torch.device("cuda", 0), Lib()

        def __init__(self, dtype):
            self.dtype = dtype

    free = 10 * 2 ** 30
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev: (free, 2 * free))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda dev: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda dev: 0)
    nij, ktot = 64 * 64, 160
    for dtype, esize in ((torch.float32, 4), (torch.float64, 8)):
        for constantT, nf in ((False, 2), (True, 4)):
            per_col = nf * nij * ktot * esize + nij * 8 + 8 * ktot * 8 + 2 * nij * ktot * esize
            want = min(32767, int(0.8 * free) // per_col)
            assert spcpl._vnudge_chunk(Eng(dtype), 10 ** 6, 64, 64, ktot, constantT) == want, (dtype, constantT)


def test_float32_multi_device_engine_shards_a_float64_R(monkeypatch):
    """MultiDeviceEngine of float32 engines: ``to_devices(R, rows=n, dtype=torch.float64)`` shards R without rounding it, and
    ``variability_nudge`` on the Sharded arguments gives each engine's block the bits of the restatement"""
    from sp_coupler_amd.multi import MultiDeviceEngine

    class Eng(F32NudgeEngine):
        def synchronize(self):
            pass

    engines = [Eng(), Eng()]
    multi = MultiDeviceEngine(engines, min_cols_per_device=1)
    n = 4
    fs = [make_les_fields(8, 6, 12, seed=60 + i) for i in range(n)]
    numpy.random.seed(2)
    Rs = numpy.stack([vo.make_R(8, 6) for _ in range(n)])
    sh = {k: multi.to_devices(numpy.stack([f[k] for f in fs]), rows=n) for k in ("qt", "qsat", "ql_av", "qt_av", "ql_ref", "presf")}
    R = multi.to_devices(Rs, rows=n, dtype=torch.float64)
    assert all(t.dtype == torch.float64 for t in R.parts) and all(t.dtype == torch.float32 for t in sh["qt"].parts)
    assert multi.to_devices(Rs, rows=n).parts[0].dtype == torch.float32          # default: the engines' dtype
    res = multi.variability_nudge(sh["qt"], sh["qsat"], R, sh["ql_av"], sh["qt_av"], sh["ql_ref"], presf=sh["presf"])
    assert [e.launches for e in engines] == [1, 1]
    beta = torch.cat([t for t in res["beta"].parts]).numpy()
    qt = torch.cat([t for t in sh["qt"].parts]).numpy()
    for i, f in enumerate(fs):
        r = v32.variability_nudge(f["qt"], f["qsat"], f["ql_av"], f["qt_av"], f["presf"], f["ql_ref"], Rs[i], 900.0)
        assert numpy.array_equal(beta[i], r["beta"]) and numpy.array_equal(qt[i], r["qt"]), i
