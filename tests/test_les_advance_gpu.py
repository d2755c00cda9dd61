"""K11 on the MI355X: Engine.les_advance against the NumPy oracle of tests/les_advance_ref.py, bit for bit (fields, ql, every
mean; gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), every array the leading part of a
poisoned buffer whose other bytes are checked afterwards; models.DeviceLESEnsemble's fused step against its unfused step and
its host twin.  The bodies live in tests/les_advance_ref.py: tools/mutation_control.py --advance runs them on wrong kernels."""
import ctypes

import numpy
import pytest
import torch

from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import device_fields_multi as dfm
from tests import les_advance_ref as lar
from tests import slab_ref
from tests.gpu_util import assert_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lar.DTYPES)
@pytest.mark.parametrize("shape", lar.SHAPES)
def test_advance_equals_the_oracle(shape, dtype):
    lar.check_parity(Engine("cuda:0", dtype=dtype), shape)


@pytest.mark.parametrize("dtype", lar.DTYPES)
@pytest.mark.parametrize("ktot", [160, 33])
def test_advance_of_planes_with_every_remainder_of_the_look_ahead(ktot, dtype):
    lar.check_planes(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lar.DTYPES)
@pytest.mark.parametrize("lead,lead_rows,pad", [(1, 0, 0), (0, 1, 0), (3, 3, 0), (0, 0, 4), (0, 0, 3), (2, 1, 5)])
def test_advance_with_views_off_the_16_byte_grid_and_pitched_rows(lead, lead_rows, pad, dtype):
    lar.check_alignment(Engine("cuda:0", dtype=dtype), lead, lead_rows, pad)


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_advance_optional_arguments(dtype):
    lar.check_optional(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_advance_without_a_mean_of_some_fields(dtype):
    """mean[f] == NULL is reachable through the C ABI only: that field is stepped, its mean is not written, and a field with
    neither a tendency nor a mean is not read"""
    eng = Engine("cuda:0", dtype=dtype)
    fields, tend, qsat = lar.case((2, 5, 7, 64), lar.NP[dtype], seed=9)
    want_new, want_q, want_means = lar.les_advance(fields, {k: tend[k] for k in ("U", "QT")}, 900.0, qsat, "QT")
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)          # noqa: E731
    f = {k: dev(v) for k, v in fields.items()}
    t = {k: dev(v) for k, v in tend.items()}
    m = {k: torch.full((2, 64), -1.0, dtype=dtype, device=eng.device) for k in ("U", "V", "THL", "QT", "QL")}
    qs, ql = dev(qsat), torch.full_like(f["QT"], -3.0)
    a = _abi.LesAdvanceArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.pitch_tend, a.pitch_mean, a.dt, a.sat_field = 2, 5, 7, 64, 4, 64, 64, 900.0, 3
    for i, k in enumerate(("U", "V", "THL", "QT")):
        a.fields[i] = f[k].data_ptr()
    a.tend[0], a.tend[3] = t["U"].data_ptr(), t["QT"].data_ptr()           # V, THL: no tendency
    a.mean[1], a.mean[3] = m["V"].data_ptr(), m["QT"].data_ptr()           # U: stepped without a mean; THL: nothing at all
    a.qsat, a.ql, a.ql_mean = qs.data_ptr(), ql.data_ptr(), m["QL"].data_ptr()
    fn = eng.lib.spc_les_advance_f32 if dtype == torch.float32 else eng.lib.spc_les_advance_f64
    with torch.cuda.device(eng.device):
        _abi.check(eng.lib, fn(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)))
    torch.cuda.synchronize()
    for k in fields:
        assert_bits("field " + k, f[k].cpu().numpy(), want_new[k])
    assert_bits("ql", ql.cpu().numpy(), want_q)
    for k in ("V", "QT", "QL"):
        assert_bits("mean " + k, m[k].cpu().numpy(), want_means[k])
    assert bool((m["U"] == -1.0).all()) and bool((m["THL"] == -1.0).all())


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_advance_of_special_values(dtype):
    lar.check_special(Engine("cuda:0", dtype=dtype))


def test_advance_argument_checks_of_the_engine():
    eng = Engine("cuda:0")
    f = torch.zeros((2, 4, 4, 8), dtype=torch.float64, device=eng.device)
    g, t = torch.zeros_like(f), torch.zeros((2, 8), dtype=torch.float64, device=eng.device)
    for bad in (lambda: eng.les_advance({"a": f, "b": g[:, :, :, ::2]}, {}, 1.0),                   # not contiguous / another shape
                lambda: eng.les_advance({"a": f.float()}, {}, 1.0),                                 # not the engine's dtype
                lambda: eng.les_advance({"a": f.cpu()}, {}, 1.0),
                lambda: eng.les_advance({}, {}, 1.0),
                lambda: eng.les_advance({"a": f}, {"b": t}, 1.0),                                   # a tendency without a field
                lambda: eng.les_advance({"a": f}, {"a": t[:, :4]}, 1.0),                            # a tendency of another shape
                lambda: eng.les_advance({"a": f}, {}, 1.0, sat="a"),                                # sat without qsat
                lambda: eng.les_advance({"a": f}, {}, 1.0, qsat=g, sat="b"),
                lambda: eng.les_advance({"a": f}, {}, 1.0, ql=g),
                lambda: eng.les_advance({"a": f}, {}, 1.0, qsat=g, sat="a", ql=f),                  # ql is a field
                lambda: eng.les_advance({"a": f, "b": f}, {}, 1.0)):                                # one field twice
        with pytest.raises(ValueError):
            bad()
    one = torch.zeros((2, 4, 4, 1), dtype=torch.float64, device=eng.device)
    with pytest.raises(_abi.SpcError) as e:
        eng.les_advance({"a": one}, {}, 1.0)
    assert e.value.code == _abi.SPC_ERR_UNSUPPORTED and "ktot == 1" in str(e.value)
    assert eng.les_advance({"a": f[:0]}, {"a": t[:0]}, 1.0)["a"].shape == (0, 8)                    # an empty ensemble: no launch
    torch.cuda.synchronize()
    assert not f.any() and not g.any()


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counting(monkeypatch):
    calls = []
    inner = Engine.les_advance

    def les_advance(self, fields, *a, **kw):
        qt, qs = fields.get("QT"), kw.get("qsat")
        res = inner(self, fields, *a, **kw)
        torch.cuda.synchronize()
        if qt is not None and qs is not None:                    # the inputs leave no qt - qsat == -0.0 (where torch's clamp may differ)
            d = qt - qs
            calls.append(int(((d == 0) & torch.signbit(d)).sum()))
        return res
    monkeypatch.setattr(Engine, "les_advance", les_advance)
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)      # the fused path at the sizes of a test
    return calls


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_fused_step_equals_the_unfused_step_and_the_host_twin(monkeypatch, dtype):
    n, nG, nL, itot, jtot, steps = 5, 19, 40, 6, 5, 3
    calls = _counting(monkeypatch)
    fused, log_f, s_f = dfm._loop(Engine("cuda:0", dtype=dtype), models.DeviceLESEnsemble, n, nG, nL, itot, jtot, steps)
    assert len(calls) >= steps and not any(calls)                 # the fused path ran, and no -0.0 difference occurred
    taken = len(calls)
    monkeypatch.setattr(models.DeviceLESEnsemble, "fused_advance", False)
    plain, log_p, s_p = dfm._loop(Engine("cuda:0", dtype=dtype), models.DeviceLESEnsemble, n, nG, nL, itot, jtot, steps)
    assert len(calls) == taken
    runs = [(plain, log_p, s_p)]
    if dtype == torch.float64:
        host, log_h, s_h = dfm._loop(Engine("cuda:0"), slab_ref.HostFieldLESEnsemble, n, nG, nL, itot, jtot, steps)
        runs.append((host, log_h, s_h))
    for ens, log, state in runs:
        dfm.same_state(state, s_f)
        assert len(log) == len(log_f) == steps + 1
        for step, (a, b) in enumerate(zip(log, log_f)):
            assert a["time"] == b["time"] and set(a["tend"]) == set(b["tend"]) and set(a["prof"]) == set(b["prof"])
            for k in a["tend"]:
                assert numpy.array_equal(a["tend"][k], b["tend"][k], equal_nan=True), (step, "tendency", k)
            for k in a["prof"]:
                assert numpy.array_equal(a["prof"][k], b["prof"][k], equal_nan=True), (step, "profile", k)
        for k in ("U", "V", "THL", "QT", "QL", "Qsat"):
            other = ens.fields3d[k]
            assert numpy.array_equal(fused.fields3d[k].cpu().numpy(), other if isinstance(other, numpy.ndarray) else other.cpu().numpy()), k
    assert not numpy.array_equal(log_f[-1]["prof"]["QT"], log_f[0]["prof"]["QT"]) and (log_f[-1]["prof"]["QL"] > 0).any()


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    blocks = lar.check_multi(one, multi, n)
    assert blocks == ([4, 3] if engines == 2 else [1, 1, 0])


def test_closed_loop_fused_in_row_blocks_equals_the_host_twin(monkeypatch):
    calls = _counting(monkeypatch)
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    dfm.check_closed_loop(Engine("cuda:0"), multi, 2, 5)
    assert len(calls) >= 6 and not any(calls)


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_the_chain_cases(dtype):
    """the cases of the lane's walk that spc_chain.hpp's kernels share, held together (les_advance_ref.check_chain)"""
    lar.check_chain(Engine("cuda:0", dtype=dtype))
