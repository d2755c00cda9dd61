"""K20 on the MI355X: Engine.les_moments against the NumPy oracle of tests/les_moments_ref.py, bit for bit
(gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), in float64 and float32, every array the leading
part of a poisoned buffer whose other bytes are checked afterwards, the fields compared with what was uploaded; and
models.DeviceLESEnsemble's get_statistics() against its twin.  The bodies live in tests/les_moments_ref.py:
tools/mutation_control.py --moments runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_moments_ref as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", mr.DTYPES)
@pytest.mark.parametrize("ktot", mr.KTOTS)
@pytest.mark.parametrize("plane", mr.PLANES)
def test_moments_equal_the_oracle(plane, ktot, dtype):
    """five fields, three pairs, one field at the faces, all four kinds of output"""
    mr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", mr.DTYPES)
def test_field_and_pair_counts(dtype):
    """1 and 8 fields, 0 and 8 pairs, a field in four pairs, (a, b) and (b, a), each kind alone, only the covariances"""
    mr.check_counts(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", mr.DTYPES)
@pytest.mark.parametrize("ktot", [7, 8, 65])
def test_other_data_per_les(ktot, dtype):
    """n = 1, 2, 5, pitched outputs; at ktot 7 and 8 adjacent LES share a wave"""
    mr.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", mr.DTYPES)
def test_the_face_field(dtype):
    """first, last and in the middle; ktot 2, 3, 8, 65; NaN directly in front of the field: x[-1] is never read"""
    mr.check_face(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", mr.DTYPES)
def test_special_values(dtype):
    """a NaN cell, an infinity, planes of -0.0, a constant plane, 1e5 with deviations of some 1e-3"""
    mr.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", mr.DTYPES)
@pytest.mark.parametrize("ktot,pad", [(65, 0), (64, 0), (160, 0), (160, 1), (7, 2)])
def test_views_off_the_16_byte_grid(ktot, pad, dtype):
    mr.check_alignment(Engine("cuda:0", dtype=dtype), ktot, pad)


@pytest.mark.parametrize("dtype", mr.DTYPES)
def test_refusals(dtype):
    """every line of the refusal list of include/spc.h through the C ABI and through the engine, and n = 0"""
    mr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", mr.DTYPES)
def test_means_are_k10s_and_std_is_k6s(dtype):
    mr.check_same_as_k10_k6(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", mr.DTYPES)
def test_large_planes(dtype):
    """one LES of 64 x 64 x 2 and of 33 x 31 x 5: long chains, the long-plane launch, the ragged tail of the load-ahead loop"""
    mr.check_large_plane(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert mr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(mr.VARIANTS))
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_statistics_equal_the_twin(monkeypatch, n, variant):
    """the attached fields, three steps and one constantT nudge before the last, on one engine and on two engines sharing the
    card, plain and with diffusion + thermo + microphysics + horizontal and vertical advection + radiation (W exists): after
    each of them every statistic bit-equal to the twin, ONE launch per device per change, none for a second read, the row
    getter equal to the batched getter (all asserted inside ensemble_run)"""
    calls = []
    inner = Engine.les_moments
    monkeypatch.setattr(Engine, "les_moments", lambda self, fields, *a, **kw: (calls.append((id(self), sorted(fields))), inner(self, fields, *a, **kw))[1])
    one = Engine("cuda:0")
    ens, log = mr.ensemble_run(one, n, calls, **mr.VARIANTS[variant])
    assert len(calls) == 5 and ("cov W-THL" in log[-1]) == (variant == "all") and (log[-1]["TKE"] > 0).all()
    del calls[:]
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    mlog = mr.ensemble_run(multi, n, calls, **mr.VARIANTS[variant])[1]
    assert len(calls) == 10 and {i for i, _ in calls} == {id(e) for e in multi.engines}
    mr.qlr.lmr.same_logs(log, mlog)


@pytest.mark.parametrize("dtype", mr.DTYPES)
def test_the_chain_cases(dtype):
    """the cases of the lane's walk that spc_chain.hpp's kernels share, held together, for both forms (les_moments_ref.check_chain)"""
    mr.check_chain(Engine("cuda:0", dtype=dtype))
