"""K10 without a GPU: the NumPy oracle of tests/slab_ref.py against answers counted by hand, the summation order of
numpy.mean that k_slab_means copies, and the host-side argument checks of the four entry points."""
import ctypes

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi
from tests import slab_ref


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    return _abi.load_library()


def test_layer_ranges_of_the_reference_known_answer():
    """idx = [0, 0, 1, 5, 20]: two empty layers, then [0,1), [1,5), [5,20)"""
    assert slab_ref.layer_ranges([0, 0, 1, 5, 20], 20) == [(0, 0), (0, 0), (0, 1), (1, 5), (5, 20)]
    assert slab_ref.layer_ranges([3, 50, -2], 20) == [(0, 3), (3, 20), (20, 0)]          # clipped at both ends


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_cloud_fraction_oracle_against_answers_counted_by_hand(dtype):
    ql = numpy.zeros((1, 8, 8, 20), dtype=dtype)
    ql[0, 0, 0, 0] = 1e-5            # layer [0,1): one column
    ql[0, 0, 1, 0] = numpy.nan       # NaN is not cloudy
    ql[0, 0, 2, 0] = -0.0            # nor is -0.0
    ql[0, 0, 3, 0] = -1e-5           # nor a negative value
    ql[0, 1, 0, 1] = 2e-5            # layer [1,5): columns (1,0), (1,1) [twice: counted once], (2,2)
    ql[0, 1, 1, 2] = 2e-5
    ql[0, 1, 1, 4] = 3e-5
    ql[0, 2, 2, 4] = 1e-6
    ql[0, 7, 7, 19] = 1e-4           # layer [5,20): columns (7,7), (1,0)
    ql[0, 1, 0, 5] = 1e-4
    idx = numpy.array([[0, 0, 1, 5, 20]], dtype=numpy.int32)
    want = numpy.array([[0, 0, 1, 3, 2]], dtype=dtype) / dtype(64)
    assert numpy.array_equal(slab_ref.cloud_fraction(ql, idx), want)
    # an index beyond ktot is clipped; a non-monotone map gives an empty layer (0) and the next one starts where it says
    idx2 = numpy.array([[1, 99, 5, 20, 20]], dtype=numpy.int32)      # [0,1) [1,20) [20,5)=empty [5,20) [20,20)=empty
    want2 = numpy.array([[1, 4, 0, 2, 0]], dtype=dtype) / dtype(64)
    assert numpy.array_equal(slab_ref.cloud_fraction(ql, idx2), want2)


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", [(64, 64, 160), (8, 8, 20), (5, 7, 33), (64, 64, 512)])
def test_numpy_mean_is_the_sequential_sum_and_one_division(shape, dtype):
    """the order k_slab_means copies: NOT the pairwise sum of ndarray.sum() over a contiguous run.  If a NumPy upgrade
    changes it, this test says so."""
    rng = numpy.random.default_rng(7)
    f = (rng.standard_normal(shape) * 3 + 1).astype(dtype)
    assert numpy.array_equal(f.mean(axis=(0, 1)), slab_ref.sequential_mean(f))
    if shape[0] * shape[1] > 128:    # and the two orders do differ on such data: the GPU test can tell them apart
        pairwise = numpy.array([numpy.ascontiguousarray(f[:, :, k]).sum() for k in range(shape[2])], dtype=dtype) / dtype(shape[0] * shape[1])
        assert not numpy.array_equal(pairwise, slab_ref.sequential_mean(f))
    z = numpy.full((4, 4, 5), -0.0, dtype=dtype)                    # the reduction starts from +0.0
    assert not numpy.signbit(z.mean(axis=(0, 1))).any()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_numpy_mean_of_one_level_is_the_pairwise_sum(dtype):
    """ktot == 1 makes the plane one contiguous run, which numpy reduces as ndarray.sum() does (k_slab_means_k1)"""
    rng = numpy.random.default_rng(8)
    f = rng.standard_normal((100, 100, 1)).astype(dtype)
    assert numpy.array_equal(f.mean(axis=(0, 1)), numpy.array([f.ravel().sum() / dtype(10000)], dtype=dtype))
    assert not numpy.array_equal(f.mean(axis=(0, 1)), slab_ref.sequential_mean(f))


def test_slab_entry_points_validate_on_the_host(lib):
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    assert lib.spc_abi_version() == 4
    for sfx in ("f64", "f32"):
        means = getattr(lib, "spc_slab_means_" + sfx)
        cloud = getattr(lib, "spc_slab_cloud_fraction_" + sfx)
        assert means(None, None) == E and b"NULL" in lib.spc_last_error()
        assert cloud(None, None) == E and b"NULL" in lib.spc_last_error()

        def m(n=4, itot=8, jtot=8, ktot=20, nf=2, pitch=20, ptr=64):
            a = _abi.SlabMeansArgs()
            a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.pitch_out = n, itot, jtot, ktot, nf, pitch
            for f in range(max(0, min(nf, _abi.SLAB_MAX_FIELDS))):
                a.fields[f], a.out[f] = ptr, ptr
            return ctypes.byref(a)
        assert means(m(ptr=None), None) == E and b"NULL" in lib.spc_last_error()
        assert means(m(n=-1), None) == E
        for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
            assert means(m(**bad), None) == E and b">= 1" in lib.spc_last_error()
        assert means(m(pitch=19), None) == E and b"pitch" in lib.spc_last_error()
        for nf in (0, -1, _abi.SLAB_MAX_FIELDS + 1):
            assert means(m(nf=nf), None) == E and b"field count" in lib.spc_last_error()
        assert means(m(n=0, ptr=None), None) == 0                         # an empty ensemble is a no-op

        def c(n=4, itot=8, jtot=8, ktot=20, nG=5, pitch_idx=5, pitch_out=5, ptr=64):
            a = _abi.SlabCloudArgs(n, itot, jtot, ktot, nG, ptr, ptr, ptr, pitch_idx, pitch_out)
            return ctypes.byref(a)
        assert cloud(c(ptr=None), None) == E and b"NULL" in lib.spc_last_error()
        assert cloud(c(n=-2), None) == E
        assert cloud(c(ktot=0), None) == E and b">= 1" in lib.spc_last_error()
        assert cloud(c(nG=0), None) == E and b"nG" in lib.spc_last_error()
        assert cloud(c(pitch_idx=4), None) == E and b"pitch" in lib.spc_last_error()
        assert cloud(c(pitch_out=4), None) == E and b"pitch" in lib.spc_last_error()
        assert cloud(c(n=0, ptr=None), None) == 0


def test_struct_layout_of_the_slab_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    probes = [("spc_slab_means_args", _abi.SlabMeansArgs, ["n_les", "itot", "ktot", "n_fields", "fields", "out", "pitch_out"]),
              ("spc_slab_cloud_args", _abi.SlabCloudArgs, ["n_les", "jtot", "nG", "ql", "idx", "out", "pitch_idx", "pitch_out"])]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){']
    want = []
    for cname, cls, fields in probes:
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(cls))
        for f in fields:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
            want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


def test_device_ensemble_class_and_protocol_flag():
    from sp_coupler_amd import models
    assert issubclass(models.DeviceLESEnsemble, models.SyntheticLESEnsemble)
    assert models.DeviceLESEnsemble.fields_on_device is True and models.DeviceLESEnsemble.batched is True
    assert not getattr(models.SyntheticLESEnsemble, "fields_on_device", False)
