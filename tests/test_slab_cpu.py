"""K10 without a GPU: the NumPy oracle of tests/slab_ref.py against answers counted by hand, the summation order of
numpy.mean that k_slab_means copies, and the host-side argument checks of the four entry points."""
import ctypes

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi
from tests import slab_edges, slab_ref


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


# -- the inputs of the edge tests of tests/test_slab_gpu.py (tests/slab_edges.py): what they cover, and that the oracle's
#    answer to each is one a wrong kernel would miss ------------------------------------------------------------------------
def test_edge_inputs_cover_what_they_claim():
    nij = [i * j for i, j in slab_edges.PLANES]
    assert {x % 4 for x in nij} == set(range(4)) and {x % 8 for x in nij} == set(range(8))
    assert {1, 2, 3, 4, 5, 6, 7} <= set(nij) and any(256 < x < 260 for x in nij) and 260 in nij and 255 in nij
    assert set(slab_edges.NGS) >= {1, 5, 63, 64, 65, 257, 600} and set(slab_edges.KTOTS) >= {1, 7, 63, 64, 65, 128, 130, 512}
    assert set(slab_edges.K1_SIZES) >= {1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 8191, 8192, 8193, 20000}
    for ktot in slab_edges.KTOTS:                              # the layer bounds the index maps put on the word boundaries
        idx = slab_edges.index_map(600, ktot, 1)
        ranges = set(slab_ref.layer_ranges(idx[0], ktot)) | set(slab_ref.layer_ranges(idx[1], ktot))
        for b in (63, 64, 65, 127, 128):
            if b < ktot:
                assert any(hi == b and lo < hi for lo, hi in ranges) and any(lo == b and lo < hi for lo, hi in ranges), (ktot, b)
        assert any(hi == ktot and lo < hi for lo, hi in ranges)
        if ktot >= 128:
            assert (64, 128) in ranges and (0, 64) in ranges
        assert (idx < 0).any() and (idx > ktot).any() and (numpy.diff(idx, axis=1) < 0).any() and (numpy.diff(idx, axis=1) == 0).any()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("plane", slab_edges.PLANES)
def test_edge_planes_have_answers_a_miscounted_row_changes(plane, dtype):
    nij = plane[0] * plane[1]
    ql, idx = slab_edges.plane_case(plane, "all", dtype)
    want = slab_ref.cloud_fraction(ql, idx)
    full = numpy.array([[hi > lo for lo, hi in slab_ref.layer_ranges(r, ql.shape[-1])] for r in idx])
    assert full.any() and not full.all() and (want[full] == 1).all() and (want[~full] == 0).all()      # exactly 1: a row twice is > 1
    ql, idx = slab_edges.plane_case(plane, "last", dtype)
    want = slab_ref.cloud_fraction(ql, idx)
    assert numpy.count_nonzero(want) == 3 and (want[want != 0] == dtype(1) / dtype(nij)).all()          # one column of one layer per LES
    ql, idx = slab_edges.plane_case(plane, "sparse", dtype)
    want = slab_ref.cloud_fraction(ql, idx)
    assert (want == 0).any() and want.max() <= 1
    if nij >= 35:
        assert ((want > 0) & (want < 1)).any()


@pytest.mark.parametrize("ktot", slab_edges.KTOTS)
@pytest.mark.parametrize("nG", slab_edges.NGS)
def test_edge_layer_maps_have_answers_of_every_kind(nG, ktot):
    ql, idx = slab_edges.layers_case(nG, ktot, numpy.float64)
    want = slab_ref.cloud_fraction(ql, idx)
    assert want.shape == (2, nG) and want.max() > 0 and want.max() <= 1
    if nG >= 5:
        assert (want == 0).any() and ((want > 0) & (want < 1)).any()
    if nG > 256:
        assert want[:, 256:].max() > 0                          # a layer of the second trip of the per-layer loops counts something
    if nG > 520:
        assert want[:, 512:].max() > 0
    # the two hand-set columns make the levels next to a boundary matter: moving a bound by one level changes the answer
    for shift in (-1, 1):
        moved = numpy.where((idx > 0) & (idx < ktot), idx + shift, idx).astype(numpy.int32)
        if nG >= 63 and ktot >= 63:
            assert not numpy.array_equal(slab_ref.cloud_fraction(ql, moved), want), shift


def test_edge_lds_case_and_its_refusal(lib):
    for dtype in (numpy.float64, numpy.float32):
        ql, idx, counts = slab_edges.lds_case(dtype)
        assert numpy.array_equal(slab_ref.cloud_fraction(ql, idx), counts.astype(dtype) / dtype(6)) and counts.max() == 2
    assert 4 * 4 * (32768 // 64) * 8 + 5 * 8 + 4 * 5 * 4 > 64 * 1024                # masks + bounds + counters: above the default limit
    assert 4 * 4 * (65536 // 64) * 8 + 2048 * 8 + 4 * 2048 * 4 == 180224 > 160 * 1024
    for sfx in ("f64", "f32"):                                                      # the host check needs no device
        a = _abi.SlabCloudArgs(1, 2, 3, 65536, 2048, 64, 64, 64, 2048, 2048)
        assert getattr(lib, "spc_slab_cloud_fraction_" + sfx)(ctypes.byref(a), None) == _abi.SPC_ERR_UNSUPPORTED
        assert b"slab_cloud_fraction needs 180224 B of LDS per workgroup (gfx950 has 163840)" in lib.spc_last_error()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_edge_one_level_planes_tell_pairwise_from_sequential(dtype):
    differ = []
    for size in slab_edges.K1_SIZES:
        f = slab_edges.k1_field(size, dtype)
        want = slab_ref.slab_means(f)
        assert want.shape == (3, 1) and numpy.array_equal(want[:, 0], [x.ravel().sum() / dtype(size) for x in f])
        if not numpy.array_equal(want, numpy.stack([slab_ref.sequential_mean(x.reshape(size, 1, 1)) for x in f])):
            differ.append(size)
    assert differ and max(differ) > 8192 and min(differ) <= 257, differ


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_edge_means_notice_a_dropped_row(dtype):
    """the fields of the remainder tests: leaving out the last row of a plane changes every mean"""
    for plane in slab_edges.PLANES:
        f = slab_edges.means_fields(plane + (33,), 3, 2, dtype, seed=1)["f1"]
        rows = f.reshape(3, -1, 33)
        if rows.shape[1] > 1:
            short = numpy.stack([slab_ref.sequential_mean(r[:-1, None, :]) * dtype(rows.shape[1] - 1) / dtype(rows.shape[1]) for r in rows])
            assert (short != slab_ref.slab_means(f)).all(), plane



def test_the_chain_cases_on_the_oracle_backed_engine():
    """the oracle alone handles every case of the chain body, none skipped; its plumbing runs without a GPU"""
    from tests.fake_engine import OracleEngine
    slab_edges.check_chain(OracleEngine())
    assert "chain" in slab_edges.BODIES and len(list(slab_edges.chain_cases(8, numpy.float64))) == 17 * 3 + 2
