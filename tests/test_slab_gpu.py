"""K10 on the MI355X: Engine.slab_means against numpy.mean(axis=(0, 1)) and Engine.slab_cloud_fraction against the oracle of
tests/slab_ref.py.  Every comparison asks for equal bits (numpy.array_equal; where NaN occur, gpu_util.assert_bits: equal
values, NaN at the same places, equal sign of zero)."""
import numpy
import pytest
import torch

from sp_coupler_amd import synthetic
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import slab_edges, slab_ref
from tests.gpu_util import assert_bits

pytestmark = pytest.mark.gpu

NP = {torch.float64: numpy.float64, torch.float32: numpy.float32}
SMALL = [(8, 8, 20), (5, 7, 33), (3, 129, 1), (1, 1, 160)]
BIG = [(64, 64, 160), (64, 64, 512)]
CASES = ([(s, n, F) for s in SMALL for n in (1, 2, 37) for F in (1, 3, 8)]
         + [(s, n, F) for s in BIG for n, F in ((1, 8), (2, 3), (37, 1))])


def _fields(shape, n, F, dtype, seed=0):
    """F host fields [n x shape] derived from one random draw (different values per field, cheap to make)"""
    rng = numpy.random.default_rng(seed)
    base = rng.standard_normal((n,) + shape, dtype=numpy.float32).astype(dtype)
    return {"f%d" % j: (base * dtype(1 + 0.37 * j) + dtype(j)) if j else base for j in range(F)}


def _dev(eng, a):
    return torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape,n,F", CASES)
def test_slab_means_equal_numpy_mean(shape, n, F, dtype):
    eng = Engine("cuda:0", dtype=dtype)
    host = _fields(shape, n, F, NP[dtype], seed=n + F)
    got = eng.slab_means({k: _dev(eng, v) for k, v in host.items()})
    assert list(got) == list(host)
    for k, v in host.items():
        g = got[k].cpu().numpy()
        assert g.dtype == NP[dtype] and g.shape == (n, shape[2])
        assert numpy.array_equal(g, slab_ref.slab_means(v)), (k, shape, n, F)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("pad", [3, 4])
def test_slab_means_into_a_pitched_out(dtype, pad):
    """rows of a wider buffer: pad 4 keeps every row 16-byte aligned (the wide-access kernel), pad 3 does not (the scalar one)"""
    eng = Engine("cuda:0", dtype=dtype)
    shape, n = (16, 16, 160), 5
    host = _fields(shape, n, 3, NP[dtype], seed=9)
    wide = {k: torch.full((n, shape[2] + pad), -7.0, dtype=dtype, device=eng.device) for k in host}
    got = eng.slab_means({k: _dev(eng, v) for k, v in host.items()}, out={k: w[:, :shape[2]] for k, w in wide.items()})
    for k, v in host.items():
        assert got[k].data_ptr() == wide[k].data_ptr()
        w = wide[k].cpu().numpy()
        assert numpy.array_equal(w[:, :shape[2]], slab_ref.slab_means(v)) and (w[:, shape[2]:] == -7.0).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_slab_means_of_special_values(dtype):
    """inf, NaN (given and made by inf - inf), planes of -0.0, denormals, and magnitudes that make the summation order visible"""
    dt = NP[dtype]
    eng = Engine("cuda:0", dtype=dtype)
    rng = numpy.random.default_rng(5)
    f = rng.standard_normal((3, 16, 16, 20)).astype(dt)
    tiny = numpy.finfo(dt).smallest_subnormal
    f[:, :, :, 0] = -0.0
    f[0, 3, 4, 1] = numpy.inf
    f[0, 3, 4, 2], f[0, 9, 9, 2] = numpy.inf, -numpy.inf
    f[1, 0, 0, 3] = numpy.nan
    f[:, :, :, 4] = tiny * rng.integers(-5000, 5001, (3, 16, 16)).astype(dt)
    f[:, :, :, 5] = 0.0
    f[2, 5, 5, 5] = tiny
    f[:, :, :, 6] *= dt(10.0) ** rng.integers(-6, 7, (3, 16, 16)).astype(dt)
    f[:, :, :, 7] = -f[:, :, :, 6]
    want = slab_ref.slab_means(f)
    assert numpy.isnan(want[0, 2]) and numpy.isnan(want[1, 3]) and numpy.isinf(want[0, 1]) and not numpy.signbit(want[:, 0]).any()
    assert (want[:, 4] != 0).any() and (numpy.abs(want[:, 4]) < numpy.finfo(dt).tiny).all()      # denormal results
    assert_bits("special", eng.slab_means({"f": _dev(eng, f)})["f"].cpu().numpy(), want)


def test_slab_means_of_a_field_larger_than_4_gib():
    """832 LES of 64 x 64 x 160 doubles: 4.36 GB in one field; 32-bit offsets would wrap in the last LES"""
    eng = Engine("cuda:0")
    n, shape = 832, (64, 64, 160)
    assert n * 64 * 64 * 160 * 8 > 2 ** 32
    gen = torch.Generator(device=eng.device).manual_seed(3)
    field = torch.rand((n,) + shape, dtype=torch.float64, device=eng.device, generator=gen)
    got = eng.slab_means({"x": field})["x"]
    for l in (0, n - 2, n - 1):
        assert numpy.array_equal(got[l].cpu().numpy(), field[l].cpu().numpy().mean(axis=(0, 1))), l
    ql = (field < 0.0005).to(torch.float64)                   # sparse "cloud": the same offsets in the cloud-fraction kernel
    idx = torch.tensor([[0, 3, 40, 160, 200]], dtype=torch.int32, device=eng.device).repeat(n, 1)
    A = eng.slab_cloud_fraction(ql, idx)
    for l in (0, n - 1):
        want = slab_ref.cloud_fraction(ql[l:l + 1].cpu().numpy(), idx[l:l + 1].cpu().numpy())
        assert want.max() > 0 and numpy.array_equal(A[l:l + 1].cpu().numpy(), want), l


def test_slab_means_argument_checks():
    eng = Engine("cuda:0")
    f = torch.zeros((2, 4, 4, 8), dtype=torch.float64, device=eng.device)
    with pytest.raises(ValueError):
        eng.slab_means({"a": f, "b": f[:, :, :, ::2]})                       # not contiguous / another shape
    with pytest.raises(ValueError):
        eng.slab_means({"a": f.float()})                                     # not the engine's dtype
    with pytest.raises(ValueError):
        eng.slab_means({"a": f.cpu()})
    with pytest.raises(ValueError):
        eng.slab_means({})
    with pytest.raises(ValueError):
        eng.slab_cloud_fraction(f, torch.zeros((2, 5), dtype=torch.int64, device=eng.device))
    assert eng.slab_means({"a": f[:0]})["a"].shape == (0, 8)                 # an empty ensemble: no launch


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_cloud_fraction_hand_counted_cases(dtype):
    eng = Engine("cuda:0", dtype=dtype)
    ql, idx, counts = slab_ref.hand_case(NP[dtype])
    ql2 = numpy.concatenate([ql, ql])                                         # the same field under both index maps
    want = counts.astype(NP[dtype]) / NP[dtype](64)
    assert numpy.array_equal(slab_ref.cloud_fraction(ql2, idx), want)
    got = eng.slab_cloud_fraction(_dev(eng, ql2), _dev(eng, idx))
    assert numpy.array_equal(got.cpu().numpy(), want)
    # pitched idx and out
    idx_w = torch.zeros((2, 9), dtype=torch.int32, device=eng.device)
    idx_w[:, :5] = _dev(eng, idx)
    out_w = torch.full((2, 8), -1.0, dtype=dtype, device=eng.device)
    eng.slab_cloud_fraction(_dev(eng, ql2), idx_w[:, :5], out=out_w[:, :5])
    assert numpy.array_equal(out_w.cpu().numpy()[:, :5], want) and (out_w.cpu().numpy()[:, 5:] == -1.0).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("nG,nL", [(91, 160), (137, 512)])
def test_cloud_fraction_random_sparse_ql_with_the_index_map_of_k2(nG, nL, dtype):
    eng = Engine("cuda:0", dtype=dtype)
    n, itot, jtot = 6, 24, 20
    gcm, zf, zh, prof = synthetic.make_batch(n, nG, nL, seed=11)
    dev = lambda d: {k: _dev(eng, v).to(dtype) for k, v in d.items()}                     # noqa: E731
    fwd = eng.forward(dev(gcm), _dev(eng, zf).to(dtype), dev(prof), 1.0, 900.0, zh=_dev(eng, zh).to(dtype), want_profiles=True)
    idx = eng.cloud_indices(_dev(eng, zh).to(dtype), fwd["Zh"])
    assert torch.equal(idx, fwd["idx"])
    rng = numpy.random.default_rng(12)
    ql = numpy.where(rng.random((n, itot, jtot, nL)) < 0.03, rng.random((n, itot, jtot, nL)) * 1e-3, 0.0).astype(NP[dtype])
    want = slab_ref.cloud_fraction(ql, idx.cpu().numpy())
    assert 0 < want.max() <= 1 and (want == 0).any()
    got = eng.slab_cloud_fraction(_dev(eng, ql), idx)
    assert numpy.array_equal(got.cpu().numpy(), want)


def test_two_engines_on_one_card_equal_one_engine():
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")), Engine("cuda:0", stream=torch.cuda.Stream("cuda:0"))],
                              min_cols_per_device=1)
    n, shape = 7, (12, 10, 40)
    host = _fields(shape, n, 3, numpy.float64, seed=21)
    ql = numpy.where(host["f0"] > 1.5, host["f0"], 0.0)
    idx = numpy.tile(numpy.array([0, 2, 2, 9, 25, 40, 44], dtype=numpy.int32), (n, 1))
    want = one.slab_means({k: _dev(one, v) for k, v in host.items()})
    want_A = one.slab_cloud_fraction(_dev(one, ql), _dev(one, idx))
    sh = {k: multi.to_devices(v, rows=n) for k, v in host.items()}
    assert len(sh["f0"].parts) == 2 and sh["f0"].parts[0].shape[0] in (3, 4)
    got = multi.slab_means(sh)
    got_A = multi.slab_cloud_fraction(multi.to_devices(ql, rows=n), multi.to_devices(idx, rows=n, dtype=torch.int32))
    multi.synchronize()
    for k in host:
        assert numpy.array_equal(got[k].to_host(), want[k].cpu().numpy()) and numpy.array_equal(got[k].to_host(), slab_ref.slab_means(host[k]))
    assert numpy.array_equal(got_A.to_host(), want_A.cpu().numpy()) and numpy.array_equal(got_A.to_host(), slab_ref.cloud_fraction(ql, idx))


# -- the edges of the kernels (tests/slab_edges.py holds the inputs and the bodies; tests/test_slab_cpu.py states that the
#    oracle's answers to these inputs are not trivial; tools/mutation_control.py shows that wrong kernels fail them) ----------
@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
@pytest.mark.parametrize("kind", slab_edges.QL_KINDS)
@pytest.mark.parametrize("plane", slab_edges.PLANES)
def test_cloud_fraction_with_fewer_rows_left_than_a_wave_takes(plane, kind, dtype):
    slab_edges.check_cloud_plane(Engine("cuda:0", dtype=dtype), plane, kind)


@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
@pytest.mark.parametrize("ktot", slab_edges.KTOTS)
@pytest.mark.parametrize("nG", slab_edges.NGS)
def test_cloud_fraction_layer_counts_level_counts_and_word_boundaries(nG, ktot, dtype):
    slab_edges.check_cloud_layers(Engine("cuda:0", dtype=dtype), nG, ktot)


@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
def test_cloud_fraction_with_opt_in_lds(dtype):
    slab_edges.check_cloud_opt_in_lds(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
def test_cloud_fraction_refuses_more_lds_than_the_device_has(dtype):
    slab_edges.check_cloud_lds_refusal(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
@pytest.mark.parametrize("ktot", slab_edges.MEANS_KTOTS)
@pytest.mark.parametrize("plane", slab_edges.PLANES)
def test_slab_means_of_every_remainder_of_rows(plane, ktot, dtype):
    slab_edges.check_means_plane(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
@pytest.mark.parametrize("lead,lead_out", [(1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (3, 3)])
def test_slab_means_from_and_into_views_off_the_16_byte_grid(lead, lead_out, dtype):
    slab_edges.check_means_unaligned_base(Engine("cuda:0", dtype=dtype), lead, lead_out)


@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
@pytest.mark.parametrize("n", [1, 3, 129, 300])
@pytest.mark.parametrize("ktot", [2, 4, 8, 16])
def test_slab_means_with_few_lanes_per_les_and_idle_lanes(ktot, n, dtype):
    slab_edges.check_means_lanes(Engine("cuda:0", dtype=dtype), ktot, n)


@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
def test_slab_means_of_sixteen_fields_and_not_seventeen(dtype):
    slab_edges.check_means_field_count(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
@pytest.mark.parametrize("size", slab_edges.K1_SIZES)
def test_slab_means_of_one_level_at_the_pairwise_block_sizes(size, dtype):
    slab_edges.check_means_k1(Engine("cuda:0", dtype=dtype), size)


@pytest.mark.parametrize("dtype", slab_edges.DTYPES)
def test_the_chain_cases(dtype):
    """the cases of the lane's walk that spc_chain.hpp's kernels share, held together (slab_edges.check_chain)"""
    slab_edges.check_chain(Engine("cuda:0", dtype=dtype))
