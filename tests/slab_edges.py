"""K10 at the edges of its kernels (sp_coupler_amd/csrc/spc_slab.hpp): the inputs as NumPy arrays (tests/test_slab_cpu.py
states on the CPU that the oracle's answer to each of them is not trivial) and the bodies of the GPU tests, each taking an
engine (tests/test_slab_gpu.py hands them Engine("cuda:0", dtype); tools/mutation_control.py hands them the engines of its
mutant libraries).  Every comparison asks for equal bits against slab_ref.slab_means (numpy.mean) / slab_ref.cloud_fraction.

Every device field is the LEADING part of a larger buffer whose tail is poison (a positive value for QL, NaN for the fields of
the means): a kernel that reads past the last row of the last LES reads the test's own buffer and changes a count or a mean."""
import numpy
import torch

from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (NP, DTYPES, TAIL_ROWS, with_tail: K10's own tests)
    DTYPES, NP, TAIL_ROWS, chain_cases, np_of as _np, run_bodies, with_tail)


#: itot x jtot: every residue of nij mod 4 (SLAB_CF_RB rows per wave) and mod 8 (SLAB_U rows of loads in flight), below and
#: above one workgroup's 256 rows (260: a second workgroup with 4 rows; 257: one with a single row), nij < 8, nij == 1
PLANES = [(1, 1), (2, 1), (1, 3), (2, 2), (1, 5), (2, 3), (1, 7), (3, 3), (4, 4), (5, 7), (17, 15), (13, 20), (257, 1), (37, 41)]
QL_KINDS = ("sparse", "all", "last")
NGS = (1, 5, 63, 64, 65, 257, 600)
KTOTS = (1, 7, 63, 64, 65, 128, 130, 512)
K1_SIZES = (1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 8191, 8192, 8193, 20000)


# -- inputs (NumPy) --------------------------------------------------------------------------------------------------------
def plane_case(plane, kind, dtype, n=3, ktot=70):
    """QL [n x plane x ktot] and an index map with empty layers, a negative entry, an entry beyond ktot and a layer that ends
    on the 64-level word boundary.  kind "sparse": random cloud; "all": cloudy at every point (A == 1 exactly in every layer
    that holds a level); "last": exactly one cloudy point, in the last row of every LES (the last row of the last workgroup)"""
    itot, jtot = plane
    rng = numpy.random.default_rng(1000 * itot + jtot)
    shape = (n, itot, jtot, ktot)
    if kind == "sparse":
        ql = numpy.where(rng.random(shape) < 0.02, rng.random(shape) * 1e-3 + 1e-9, 0.0)
    elif kind == "all":
        ql = rng.random(shape) * 1e-3 + 1e-9
    else:
        ql = numpy.zeros(shape)
        ql[:, -1, -1, ktot - 1] = 1e-4
    idx = numpy.tile(numpy.array([0, 3, 3, 40, 64, 70, 99], dtype=numpy.int32), (n, 1))      # [0,0) [0,3) [3,3) [3,40) [40,64) [64,70) [70,70)
    idx[1] = [-2, 1, 64, 65, 69, 70, 70]                                                      # [0,0) [0,1) [1,64) [64,65) [65,69) [69,70) [70,70)
    return ql.astype(dtype), idx


def index_map(nG, ktot, seed):
    """two index maps [2 x nG] whose layer bounds fall on 0, 63, 64, 65, 127, 128 and ktot (as far as ktot reaches): a layer
    that starts on a word boundary, one that ends on it, one that does both ([64, 128)), single-level layers on either side;
    then a negative entry, a decreasing step, a run of equal entries, and sorted random entries up to beyond ktot"""
    rng = numpy.random.default_rng(seed)
    rows = []
    for core in ([0, 63, 64, 65, 127, 128, ktot], [64, 128, ktot, -3, 1]):
        core = [b for b in core if b <= ktot]
        fill = [-2, ktot // 2, ktot // 2, ktot // 2, -1, 3] + sorted(int(x) for x in rng.integers(0, ktot + 4, nG))
        rows.append((core + fill)[:nG])
    if nG > 256:                       # layers above r = 256 (the second trip of the per-layer loops) that hold every level
        rows[0][nG - 2:] = [0, ktot]
        rows[1][nG - 2:] = [-1, ktot + 1]
    if nG > 520:                       # and the third trip
        rows[0][515:517] = [0, ktot]
    return numpy.array(rows, dtype=numpy.int32)


def layers_case(nG, ktot, dtype, plane=(5, 7)):
    """random sparse QL on a plane of 35 rows (35 % 4 == 3) under index_map(nG, ktot); two columns are set by hand: (0, 0) is
    cloudy exactly at the last level below each boundary, (1, 1) exactly at the first level above it"""
    rng = numpy.random.default_rng(7 * nG + ktot)
    shape = (2,) + plane + (ktot,)
    ql = numpy.where(rng.random(shape) < max(0.04, 1.0 / ktot) / 2, 1e-4, 0.0)
    ql[:, 0, 0, :] = 0.0
    ql[:, 1, 1, :] = 0.0
    for b in (63, 64, 65, 127, 128, ktot):
        if 1 <= b <= ktot:
            ql[:, 0, 0, b - 1] = 2e-4
        if b < ktot:
            ql[:, 1, 1, b] = 3e-4
    return ql.astype(dtype), index_map(nG, ktot, 31 * nG + ktot)


def lds_case(dtype, ktot=32768, nG=5):
    """a 2 x 3 plane of 32 768 levels: 64 KiB of row masks alone, so the kernel needs the opt-in LDS limit"""
    ql = numpy.zeros((2, 2, 3, ktot), dtype=dtype)
    ql[0, 0, 0, 0] = ql[0, 1, 2, 64] = ql[0, 1, 1, ktot - 1] = ql[1, 0, 1, 20000] = ql[1, 1, 0, 20000] = 1e-4
    idx = numpy.array([[1, 64, 65, 20000, ktot], [0, 20000, 20001, ktot - 1, ktot + 7]], dtype=numpy.int32)[:, :nG]
    counts = numpy.array([[1, 0, 1, 0, 1], [0, 0, 2, 0, 0]])
    return ql, idx, counts


def means_fields(shape, n, F, dtype, seed):
    rng = numpy.random.default_rng(seed)
    base = (rng.standard_normal((n,) + tuple(shape)) * 3 + 1).astype(dtype)
    return {"f%d" % j: (base * dtype(1 + 0.37 * j) + dtype(j)) if j else base for j in range(F)}


def k1_field(size, dtype, n=3):
    rng = numpy.random.default_rng(size)
    return (rng.standard_normal((n, size, 1, 1)) * 3 + 1).astype(dtype)


# -- device plumbing -------------------------------------------------------------------------------------------------------
def run_cloud(eng, ql, idx):
    q, qbuf = with_tail(eng, ql, 1.0)
    i, _ = with_tail(eng, idx, int(ql.shape[-1]), tail_elems=max(256, idx.shape[1]))
    out, obuf = with_tail(eng, numpy.full(idx.shape, -1.0, dtype=ql.dtype), -7.0, tail_elems=64)
    got = eng.slab_cloud_fraction(q, i, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert (obuf[out.numel():] == -7.0).all() and (qbuf[q.numel():] == 1.0).all()
    return got.cpu().numpy()


def run_means(eng, fields, lead=0, lead_out=0):
    dev = {k: with_tail(eng, v, float("nan"), lead=lead)[0] for k, v in fields.items()}
    n, ktot = next(iter(fields.values())).shape[0], next(iter(fields.values())).shape[-1]
    outs = {k: with_tail(eng, numpy.full((n, ktot), -1.0, dtype=v.dtype), -7.0, lead=lead_out, tail_elems=64) for k, v in fields.items()}
    got = eng.slab_means(dev, out={k: o[0] for k, o in outs.items()})
    for k, (o, buf) in outs.items():
        assert got[k].data_ptr() == o.data_ptr()
        assert (buf[:lead_out] == -7.0).all() and (buf[lead_out + o.numel():] == -7.0).all(), k      # nothing written around out
    return {k: v.cpu().numpy() for k, v in got.items()}


# -- bodies ----------------------------------------------------------------------------------------------------------------
def check_cloud_plane(eng, plane, kind):
    """items 5 and 8: fewer than SLAB_CF_RB rows left for a wave; all-cloudy planes; one cloudy point in the last row"""
    ql, idx = plane_case(plane, kind, _np(eng))
    want = slab_ref.cloud_fraction(ql, idx)
    got = run_cloud(eng, ql, idx)
    assert numpy.array_equal(got, want), (plane, kind, got, want)


def check_cloud_layers(eng, nG, ktot):
    """items 6 and 7: the strides of the per-layer loops, partial and whole 64-level words, bounds on the word boundaries,
    negative entries, decreasing steps"""
    ql, idx = layers_case(nG, ktot, _np(eng))
    want = slab_ref.cloud_fraction(ql, idx)
    got = run_cloud(eng, ql, idx)
    assert numpy.array_equal(got, want), (nG, ktot, numpy.argwhere(got != want)[:5])


def check_cloud_opt_in_lds(eng):
    """item 9: above 64 KiB of LDS the kernel runs with the raised limit"""
    ql, idx, counts = lds_case(_np(eng))
    want = counts.astype(_np(eng)) / _np(eng)(6)
    assert numpy.array_equal(slab_ref.cloud_fraction(ql, idx), want)
    assert numpy.array_equal(run_cloud(eng, ql, idx), want)


def check_cloud_lds_refusal(eng):
    """item 9: 65 536 levels and 2 048 layers need 180 224 B of LDS: refused by the host check, nothing launched"""
    from sp_coupler_amd import _abi
    ktot, nG = 65536, 2048
    ql = torch.zeros((1, 2, 3, ktot), dtype=eng.dtype, device=eng.device)
    idx = torch.zeros((1, nG), dtype=torch.int32, device=eng.device)
    out = torch.full((1, nG), -1.0, dtype=eng.dtype, device=eng.device)
    try:
        eng.slab_cloud_fraction(ql, idx, out=out)
    except _abi.SpcError as e:
        assert e.code == _abi.SPC_ERR_UNSUPPORTED and not isinstance(e, ValueError), e
        assert "slab_cloud_fraction needs 180224 B of LDS per workgroup (gfx950 has 163840)" in str(e), e
    else:
        raise AssertionError("180 224 B of LDS were not refused")
    torch.cuda.synchronize(eng.device)
    assert (out == -1.0).all()


def check_means_plane(eng, plane, ktot):
    """item 10: every remainder nij % SLAB_U, nij < 8 and nij == 1; ktot picks the instantiation (160: wide; 33: scalar by
    its pitch; 2 / 4: wide with one lane per LES; 8: wide with a wave spanning several LES)"""
    fields = means_fields(plane + (ktot,), 3, 2, _np(eng), seed=plane[0] * 100 + plane[1] + ktot)
    got = run_means(eng, fields)
    for k, v in fields.items():
        assert numpy.array_equal(got[k], slab_ref.slab_means(v)), (plane, ktot, k)


def check_means_unaligned_base(eng, lead, lead_out):
    """item 10: ktot and the pitch allow 16-byte accesses, the base pointer of a field (``lead`` elements into its buffer) or
    of out (``lead_out``) does not: the scalar instantiation must be chosen"""
    fields = means_fields((5, 7, 160), 4, 3, _np(eng), seed=lead + 10 * lead_out)
    got = run_means(eng, fields, lead=lead, lead_out=lead_out)
    for k, v in fields.items():
        assert numpy.array_equal(got[k], slab_ref.slab_means(v)), (lead, lead_out, k)


def check_means_lanes(eng, ktot, n):
    """item 10: the wide instantiation with ktot == V (one lane per LES) and ktot < 64 V (a wave spans several LES); n picks a
    last workgroup that is partly idle (chains % 256 != 0) or a single partly idle workgroup"""
    fields = means_fields((5, 7, ktot), n, 2, _np(eng), seed=ktot + n)
    got = run_means(eng, fields)
    for k, v in fields.items():
        assert numpy.array_equal(got[k], slab_ref.slab_means(v)), (ktot, n, k)


def check_means_field_count(eng):
    """item 10: 16 fields in one launch, 17 refused"""
    from sp_coupler_amd import _abi
    assert _abi.SLAB_MAX_FIELDS == 16
    fields = means_fields((3, 5, 20), 3, 17, _np(eng), seed=16)
    sixteen = {k: fields[k] for k in list(fields)[:16]}
    got = run_means(eng, sixteen)
    assert list(got) == list(sixteen)
    for k, v in sixteen.items():
        assert numpy.array_equal(got[k], slab_ref.slab_means(v)), k
    try:
        eng.slab_means({k: torch.from_numpy(v).to(eng.device) for k, v in fields.items()})
    except ValueError as e:
        assert "16" in str(e)
    else:
        raise AssertionError("17 fields were not refused")


def check_means_k1(eng, size):
    """item 11: ktot == 1, planes on both sides of the block sizes of numpy's pairwise sum (8, 128, 8192)"""
    f = k1_field(size, _np(eng))
    want = slab_ref.slab_means(f)
    got = run_means(eng, {"f": f})["f"]
    assert_bits("k1 %d" % size, got, want)
    f2 = f.reshape(f.shape[0], 1, size, 1)                       # the same run as one row of the plane
    assert numpy.array_equal(run_means(eng, {"f": f2})["f"], want)


def check_chain(eng):
    """the cases of the lane's walk (les_harness.chain_cases) for the 8 rows a lane has in flight, the fields and the means in
    poison (run_means)"""
    for shape, lead in chain_cases(8, _np(eng)):
        fields = means_fields(shape[1:], shape[0], 2, _np(eng), seed=900 + shape[2] + shape[3] + lead)
        got = run_means(eng, fields, lead=lead, lead_out=lead)
        for k, v in fields.items():
            assert_bits("chain %s lead %d %s" % (shape, lead, k), got[k], slab_ref.slab_means(v))


MEANS_KTOTS = (160, 33, 2, 4, 8)


BODIES = ("cloud_plane", "cloud_layers", "cloud_opt_in_lds", "means_plane", "means_k1", "chain")


def jobs(eng):
    return [("cloud_plane", lambda: [check_cloud_plane(eng, p, k) for p in PLANES for k in QL_KINDS]),
            ("cloud_layers", lambda: [check_cloud_layers(eng, g, k) for g in NGS for k in KTOTS]),
            ("cloud_opt_in_lds", lambda: check_cloud_opt_in_lds(eng)),
            ("means_plane", lambda: [check_means_plane(eng, p, k) for p in PLANES for k in MEANS_KTOTS]),
            ("means_k1", lambda: [check_means_k1(eng, s) for s in K1_SIZES]),
            ("chain", lambda: check_chain(eng))]


def check_everything(eng):
    """the bodies BODIES on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the names of the
    bodies that failed (AssertionError) in the order they ran."""
    return run_bodies(BODIES, jobs(eng))
