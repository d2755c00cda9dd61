"""The inputs of tests/vnudge_edges.py on the CPU: no kernel runs here.  For every body and dtype the REFERENCE alone
(oracle/vnudge_oracle.py in float64, tests/vnudge_f32_ref.py in float32) must reach what the body claims, with error None: a
generator that stops reaching a branch fails here, it does not pass vacuously on the GPU."""
import numpy
import pytest
import torch

from tests import vnudge_edges as ve

IDS = {torch.float64: "f64", torch.float32: "f32"}
dtypes = pytest.mark.parametrize("dtype", ve.DTYPES, ids=lambda d: IDS[d])


def _refs(body, dtype):
    """[(name, fields, references)] of the body's launches, constantT (the statuses do not depend on it)"""
    out = []
    for n, (name, fs, routes) in enumerate(ve.launches(body, dtype)):
        refs = ve.reference(body, n, dtype, True)
        assert len(refs) == len(fs) and all(r["error"] is None for r in refs), name
        assert len({f["qt"].shape for f in fs}) == 1, name
        out.append((name, fs, refs))
    return out


def _both_finders(st):
    return ((st & 1) != 0).any() and ((st & 4) != 0).any()


def test_leaf_sizes_restate_numpys_split():
    """ve.leaf_sizes against the restated pairwise sum of the oracle, which tests/test_vnudge.py pins to ndarray.sum()"""
    for n in (1, 7, 8, 9, 63, 128, 136, 200, 256, 512, 4096, 8192, 8193, 8200, 8464):
        a = numpy.random.default_rng(n).normal(size=n)
        total, lo = 0.0, 0
        for chunk in ve.leaf_sizes(n):                      # the leaves summed as numpy sums a block, joined left to right:
            sums = []                                       # right for these n, whose trees join neighbours of equal depth
            for m in chunk:
                assert 1 <= m <= 128
                sums.append(ve.vo._leaf(a, lo, m))
                lo += m
            while len(sums) > 1:
                sums = [sums[i] + sums[i + 1] for i in range(0, len(sums), 2)]
            total += sums[0]
        assert lo == n and total == float(a.sum()), n
    assert ve.leaf_sizes(136) == [[64, 72]] and ve.leaf_sizes(200) == [[96, 104]] and ve.leaf_sizes(8193)[1] == [1]


@dtypes
def test_designed_levels_reach_every_branch(dtype):
    assert [pl for pl in ve.DESIGNED_PLANES] == [(9, 7), (2, 3), (1, 1), (1, 8), (3, 3), (64, 64), (92, 92)]
    for (name, fs, refs), (itot, jtot) in zip(_refs("designed_levels", dtype), ve.DESIGNED_PLANES):
        nij, f, r = itot * jtot, fs[0], refs[0]
        dropped = ve.designed_dropped(nij)
        assert len(dropped) <= 3 and (nij > 2 and not dropped or nij <= 2), name
        assert tuple(r["status"]) == ve.designed_status(nij), (name, r["status"])
        if nij == 63:
            assert tuple(r["status"]) == (0, 2, 1, 0, 2, 2, 10, 24, 1, 5, 2, 1)
        dt = ve.NP[dtype]
        assert all(numpy.array_equal(v, v.astype(dt).astype(numpy.float64), equal_nan=True) for v in f.values()), name   # exact in dtype
        assert f["ql_ref"][1] == float(dt(1e-9)) and f["ql_ref"][2] == float(numpy.nextafter(dt(1e-9), dt(1)))
        assert f["ql_av"][3] == f["ql_ref"][3] > 0 and (f["ql"][:, :, 3] > 0).any()
        assert r["beta"][1] > 0 and r["beta"][1] < 1 and r["beta"][5] == 1.0 and r["beta"][6] == 1.0 and r["beta"][7] == 1.0
        assert r["beta"][8] == 0.0 and not numpy.signbit(r["beta"][8]) and r["alpha"][8] == -numpy.inf       # f(0) == 0
        assert 0 < r["beta"][2] < 5 and 0 < r["beta"][11] < 5
        if 9 not in dropped:
            assert r["a"][9] > 0 and r["beta"][9] == 1.0                       # brentq returned 5.0, the noise search ran
        if 4 not in dropped:
            i1, i2 = ve.tie_points(nij)
            d = (f["qt"][:, :, 4] - f["qsat"][:, :, 4]).astype(dt).ravel()
            ties = [i1, i2] + ([i1 + 1] if i1 + 1 < i2 else [])
            assert i1 < i2 and sorted(numpy.nonzero(d == d.max())[0]) == sorted(ties) and int(numpy.argmax(d)) == i1
            assert all(i1 // ve.argmax_segment(nij, TL) != i2 // ve.argmax_segment(nij, TL) for TL in (32, 64, 128, 256, 512))
            q, s, av = f["qt"].reshape(nij, 12)[:, 4], f["qsat"].reshape(nij, 12)[:, 4], f["qt_av"][4]
            beta = [float((dt(s[i]) - dt(av)) / (dt(q[i]) - dt(av))) for i in ties]
            assert r["beta"][4] == beta[0] and len(set(beta)) == len(beta) and all(0 <= b < 5 for b in beta)   # each its own beta
            # 64 x 64 (256 threads per level) and 92 x 92 (512): the first two maxima lie in ONE lane's segment
            for plane, TL in ((4096, 256), (8464, 512)):
                if nij == plane:
                    assert i1 // ve.argmax_segment(nij, TL) == (i1 + 1) // ve.argmax_segment(nij, TL)
        if 10 not in dropped:
            d = (f["qt"][:, :, 10] - f["qsat"][:, :, 10]).ravel()
            assert numpy.isnan(r["beta"][10]) and numpy.isnan(d).sum() == 2 and int(numpy.argmax(d)) == nij - 2
            assert int(numpy.nanargmax(d)) == 0 and numpy.isnan(r["qt"][:, :, 10]).all() and numpy.isnan(r["qt_std"][10])
        assert numpy.array_equal(r["qt"][:, :, 3], f["qt"][:, :, 3].astype(dt))
        for k in (6, 7):              # touched, not applied: qt stays, thl (constantT) is corrected all the same
            assert numpy.array_equal(r["qt"][:, :, k], f["qt"][:, :, k].astype(dt))
            assert not numpy.array_equal(r["thl"][:, :, k], f["thl"][:, :, k].astype(dt))
    # the tie of the 9 x 7 plane: 9 and 54
    assert ve.tie_points(63) == (9, 54)


@dtypes
def test_tall_has_every_kind_of_level_above_256(dtype):
    for name, fs, refs in _refs("tall", dtype):
        st = refs[0]["status"]
        assert len(st) in (300, 513) and len(st) > 256
        for part in (st[:256], st[256:]):
            assert (part == 1).any() and ((part & 4) != 0).any() and (part == 2).any() and (part == 0).any(), name
        assert st[-1] != 0 and st[256] != 0 and st[255] != 0, name              # k = 255, 256 and the last level are active


@dtypes
def test_std_many_workgroups_launch_the_256_row_kernel(dtype):
    shapes = []
    for name, fs, refs in _refs("std_many_workgroups", dtype):
        itot, jtot, ktot = fs[0]["qt"].shape
        wg, rows = ve.std_workgroups(len(fs), ktot)
        assert wg > 256 and rows == 256, (name, wg)
        shapes.append((itot * jtot, -(-itot * jtot // rows), itot * jtot % rows))
        assert any(_both_finders(r["status"]) for r in refs)
        assert all((r["status"] != 0).any() and (r["status"] == 0).sum() >= ktot - 4 for r in refs), name
        assert len({tuple(r["status"]) for r in refs}) == len(refs), name       # every LES has its own pattern
    assert shapes[0] == (256, 1, 0) and shapes[1][1] >= 3 and shapes[1][2] != 0   # one full tile; three tiles, the last ragged
    assert ve.std_workgroups(2, 160) == (20, 512)                                # the largest launch of the old matrix


@dtypes
def test_small_trees_have_the_claimed_leaves(dtype):
    leaves = []
    for name, fs, refs in _refs("small_trees", dtype):
        itot, jtot, _ = fs[0]["qt"].shape
        leaves.append(ve.leaf_sizes(itot * jtot))
        assert _both_finders(refs[0]["status"]) and (refs[0]["status"] == 2).any(), (name, refs[0]["status"])
    assert leaves == [[[128, 128]], [[128, 128, 128, 128]], [[64, 72]], [[96, 104]]]


@dtypes
def test_chunk_edges_have_the_claimed_chunks(dtype):
    leaves = []
    for name, fs, refs in _refs("chunk_edges", dtype):
        itot, jtot, ktot = fs[0]["qt"].shape
        assert ktot == 5
        leaves.append(ve.leaf_sizes(itot * jtot))
        st = refs[0]["status"]
        assert (st == 1).any() and ((st & 4) != 0).any(), (name, st)
        f, r = fs[0], refs[0]
        for k in numpy.nonzero(st == 1)[0]:             # the plane's last point, the end of its last chunk, is cloudy at the root
            last = r["beta"][k] * (f["qt"][-1, -1, k] - f["qt_av"][k]) + f["qt_av"][k] - f["qsat"][-1, -1, k]
            assert last > 1e-5, (name, k, last)
    assert [len(c) for c in leaves] == [1, 2, 2]
    assert leaves[0][0] == [128] * 64 and leaves[1][1] == [1] and leaves[2][1] == [8] and leaves[1][0] == leaves[2][0] == [128] * 64


@dtypes
def test_ragged_columns_have_ragged_tile_groups(dtype):
    (na, fa, ra), (nb, fb, rb) = _refs("ragged_columns", dtype)
    assert len(fa) == 3 and fa[0]["qt"].shape == (64, 64, 21) and len(fb) == 37 and fb[0]["qt"].shape == (9, 7, 23)
    # vnudge_impl: 64 x 64 planes take kt = 2 levels per workgroup, tg = 16 / kt tiles per group
    kt = 2
    tiles, tg = -(-21 // kt), 16 // kt
    assert tiles % tg != 0 and -(-tiles // tg) == 2                             # the second group of EVERY column is ragged
    assert 23 % 16 != 0                                                          # streamed (kt = 1, tg = 16): 23 tiles, ragged too
    assert (37 * 2) % 8 != 0                                                     # kt = 16: 74 groups on 80 workgroups
    for name, refs in ((na, ra), (nb, rb)):
        assert len({tuple(r["status"]) for r in refs}) == len(refs), name       # every LES has its own pattern
        assert all((r["status"] != 0).any() for r in refs) and any(_both_finders(r["status"]) for r in refs), name


def test_same_bits_tells_zeros_and_nans_apart():
    a = numpy.array([0.0, numpy.nan, numpy.inf, 1.0])
    assert ve.same_bits(a, a.copy())
    assert not ve.same_bits(a, numpy.array([-0.0, numpy.nan, numpy.inf, 1.0]))
    assert not ve.same_bits(a, numpy.array([0.0, 2.0, numpy.inf, 1.0]))
    assert not ve.same_bits(a, numpy.array([0.0, numpy.nan, -numpy.inf, 1.0]))
    assert not ve.same_bits(a, a.astype(numpy.float32))
    assert ve.same_bits(numpy.array([1, 2], dtype=numpy.int32), numpy.array([1, 2], dtype=numpy.int32))


def test_route_restores_the_environment(monkeypatch):
    import os
    monkeypatch.setenv("SPC_VN_PAIR", "0")
    monkeypatch.delenv("SPC_VN_GLOBAL", raising=False)
    with ve.route("global"):
        assert os.environ["SPC_VN_GLOBAL"] == "1" and os.environ["SPC_VN_PAIR"] == "1" and os.environ["SPC_VN_TRANSPOSE"] == "1"
    assert os.environ["SPC_VN_PAIR"] == "0" and "SPC_VN_GLOBAL" not in os.environ
