"""K26 without a GPU: the struct layout of spc_les_hmix_args, the host-side refusals of spc_les_hmix_* and
spc_les_hmix_lines_per_block, sp_coupler_amd/horizontal_mixing.py against hand values, the properties of the NumPy oracle of
tests/les_hmix_ref.py that the kernel inherits by being bit-equal to it (its distance from a dense cyclic solve in extended
precision, conservation of the line and the plane sum, the bounds of a mixed line), and models.DeviceLESEnsemble's
enable_mixing(implicit=True) on an oracle-backed engine against its host twin, one case per key of its caches."""
import ctypes
import functools
import math
import os
import subprocess

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi, device_les, models, spcpl
from sp_coupler_amd import horizontal_mixing as hm
from sp_coupler_amd import mixing
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_hmix_ref as lhr
from tests import les_micro_ref as lmr
from tests import les_mix_ref as lxr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPS = [numpy.float64, numpy.float32]
#: the line lengths of the oracle's own tests: the closing unknown beside 1, 2, 3 and 4 others, a chunk, 33 and 64 cells
LENGTHS = (2, 3, 4, 5, 8, 33, 64)
SEEDS = (0, 1, 2)
FIELDS = ("U", "THL", "X")                                         # the winds' pair, the scalars' (the largest weights), a pair of its own
#: the largest distance of the oracle from the dense longdouble solve seen over cases(), in units of eps max|x| of the line, and
#: the limit: four times that (the seeds are few and the distance grows with n)
SEEN = {numpy.float64: 3.29, numpy.float32: 2.87}
LIMIT = {t: 4 * v for t, v in SEEN.items()}


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


# -- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_struct_layout_of_the_horizontal_mixing_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.LesHmixArgs, "spc_les_hmix_args"
    fields = ["n_les", "itot", "jtot", "ktot", "n_fields", "axes", "reserved", "fields", "ax", "ay", "km", "kh2"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_ABI_VERSION);', 'printf("%d\\n", SPC_HMIX_MAX_FIELDS);']
    want = [ctypes.sizeof(cls), 4, _abi.SPC_HMIX_MAX_FIELDS]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and _abi.ABI_VERSION == 4 and _abi.SPC_HMIX_MAX_FIELDS == 6


def _args(n=4, itot=8, jtot=8, ktot=20, n_fields=3, axes=3, fields=None, ax=None, ay=None, **ptrs):
    g = _abi.LesHmixArgs()
    g.n_les, g.itot, g.jtot, g.ktot, g.n_fields, g.axes = n, itot, jtot, ktot, n_fields, axes
    for i, k in enumerate(("km", "kh2")):                          # distinct, 16-byte aligned, never dereferenced
        setattr(g, k, ptrs.get(k, 4096 * (i + 1)))
    for f in range(_abi.SPC_HMIX_MAX_FIELDS):
        g.fields[f] = (fields or {}).get(f, 4096 * (f + 10))
        g.ax[f] = (ax or {}).get(f, 4096 * (f + 20))
        g.ay[f] = (ay or {}).get(f, 4096 * (f + 30))
    return g


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch, so none of these calls needs a device; in the order of the checks, each with the
    complete text of spc_last_error()"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_hmix_" + sfx)
    esize = 8 if sfx == "f64" else 4

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert (fn(None, None), lib.spc_last_error()) == (E, b"args is NULL")
    assert call(n=-1) == (E, b"les_hmix: n_les = -1 < 0")
    assert call(jtot=0) == (E, b"les_hmix: itot, jtot and ktot must be >= 1")
    for count in (0, 7, -1):
        assert call(n_fields=count) == (E, b"les_hmix: field count %d outside 1 ... 6" % count)
    for axes in (0, 4, -1):
        assert call(axes=axes) == (E, b"les_hmix: axes %d outside 1 ... 3 (bit 0: along i, bit 1: along j)" % axes)
        assert call(axes=axes, n=0)[0] == E                         # the scalar checks come before the no-op
    assert call(n=0, km=None, fields={0: None})[0] == 0             # n_les == 0: a no-op after the scalar checks
    for k in ("km", "kh2"):
        assert call(**{k: None}) == (E, b"required pointer %s is NULL" % k.encode())
    for k in ("fields", "ax", "ay"):
        assert call(**{k: {1: None}}) == (E, b"required pointer %s[f] is NULL" % k.encode())
    assert call(fields={2: 4096 * 10}) == (E, b"les_hmix: fields[0] and fields[2] are the same field")
    also = b"les_hmix: fields[%d] is also km, kh2 or a coefficient (it is written while they are read)"
    assert call(fields={1: 4096}) == (E, also % 1) and call(fields={0: 8192}) == (E, also % 0)
    assert call(ax={2: 4096 * 10}) == (E, also % 0) and call(ay={0: 4096 * 12}) == (E, also % 2)
    for kw in (dict(km=4096 + esize // 2), dict(kh2=8192 + 1), dict(fields={1: 4096 * 11 + 2}), dict(ax={0: 4096 * 20 + 1}), dict(ay={2: 4096 * 32 + esize - 1})):
        assert call(**kw) == (E, b"les_hmix: a pointer is not aligned to its element type")
    top = 641 if esize == 8 else 1281
    assert lib.spc_les_hmix_lines_per_block(top, esize) == 16 and lib.spc_les_hmix_lines_per_block(top + 1, esize) == 0
    assert call(itot=top + 1) == (U, b"les_hmix: itot %d above the %d cells of a line of which 16 fit the LDS" % (top + 1, top))
    assert call(jtot=top + 1) == (U, b"les_hmix: jtot %d above the %d cells of a line of which 16 fit the LDS" % (top + 1, top))
    assert call(itot=top + 1, jtot=top + 1, axes=1)[1].startswith(b"les_hmix: itot")
    assert call(itot=top + 1, jtot=top + 1, axes=2)[1].startswith(b"les_hmix: jtot")
    assert call(n=2 ** 40, itot=2, jtot=1, ktot=1, axes=1) == (U, b"les_hmix: too many workgroups")
    assert call(n=2 ** 40, itot=1, jtot=2, ktot=1, axes=2) == (U, b"les_hmix: too many workgroups")


def test_lines_per_block_of_both_types(lib):
    """256 lines while q and z fit 64 KiB, then 128 and 64; 32 and 16 lines of the whole LDS; every extent up to 256 is supported in
    both types; the table of the oracle-backed engine is the library's"""
    f = lib.spc_les_hmix_lines_per_block
    assert [f(n, 8) for n in (1, 2, 17, 18, 33, 34, 64, 65, 66, 256, 321, 322, 641, 642)] == [256, 256, 256, 128, 128, 64, 64, 64, 32, 32, 32, 16, 16, 0]
    assert [f(n, 4) for n in (1, 33, 34, 65, 66, 129, 130, 256, 641, 642, 1281, 1282)] == [256, 256, 128, 128, 64, 64, 32, 32, 32, 16, 16, 0]
    assert f(0, 8) == f(-1, 4) == f(8, 2) == f(8, 16) == 0
    for esize in (4, 8):
        assert all(f(n, esize) for n in range(1, 257))
        assert all(f(n, esize) == lhr.lines_per_block(n, esize) for n in list(range(0, 700)) + [1281, 1282])


# -- horizontal_mixing.py -------------------------------------------------------------------------------------------------------
def test_the_host_module_against_hand_values():
    assert hm.KH_CAP == 1000.0 and hm.coefficients is mixing.coefficients
    assert hm.bound(3).tolist() == [2000.0] * 3 and hm.bound(3).dtype == numpy.float64
    assert hm.bound(2, numpy.array([5.0, 7.5])).tolist() == [10.0, 15.0] and hm.bound(1, 0.25).tolist() == [0.5]
    _, _, wind, scalar = hm.coefficients(900.0, 200.0, numpy.array([200.0, 300.0]), prandtl=0.5)
    assert numpy.allclose(wind[0], [0.01125, 0.01125], rtol=1e-15) and numpy.allclose(wind[1], [0.01125, 0.005], rtol=1e-15)
    assert numpy.allclose(scalar[0], 2 * wind[0], rtol=1e-15) and numpy.allclose(scalar[1], 2 * wind[1], rtol=1e-15)
    for bad in (0.0, -1.0, float("nan"), float("inf"), numpy.array([1.0, 0.0])):
        with pytest.raises(ValueError, match="kh_cap"):
            hm.bound(2, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for call in (lambda: hm.coefficients(bad, 200.0, 200.0), lambda: hm.coefficients(900.0, bad, 200.0), lambda: hm.coefficients(900.0, 200.0, bad),
                     lambda: hm.coefficients(900.0, 200.0, 200.0, prandtl=bad)):
            with pytest.raises(ValueError):
                call()


# -- the oracle's own properties -------------------------------------------------------------------------------------------------
def dense_solve(x, w, axis):
    """Gauss-Jordan in numpy.longdouble of the dense cyclic system of every line of ``x`` along ``axis`` with the face weights
    ``w`` as they are (rounded): row i holds 1 + w[im] + w[i] on the diagonal, -w[i] at ip and -w[im] at im.  The matrix is
    strictly diagonally dominant by columns and by rows, so no pivoting is needed"""
    L = numpy.longdouble
    X, W = numpy.moveaxis(x, axis, -1).astype(L), numpy.moveaxis(w, axis, -1).astype(L)
    n = X.shape[-1]
    M = numpy.zeros(X.shape + (n + 1,), dtype=L)
    for i in range(n):
        M[..., i, i] += 1 + W[..., i] + W[..., i - 1]
        M[..., i, (i + 1) % n] -= W[..., i]
        M[..., i, (i - 1) % n] -= W[..., i - 1]
    M[..., n] = X
    for a in range(n):
        row = M[..., a, :] / M[..., a, a][..., None]
        col = M[..., :, a].copy()
        col[..., a] = 0
        M = M - col[..., None] * row[..., None, :]
        M[..., a, :] = row
    return numpy.moveaxis(M[..., n], -1, axis)


@functools.lru_cache(maxsize=None)
def cases(dtype):
    """the cases the three properties share, computed once and left unchanged: (x, w, axis, x' of the oracle, the longdouble solve)
    for lines of LENGTHS cells along i and along j, SEEDS and FIELDS; the weights reach about 1.35 (THL)"""
    out = []
    for n in LENGTHS:
        for seed in SEEDS:
            for axis, shape in ((1, (2, n, 3, 2)), (2, (2, 3, n, 2))):
                c = lhr.case(shape, dtype, seed=100 + seed)
                for k in FIELDS:
                    w = lhr.weights(c["km"], c["coef"][k][axis - 1], c["kh2"], axis)
                    new = lhr.sweep(c[k], w, axis)
                    for a in (c[k], w, new):
                        a.setflags(write=False)
                    out.append((c[k], w, axis, new, dense_solve(c[k], w, axis)))
    return out


@pytest.mark.parametrize("dtype", NPS)
def test_the_oracle_solves_the_cyclic_system(dtype):
    """float64 and float32 against the dense longdouble solve of every line.  The condensation is a block elimination (a Thomas
    solve with two right-hand sides, then a Schur complement of one unknown) whose backward error we did not derive; the limit is
    measured as the rule of this test says: the largest distance over cases() is 3.29 (float64) and 2.87 (float32) units of
    eps max|x| of the line, and the limit is four times that, 13.16 and 11.48: the seeds are few and the distance grows with n."""
    eps = float(numpy.finfo(dtype).eps)
    worst, top = 0.0, 0.0
    for x, w, axis, new, exact in cases(dtype):
        scale = eps * numpy.abs(x).max(axis=axis, keepdims=True).astype(numpy.longdouble)
        worst = max(worst, float((numpy.abs(new - exact) / scale).max()))
        top = max(top, float(w.max()))
        assert (new != x).any()
    print("%s: the oracle is at most %.3g eps max|x| from the longdouble solve; the largest weight is %.3g" % (numpy.dtype(dtype).name, worst, top))
    assert top > 1.3 and worst <= LIMIT[dtype], worst


@pytest.mark.parametrize("dtype", NPS)
def test_the_line_sum_is_conserved_to_rounding(dtype):
    """w is one number for both cells of a face, so the matrix of the rounded weights is symmetric with unit column sums and the
    EXACT solution of a line has the sum of the line.  Every computed cell is at most LIMIT eps max|x| from it
    (test_the_oracle_solves_the_cyclic_system), so the sum of the n cells of a line moves by at most n LIMIT eps max|x|.  The sums
    are taken exactly (math.fsum, float64; the float32 values convert exactly)."""
    eps = float(numpy.finfo(dtype).eps)
    exact = lambda a: math.fsum(numpy.asarray(a, dtype=numpy.float64).ravel())                 # noqa: E731
    for x, w, axis, new, _ in cases(dtype):
        X, N = numpy.moveaxis(x, axis, -1).reshape(-1, x.shape[axis]), numpy.moveaxis(new, axis, -1).reshape(-1, x.shape[axis])
        for old, mixed in zip(X, N):
            change = exact(numpy.concatenate([mixed.astype(numpy.float64), -old.astype(numpy.float64)]))
            assert abs(change) <= len(old) * LIMIT[dtype] * eps * float(numpy.abs(old).max()), (axis, len(old), change)


@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("shape", [(2, 5, 8, 3), (1, 33, 4, 2), (2, 2, 3, 5), (1, 64, 64, 1)])
def test_the_plane_sum_is_conserved_by_both_sweeps(shape, dtype):
    """the first sweep moves the sum of each of its lines by at most itot LIMIT eps max|x|, the second that of each of its lines by
    at most jtot LIMIT eps max|x'| (the bound of the line sum, with max|x'| <= max|x| (1 + LIMIT eps) by the bound below); a plane
    (l, :, :, k) has jtot lines of the first kind and itot of the second"""
    eps = float(numpy.finfo(dtype).eps)
    lim = LIMIT[dtype]
    c = lhr.case(shape, dtype, seed=5)
    outs = lhr.oracle(c)
    for k in lhr.NAMES:
        x, new = c[k].astype(numpy.float64), outs[k].astype(numpy.float64)
        for l in range(shape[0]):
            for lev in range(shape[3]):
                change = math.fsum(numpy.concatenate([new[l, :, :, lev].ravel(), -x[l, :, :, lev].ravel()]))
                top = float(numpy.abs(x[l, :, :, lev]).max())
                assert abs(change) <= shape[1] * shape[2] * lim * eps * top * (2 + lim * eps), (k, l, lev, change)
        assert (new != x).any()


@pytest.mark.parametrize("dtype", NPS)
def test_a_mixed_line_stays_within_its_minimum_and_maximum(dtype):
    """The matrix is an M-matrix whose rows sum to 1, so its inverse is not negative and has rows that sum to 1: the exact x' is a
    convex combination of the line.  Every computed cell is at most LIMIT eps max|x| from it, which is the slack.  A constant
    finite line is its own minimum and maximum: it stays constant to that slack (it does not keep its bits)."""
    eps = float(numpy.finfo(dtype).eps)
    for x, w, axis, new, _ in cases(dtype):
        x64, n64 = x.astype(numpy.float64), new.astype(numpy.float64)
        slack = LIMIT[dtype] * eps * numpy.abs(x64).max(axis=axis, keepdims=True)
        assert (n64 >= x64.min(axis=axis, keepdims=True) - slack).all() and (n64 <= x64.max(axis=axis, keepdims=True) + slack).all()
    c = lhr.case((2, 33, 3, 2), dtype, seed=8)
    flat = numpy.full_like(c["THL"], 290.7)
    new = lhr.sweep(flat, lhr.weights(c["km"], c["coef"]["THL"][0], c["kh2"], 1), 1)
    assert numpy.abs(new.astype(numpy.float64) - float(flat[0, 0, 0, 0])).max() <= LIMIT[dtype] * eps * 290.7


# -- the engines --------------------------------------------------------------------------------------------------------------------
def test_bodies_on_the_oracle_backed_engine():
    """the plumbing of every body but the refusals (which need the library) runs without a GPU"""
    eng = lhr.HmixOracleEngine()
    for name, job in lhr.jobs(eng):
        if name != "refusals":
            job()


def test_row_blocks_of_a_multi_engine_equal_one_engine():
    """MultiDeviceEngine.les_hmix over Sharded row blocks 4 + 3 and 1 + 1 + 0, on oracle-backed engines"""
    for engines, n, blocks in ((2, 7, [4, 3]), (3, 2, [1, 1, 0])):
        multi = MultiDeviceEngine([lhr.HmixOracleEngine() for _ in range(engines)], min_cols_per_device=1)
        assert lhr.check_multi(lhr.HmixOracleEngine(), multi, n) == blocks


# -- the ensemble ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(lhr.VARIANTS))
def test_ensemble_equals_the_host_twin(variant):
    """three steps and a constantT nudge before the last: every profile, field and viscosity bit-equal to the host twin after each
    of them: plain, with radiation + thermo + microphysics + K23 + K25, ("forced") with K19, K21, K23 and K25, and with K15 by the
    slab mean of the uncapped km"""
    host = lhr.check_ensemble(lhr.HmixOracleEngine(), [lhr.HmixOracleEngine()], 3, variant)
    assert variant != "forced" or host[-1]["counts"].sum() > 0


def change_of(key):
    """what changes the cache key ``key`` before the second step, on the twin and on the device ensemble alike"""
    def change(ens, step):
        if step != 1:
            return
        if key == "dt":
            ens.model_time += 300.0
        elif key == "prandtl":
            ens.mix_par["prandtl"] = 0.6
        elif key == "kh_cap":
            ens.mix_par["kh_cap"] = 0.05
    return change


@pytest.mark.parametrize("key", ("dt", "prandtl", "kh_cap"))
def test_uploads_follow_their_keys_with_k19_k21_k23_and_k25_enabled(monkeypatch, key):
    """one case per key of the caches: the key changes between the first and the second step, and the device ensemble stays
    bit-equal to the twin, which keeps nothing; an ensemble that ignores the keys of the mixing's uploads (every comparison of a
    key inside _mix says "the same") does not"""
    kw = dict(lhr.VARIANTS["forced"], change=change_of(key))
    host = lhr.ensemble_run(lhr.HmixOracleEngine(), 3, False, **kw)[1]
    same = lhr.ensemble_run(lhr.HmixOracleEngine(), 3, False, **lhr.VARIANTS["forced"])[1]
    assert (host[2]["field U"] != same[2]["field U"]).any() or (host[2]["field THL"] != same[2]["field THL"]).any()
    lmr.same_logs(host, lhr.ensemble_run(lhr.HmixOracleEngine(), 3, True, **kw)[1])
    inner = models.DeviceLESEnsemble._mix

    def stale(self, dt):
        saved = device_les._kept
        device_les._kept = lambda old, k, make: old if old is not None else make()
        try:
            return inner(self, dt)
        finally:
            device_les._kept = saved
    monkeypatch.setattr(models.DeviceLESEnsemble, "_mix", stale)
    with pytest.raises(AssertionError):
        lmr.same_logs(host, lhr.ensemble_run(lhr.HmixOracleEngine(), 3, True, **kw)[1])


def test_uploads_are_kept_until_their_inputs_change():
    ens = lhr.ensemble_run(lhr.HmixOracleEngine(), 2, True, steps=0)[0]
    ens.evolve_model_batched(ens.model_time + 60.0)
    coef, kh2, huge = ens._mix_coef, ens._hmix_kh2, ens._hmix_huge
    ens.evolve_model_batched(ens.model_time + 60.0)
    assert ens._mix_coef is coef and ens._hmix_kh2 is kh2 and ens._hmix_huge is huge
    ens.evolve_model_batched(ens.model_time + 30.0)
    assert ens._mix_coef is not coef and ens._hmix_kh2 is kh2
    ens.mix_par["kh_cap"] = 5.0
    ens.evolve_model_batched(ens.model_time + 30.0)
    assert ens._hmix_kh2 is not kh2 and ens._mix_spare == {}


class Spy(lhr.HmixOracleEngine):
    calls = None


for _name in ("les_mix", "les_hmix", "les_vmix", "slab_means"):
    def _spy(self, *a, _n=_name, **kw):
        self.calls.append((_n, len(a[0]) if _n == "les_mix" else None))
        return getattr(lhr.HmixOracleEngine, _n)(self, *a, **kw)
    setattr(Spy, _name, _spy)


def test_launches_per_step():
    """implicit: per step one les_mix WITHOUT fields, one les_hmix, then les_vmix where enabled, never a second les_mix;
    explicit: what it was, and never a les_hmix"""
    for vmix in (False, True):
        eng = Spy()
        eng.calls = []
        ens, log = lhr.ensemble_run(eng, 2, True, vmix=vmix)
        mine = [c for c in eng.calls if c[0].startswith("les_")]
        assert mine == ([("les_mix", 0), ("les_hmix", None)] + ([("les_vmix", None)] if vmix else [])) * 3, mine
        assert ens.mixing_capped is False and ens.mixing_k_max > 0 and ens._mix_spare == {}
        assert not vmix or ens.get_vertical_viscosity_batched() is ens.get_eddy_viscosity_batched()
    eng = Spy()
    eng.calls = []
    ens, log = lhr.ensemble_run(eng, 2, True, implicit=False, vmix=True)
    mine = [c for c in eng.calls if c[0].startswith("les_")]
    assert mine == [("les_mix", 4), ("les_mix", 0), ("les_vmix", None)] * 3 and ens.mixing_capped is True, mine


@pytest.mark.parametrize("variant", ["plain", "forced"])
def test_the_explicit_mode_is_what_it_was(variant):
    """implicit=False, given or left out: the device ensemble is bit-equal to K24's own twin of tests/les_mix_ref.py, which knows
    nothing of K26, and to the ensemble that never heard the argument"""
    kw = lxr.VARIANTS[variant]
    host = lxr.ensemble_run(lhr.HmixOracleEngine(), 3, False, **kw)[1]
    plain = lxr.ensemble_run(lhr.HmixOracleEngine(), 3, True, **kw)[1]
    given = lhr.ensemble_run(lhr.HmixOracleEngine(), 3, True, implicit=False, **kw)[1]
    lmr.same_logs(host, plain)
    lmr.same_logs(host, given)


def test_refusals_of_enable_mixing():
    ens = lxr.ensemble_run(lhr.HmixOracleEngine(), 2, True, mixing=None, steps=0)[0]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kh_cap"):
            ens.enable_mixing(implicit=True, kh_cap=bad)
    assert ens.mixing is False
    ens.enable_mixing(implicit=True)
    assert ens.mix_par["implicit"] is True and ens.mix_par["kh_cap"] == hm.KH_CAP
    ens.enable_mixing()
    assert ens.mix_par["implicit"] is False
    bare = lxr.ensemble_run(lhr.lvr.VmixOracleEngine(), 2, True, mixing=None, steps=0)[0]
    with pytest.raises(ValueError, match="no les_hmix"):
        bare.enable_mixing(implicit=True)
    bare.enable_mixing()                                            # (the explicit mode needs no les_hmix)
    assert bare.mixing is True


def test_nan_stays_in_its_line_then_in_its_plane():
    """the consequence the header states, on the oracle: after the first sweep the NaN fills its line along i, after the second the
    j lines of those cells"""
    c = lhr.case((2, 4, 5, 3), numpy.float64, seed=2)
    c["X"][1, 2, 3, 1] = numpy.nan
    one, both = lhr.oracle(c, ("X",), 1)["X"], lhr.oracle(c, ("X",), 3)["X"]
    hit = numpy.zeros(c["X"].shape, dtype=bool)
    hit[1, :, 3, 1] = True
    assert numpy.array_equal(numpy.isnan(one), hit)
    hit[1, :, :, 1] = True
    assert numpy.array_equal(numpy.isnan(both), hit)
    assert_bits("n == 1 keeps every bit", lhr.sweep(c["X"][:, :1], lhr.weights(c["km"][:, :1], c["coef"]["X"][0], c["kh2"], 1), 1), c["X"][:, :1])


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(lhr.VARIANTS))
def test_float32_ensemble_equals_the_host_twin(variant):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    host = lhr.check_ensemble(f32_of(lhr.HmixOracleEngine)(), [f32_of(lhr.HmixOracleEngine)()], 3, variant)
    assert variant != "forced" or host[-1]["counts"].sum() > 0
