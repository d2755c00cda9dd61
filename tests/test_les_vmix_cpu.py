"""K25 without a GPU: the properties of the NumPy oracle of tests/les_vmix_ref.py that the kernel inherits by being bit-equal to it
(conservation, the bounds of a mixed column, its distance from an extended-precision solve beside K15's), the functions of
sp_coupler_amd/vertical_mixing.py against hand-computed values and against diffusion.matrix, and models.DeviceLESEnsemble's
enable_vertical_mixing() on an oracle-backed engine against its host twins, one case per key of its caches."""
import math

import numpy
import pytest

from sp_coupler_amd import device_les, models, spcpl
from sp_coupler_amd import diffusion as df
from sp_coupler_amd import mixing
from sp_coupler_amd import vertical_mixing as vm
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_diffuse_ref as ldr
from tests import les_micro_ref as lmr
from tests import les_vmix_ref as lvr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

SHAPES = [(3, 8, 8, 20), (2, 2, 2, 5), (2, 3, 5, 7), (1, 1, 4, 2), (2, 3, 5, 65)]
NPS = [numpy.float64, numpy.float32]
#: the roundings of one level of the rule: b (2), lo q, the pivot, the division, q, lo y, the sum, y; the product and the sum of the
#: back substitution
ROUNDINGS = 11


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def system(c, name):
    """float64 (lo, up) [n x itot x jtot x ktot] of the field: the off-diagonals the rule forms, as it rounds them"""
    s = lvr.faces(c["km"], c["kb"], c["kv2"])
    el, eu = c["coef"][name]
    lo = el[:, None, None, :] * s
    up = numpy.zeros_like(lo)
    up[..., :-1] = eu[:, None, None, :-1] * s[..., 1:]
    return lo.astype(numpy.float64), up.astype(numpy.float64)


def weighted_residual_bound(u, lo, up, new, w):
    """ROUNDINGS * 3 u sum_k w[k] (|A| |x'|)[k] per column: the computed x' solves (A + dA) x' = d with |dA| <= ROUNDINGS u |L| |U|
    to first order (every rounding of a level perturbs one entry of the computed factors by a relative u), and |L| |U| <= 3 |A|
    for a tridiagonal matrix that is diagonally dominant (N. Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
    theorems 9.12 and 9.13)"""
    a = numpy.abs(new)
    row = (1.0 + lo + up) * a
    row[..., 1:] += lo[..., 1:] * a[..., :-1]
    row[..., :-1] += up[..., :-1] * a[..., 1:]
    return 3 * ROUNDINGS * u * (w[:, None, None, :] * row)


# -- the oracle's own properties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_weighted_column_sum_is_conserved_to_rounding(shape, dtype):
    """Without a flux and a drag, with w = Rhobf dz (float64) and A the matrix of the rounded lo and up: exactly,
    sum w x' - sum w x = - sum_k w[k] ((A x')[k] - x[k]) + sum over the faces of (w[k] lo[k] - w[k-1] up[k-1]) (x'[k-1] - x'[k]).
    The first term is the residual of the solve: at most 3 * 11 u sum w |A| |x'| (weighted_residual_bound).  The second is what the
    rounding of the coefficients leaves of the symmetry w[k] el[k] = w[k-1] eu[k-1]: el and eu are rounded to T once (a relative u
    each) and lo = fl(el s), up = fl(eu s) once more, four roundings in all, and the float64 formation of el, eu and w adds at most
    eight roundings of float64: |w[k] lo[k] - w[k-1] up[k-1]| <= (4 u + 8 u64) max of the two.  The sums are taken exactly
    (math.fsum, float64; the float32 values convert exactly)."""
    u, u64 = float(numpy.finfo(dtype).eps) / 2, 2.0 ** -53
    exact = lambda a: math.fsum(numpy.asarray(a, dtype=numpy.float64).ravel())                 # noqa: E731
    c = lvr.case(shape, dtype, seed=3)
    outs, _ = lvr.oracle(c, flux=False, drag=False)
    w = c["w"]
    moved = False
    for k in lvr.NAMES:
        x, new = c[k].astype(numpy.float64), outs[k].astype(numpy.float64)
        lo, up = system(c, k)
        moved = moved or bool((new != x).any())
        resid = weighted_residual_bound(u, lo, up, new, w)
        skew = numpy.zeros_like(new)
        skew[..., 1:] = (4 * u + 8 * u64) * numpy.maximum(w[:, None, None, 1:] * lo[..., 1:], w[:, None, None, :-1] * up[..., :-1]) \
            * numpy.abs(new[..., :-1] - new[..., 1:])
        for col in numpy.ndindex(shape[:3]):
            wl = w[col[0]]
            change = exact(numpy.concatenate([wl * new[col], -(wl * x[col])]))
            bound = exact(resid[col]) + exact(skew[col]) + 2 * u64 * exact(wl * (numpy.abs(new[col]) + numpy.abs(x[col])))   # (the products w x)
            assert abs(change) <= bound * (1 + 1e-9), (k, col, change, bound)
    assert moved


@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_mixed_column_stays_within_its_minimum_and_maximum(shape, dtype):
    """Without a flux and a drag the matrix is an M-matrix whose rows sum to 1, so its inverse is not negative, has rows that sum
    to 1 and the norm 1: the exact x' is a convex combination of the column.  The computed x' solves the system with the residual
    of weighted_residual_bound (w = 1), so it is at most 3 * 11 u (1 + 2 max(lo + up)) max|x'| away."""
    u = float(numpy.finfo(dtype).eps) / 2
    c = lvr.case(shape, dtype, seed=4)
    outs, _ = lvr.oracle(c, flux=False, drag=False)
    for k in lvr.NAMES:
        x, new = c[k].astype(numpy.float64), outs[k].astype(numpy.float64)
        lo, up = system(c, k)
        slack = 3 * ROUNDINGS * u * (1 + 2 * (lo + up).max(axis=3)) * numpy.abs(new).max(axis=3)
        assert (new >= (x.min(axis=3) - slack)[..., None]).all() and (new <= (x.max(axis=3) + slack)[..., None]).all(), k


def level_case(n=3, ktot=40, seed=11):
    """a km that is constant on every level, so that K15 can take it as a face diffusivity: (case, kd [n x ktot], zh, zf, rhobf)"""
    rng = numpy.random.default_rng(seed)
    rhobf, zh, zf, _, _ = lvr.lrr.grid(n, ktot, rng)
    shape = (n, 3, 4, ktot)
    c = lvr.case(shape, numpy.float64, seed=seed)
    prof = 8.0 * rng.random((n, ktot)) ** 2
    c["km"] = numpy.ascontiguousarray(numpy.broadcast_to(prof[:, None, None, :], shape))
    wind, scalar, c["s0"] = vm.coefficients(zh, zf, rhobf, lvr.DT)
    c["coef"] = {k: wind for k in lvr.NAMES}
    c["kb"], c["kv2"] = vm.background(n, ktot, vm.K_BG, 1e3)
    return c, mixing.face_diffusivity(prof, vm.K_BG), zh, zf, rhobf


def longdouble_solve(x, a, b, cc):
    """Thomas in numpy.longdouble of the tridiagonal system (a, b, cc [n x ktot]) for the columns x [n x itot x jtot x ktot]"""
    L = numpy.longdouble
    P = lambda v, k: v[:, None, None, k].astype(L)                                           # noqa: E731
    x = x.astype(L)
    ktot = x.shape[3]
    q, y = numpy.empty_like(x), numpy.empty_like(x)
    for k in range(ktot):
        den = P(b, k) - (P(a, k) * q[..., k - 1] if k else 0)
        q[..., k] = P(cc, k) / den
        y[..., k] = (x[..., k] - (P(a, k) * y[..., k - 1] if k else 0)) / den
    out = y.copy()
    for k in range(ktot - 2, -1, -1):
        out[..., k] = y[..., k] - q[..., k] * out[..., k + 1]
    return out


def test_no_further_from_an_extended_solve_than_four_times_k15():
    """float64, a km constant per level: K25's oracle and K15's oracle (diffusion.profiles(kd=...)) against a numpy.longdouble
    Thomas solve of diffusion.matrix(kd=...)'s system.  Both round the same count of operations; K25 forms its coefficients per
    cell.  K25's distance may be at most 4 times K15's plus 4 ulp of max|x|.  Measured on this case: K25 2.12e-15 against K15's
    1.64e-15 on U (ratio 1.29), 1.11e-13 against 1.08e-13 on THL (ratio 1.03), 7.01e-16 against 7.01e-16 on X (ratio 1.00)."""
    c, kd, zh, zf, rhobf = level_case()
    a, b, cc, _, _ = df.matrix(zh, zf, rhobf, lvr.DT, kd=kd)
    pa, pm, pcp, _ = df.profiles(zh, zf, rhobf, lvr.DT, kd=kd)
    outs, _ = lvr.oracle(c, flux=False, drag=False)
    for k in ("U", "THL", "X"):
        exact = longdouble_solve(c[k], a, b, cc)
        d25 = float(numpy.abs(outs[k] - exact).max())
        d15 = float(numpy.abs(ldr.les_diffuse(c[k], pa, pm, pcp, None, None) - exact).max())
        ulp = float(numpy.spacing(numpy.abs(c[k]).max()))
        print("%s: K25 %.3g K15 %.3g ratio %.3g" % (k, d25, d15, d25 / d15 if d15 else float("inf")))
        assert d25 <= 4 * d15 + 4 * ulp, (k, d25, d15)
        assert (outs[k] != c[k]).any()


# -- vertical_mixing.py ------------------------------------------------------------------------------------------------------------
def test_coefficients_background_and_drag_against_hand_computed_values():
    zh, zf = numpy.array([0.0, 20.0, 40.0]), numpy.array([10.0, 30.0, 50.0])
    rho = numpy.ones((2, 3))
    wind, scalar, s0 = vm.coefficients(zh, zf, rho, 10.0, prandtl=0.5)
    assert wind[0].shape == wind[1].shape == scalar[0].shape == (2, 3) and s0.shape == (2,) and wind[0].dtype == numpy.float64
    assert numpy.allclose(wind[0], [[0.0, 0.0125, 0.0125]] * 2, rtol=1e-15) and numpy.allclose(wind[1], [[0.0125, 0.0125, 0.0]] * 2, rtol=1e-15)
    assert numpy.allclose(scalar[0], 2 * wind[0], rtol=1e-15) and numpy.allclose(scalar[1], 2 * wind[1], rtol=1e-15) and s0.tolist() == [0.5, 0.5]
    rho = numpy.array([[1.0, 3.0, 5.0]])
    wind, _, _ = vm.coefficients(zh, zf, rho, 10.0)
    assert numpy.allclose(wind[0], [[0.0, 0.5 * 10 * 2 / (60 * 20), 0.5 * 10 * 4 / (100 * 20)]], rtol=1e-15)
    assert numpy.allclose(wind[1], [[0.5 * 10 * 2 / (20 * 20), 0.5 * 10 * 4 / (60 * 20), 0.0]], rtol=1e-15)
    kb, kv2 = vm.background(2, 3)
    assert kb.tolist() == [[2 * df.K_BG] * 3] * 2 and kv2.tolist() == [2 * vm.KV_CAP] * 2 and vm.K_BG == df.K_BG
    kb, kv2 = vm.background(2, 3, k_bg=0.0, kv_cap=numpy.array([5.0, 7.0]))
    assert not kb.any() and kv2.tolist() == [10.0, 14.0]
    dr = vm.drag(numpy.array([0.1, 1.0]), zf, numpy.array([20.0, 20.0, 20.0]), 10.0)
    assert numpy.allclose(dr, [10.0 * (0.4 / math.log(100.0)) ** 2 / 20.0, 10.0 * (0.4 / math.log(10.0)) ** 2 / 20.0], rtol=1e-15)
    assert vm.KAPPA == mixing.KAPPA == 0.4 and vm.coefficients([0.0], [10.0], [[1.0]], 10.0)[0][0].tolist() == [[0.0]]


def test_refusals_of_the_host_module():
    zh, zf = numpy.array([0.0, 20.0]), numpy.array([10.0, 30.0])
    for z0m in (0.0, -1.0, 10.0, 11.0, float("nan"), numpy.array([0.1, 10.0])):
        with pytest.raises(ValueError, match="z0m"):
            vm.drag(z0m, zf, numpy.array([20.0, 20.0]), 10.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for call in (lambda: vm.coefficients(zh, zf, numpy.ones((1, 2)), bad), lambda: vm.coefficients(zh, zf, numpy.ones((1, 2)), 1.0, prandtl=bad),
                     lambda: vm.background(1, 2, kv_cap=bad), lambda: vm.drag(0.1, zf, numpy.array([20.0, 20.0]), bad)):
            with pytest.raises(ValueError):
                call()
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="k_bg"):
            vm.background(1, 2, k_bg=bad)
    with pytest.raises(ValueError):
        vm.coefficients(zh, zf[::-1], numpy.ones((1, 2)), 1.0)           # levels that do not ascend


def test_el_and_eu_are_the_off_diagonals_of_the_diffusion_matrix():
    """for a km that is constant per level, el[k] * 2 kd[k] and eu[k] * 2 kd[k+1] are -a[k] and -c[k] of diffusion.matrix(kd=...)
    in float64, to four roundings"""
    c, kd, zh, zf, rhobf = level_case()
    a, _, cc, _, _ = df.matrix(zh, zf, rhobf, lvr.DT, kd=kd)
    el, eu = vm.coefficients(zh, zf, rhobf, lvr.DT)[0]
    assert numpy.allclose(el[:, 1:] * 2 * kd[:, 1:], -a[:, 1:], rtol=4 * 2.0 ** -52, atol=0)
    assert numpy.allclose(eu[:, :-1] * 2 * kd[:, 1:], -cc[:, :-1], rtol=4 * 2.0 ** -52, atol=0)
    assert not el[:, 0].any() and not eu[:, -1].any()
    s = lvr.faces(c["km"], c["kb"], c["kv2"])
    assert numpy.allclose(s[:, 0, 0, 1:], 2 * kd[:, 1:], rtol=4 * 2.0 ** -52, atol=0)


# -- the engines --------------------------------------------------------------------------------------------------------------------
def test_bodies_on_the_oracle_backed_engine():
    """the plumbing of every body but the refusals (which need the library) runs without a GPU"""
    eng = lvr.VmixOracleEngine()
    for name, job in lvr.jobs(eng):
        if name != "refusals":
            job()


def test_row_blocks_of_a_multi_engine_equal_one_engine():
    """MultiDeviceEngine.les_vmix over Sharded row blocks 4 + 3 and 1 + 1 + 0, on oracle-backed engines"""
    for engines, n, blocks in ((2, 7, [4, 3]), (3, 2, [1, 1, 0])):
        multi = MultiDeviceEngine([lvr.VmixOracleEngine() for _ in range(engines)], min_cols_per_device=1)
        assert lvr.check_multi(lvr.VmixOracleEngine(), multi, n) == blocks


# -- the ensemble ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,cap,z0m", [("plain", None, True), ("plain", 1e6, True), ("plain", None, False), ("all", None, True), ("forced", None, True)])
def test_ensemble_equals_the_host_twin(variant, cap, z0m):
    """three steps and a constantT nudge before the last: every profile, field and both viscosities bit-equal to the host twin
    after each of them, with a cap of K24 that binds (the second buffer) and one that never does (km itself), with and without a
    roughness length, with radiation + thermo + microphysics + K23, and ("forced") with K19, K21, K23 and K24"""
    host, capped = lvr.check_ensemble(lvr.VmixOracleEngine(), [lvr.VmixOracleEngine()], 3, variant, cap=cap, z0m=z0m)
    assert (cap is None or not any(capped)) and (cap is not None or variant != "plain" or all(capped))
    assert variant != "forced" or host[-1]["counts"].sum() > 0


def test_the_drag_needs_a_roughness_length_and_slows_the_lowest_level():
    with_z0m = lvr.ensemble_run(lvr.VmixOracleEngine(), 3, True)[1]
    without = lvr.ensemble_run(lvr.VmixOracleEngine(), 3, True, z0m=False)[1]
    off = lvr.ensemble_run(lvr.VmixOracleEngine(), 3, True, drag=False)[1]
    lmr.same_logs([{k: v for k, v in r.items() if k != "p z0m"} for r in without], [{k: v for k, v in r.items() if k != "p z0m"} for r in off])
    assert numpy.abs(with_z0m[-1]["field U"][..., 0]).mean() < numpy.abs(without[-1]["field U"][..., 0]).mean()
    assert_bits("the scalars feel no drag in the first step", with_z0m[1]["field QT"], without[1]["field QT"])


def change_of(key):
    """what changes the cache key ``key`` before the second step, on a twin and on the device ensemble alike"""
    def change(ens, step):
        if step != 1:
            return
        if key == "dt":
            ens.model_time += 300.0
        elif key == "Rhobf":
            ens.p["Rhobf"] = ens.p["Rhobf"] * 1.25
        elif key == "prandtl":
            ens.mix_par["prandtl"] = 0.6
        elif key == "k_bg":
            ens.vmix_par["k_bg"] = 2.5
        elif key == "kv_cap":
            ens.vmix_par["kv_cap"] = 0.5
        elif key == "z0m":
            ens.set_forcings_batched(Z0M_surf=numpy.full(ens.n, 0.5))
    return change


KEYS = ("dt", "Rhobf", "prandtl", "k_bg", "kv_cap", "z0m")


@pytest.mark.parametrize("key", KEYS)
def test_uploads_follow_their_keys_with_k19_k21_k23_and_k24_enabled(monkeypatch, key):
    """one case per key of the caches: the key changes between the first and the second step, and the device ensemble stays
    bit-equal to the twin, which keeps nothing; an ensemble that ignores the keys of K25's uploads (every comparison of a key
    inside _vmix says "the same") does not"""
    kw = dict(lvr.VARIANTS["forced"], change=change_of(key))
    host = lvr.ensemble_run(lvr.VmixOracleEngine(), 3, False, **kw)[1]
    same = lvr.ensemble_run(lvr.VmixOracleEngine(), 3, False, **lvr.VARIANTS["forced"])[1]
    assert (host[2]["field U"] != same[2]["field U"]).any() or (host[2]["field THL"] != same[2]["field THL"]).any()
    lmr.same_logs(host, lvr.ensemble_run(lvr.VmixOracleEngine(), 3, True, **kw)[1])
    inner = models.DeviceLESEnsemble._vmix

    def stale(self, dt):
        saved = device_les._kept
        device_les._kept = lambda old, k, make: old if old is not None else make()
        try:
            return inner(self, dt)
        finally:
            device_les._kept = saved
    monkeypatch.setattr(models.DeviceLESEnsemble, "_vmix", stale)
    with pytest.raises(AssertionError):
        lmr.same_logs(host, lvr.ensemble_run(lvr.VmixOracleEngine(), 3, True, **kw)[1])


def test_uploads_are_kept_until_their_inputs_change():
    ens = lvr.ensemble_run(lvr.VmixOracleEngine(), 2, True, steps=0)[0]
    ens.evolve_model_batched(ens.model_time + 60.0)
    coef, drag = ens._vmix_coef, ens._vmix_drag
    ens.evolve_model_batched(ens.model_time + 60.0)
    assert ens._vmix_coef is coef and ens._vmix_drag is drag
    ens.evolve_model_batched(ens.model_time + 30.0)
    assert ens._vmix_coef is not coef and ens._vmix_drag is not drag


def test_refusals_of_enable_vertical_mixing():
    eng = lvr.VmixOracleEngine()
    ens = lvr.lxr.ensemble_run(eng, 2, True, mixing=None, steps=0)[0]
    with pytest.raises(ValueError, match="enable_mixing"):
        ens.enable_vertical_mixing()
    ens.enable_mixing()
    for kw in (dict(kv_cap=0.0), dict(kv_cap=float("nan")), dict(k_bg=-1.0)):
        with pytest.raises(ValueError):
            ens.enable_vertical_mixing(**kw)
    assert ens.vertical_mixing is False and ens.get_vertical_viscosity_batched() is None
    ens.enable_vertical_mixing()
    assert ens.vmix_par == dict(kv_cap=vm.KV_CAP, k_bg=df.K_BG, drag=True)
    with pytest.raises(ValueError, match="one vertical diffusion"):
        ens.enable_diffusion()
    with pytest.raises(ValueError, match="one vertical diffusion"):
        ens.enable_mixing(vertical=True)
    other = lvr.lxr.ensemble_run(eng, 2, True, mixing=None, steps=0)[0]
    other.enable_diffusion()
    other.enable_mixing()
    with pytest.raises(ValueError, match="one vertical diffusion"):
        other.enable_vertical_mixing()
    other.enable_mixing(vertical=True)
    with pytest.raises(ValueError, match="one vertical diffusion"):
        other.enable_vertical_mixing()
    bare = lvr.lxr.ensemble_run(lvr.lxr.MixOracleEngine(), 2, True, steps=0)[0]
    with pytest.raises(ValueError, match="no les_vmix"):
        bare.enable_vertical_mixing()


def test_launches_per_step_and_a_second_read_launches_nothing():
    """never enabled: no les_vmix; enabled: per step one les_vmix behind the step's les_mix, two of them exactly where the cap
    bound; reading the viscosity or the profiles again launches nothing"""
    calls = []

    class Spy(lvr.VmixOracleEngine):
        pass
    for name in ("les_mix", "les_vmix", "slab_means", "les_thermo"):
        def spy(self, *a, _n=name, **kw):
            calls.append(_n)
            return getattr(lvr.VmixOracleEngine, _n)(self, *a, **kw)
        setattr(Spy, name, spy)
    ens, _ = lvr.ensemble_run(Spy(), 2, True, vmix=False)
    assert "les_vmix" not in calls and ens.vertical_mixing is False and calls.count("les_mix") == 3
    for cap, per_step in ((None, 2), (1e6, 1)):
        del calls[:]
        ens, log = lvr.ensemble_run(Spy(), 2, True, cap=cap)
        mine = [k for k in calls if k.startswith("les_")]
        assert mine == (["les_mix"] * per_step + ["les_vmix"]) * 3, mine
        del calls[:]
        kv = ens.get_vertical_viscosity_batched()
        prof = {k: numpy.empty((2, 20)) for k in ("U", "THL")}
        ens.get_profiles_batched(tuple(prof), prof)
        assert ens.get_vertical_viscosity_batched() is kv and not calls
        assert (kv is ens.get_eddy_viscosity_batched()) == (cap is not None)


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant,cap,z0m", [("plain", None, True), ("plain", 1e6, True), ("plain", None, False), ("all", None, True), ("forced", None, True)])
def test_float32_ensemble_equals_the_host_twin(variant, cap, z0m):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    host, capped = lvr.check_ensemble(f32_of(lvr.VmixOracleEngine)(), [f32_of(lvr.VmixOracleEngine)()], 3, variant, cap=cap, z0m=z0m)
    assert (cap is None or not any(capped)) and (cap is not None or variant != "plain" or all(capped))
    assert variant != "forced" or host[-1]["counts"].sum() > 0
