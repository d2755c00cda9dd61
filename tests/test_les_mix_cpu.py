"""K24 without a GPU: the properties of the NumPy oracle of tests/les_mix_ref.py that the kernel inherits by being bit-equal to it
(shared faces, conservation, convexity, the bounds of km), the functions of sp_coupler_amd/mixing.py against hand-computed
values, what Engine.les_mix hands the library, models.DeviceLESEnsemble's enable_mixing() on an oracle-backed engine against its
host twins, and diffusion.profiles' new argument."""
import math

import numpy
import pytest
import torch

from sp_coupler_amd import _abi, mixing, models, spcpl, sputils
from sp_coupler_amd import diffusion as df
from sp_coupler_amd import microphysics
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_full_ref as lfr
from tests import les_mix_ref as lxr
from tests import test_engine_les_args_cpu as args_cpu
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

SHAPES = [(3, 8, 8, 20), (2, 2, 2, 5), (2, 3, 5, 7), (1, 1, 4, 3), (2, 33, 5, 65)]
NPS = [numpy.float64, numpy.float32]


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def cases(shape, dtype):
    """the case of the parity tests, and one with a step so long that the cap binds"""
    return [lxr.case(shape, dtype, seed=3), lxr.case(shape, dtype, seed=4, dt=3600.0)]


# -- the oracle's own properties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_both_cells_of_a_face_form_the_same_flux(shape, dtype):
    for c in cases(shape, dtype):
        km = lxr.oracle(c, ())[0]
        for k in lxr.NAMES:
            fw, fe, fs, fn = lxr.face_fluxes(lxr.field_of(c, k), km, *c["coef"][k])
            assert_bits("fe == fw[ip] " + k, fe, numpy.roll(fw, -1, axis=1))
            assert_bits("fn == fs[jp] " + k, fn, numpy.roll(fs, -1, axis=2))


@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_plane_sums_are_conserved_to_rounding(shape, dtype):
    """out = fl(x + h), h = fl(hx + hy), hx = fl(fe - fw), hy = fl(fn - fs): four roundings per cell and field, each with an error
    of at most u times the COMPUTED value (u = eps / 2, round to nearest); the fluxes themselves are shared by the two cells of a
    face, so their exact sum over a periodic plane is zero.  Hence |sum(out) - sum(x)| <= u * sum(|out| + |h| + |hx| + |hy|) over
    the plane, the difference of the sums taken exactly (ONE math.fsum over the new values and the negated old ones, float64; the
    float32 ones convert exactly)."""
    u = float(numpy.finfo(dtype).eps) / 2
    exact = lambda a: math.fsum(numpy.asarray(a, dtype=numpy.float64).ravel())                 # noqa: E731
    moved = False
    for c in cases(shape, dtype):
        km, _, outs = lxr.oracle(c)
        for k in lxr.NAMES:
            x = lxr.field_of(c, k)
            fw, fe, fs, fn = lxr.face_fluxes(x, km, *c["coef"][k])
            hx, hy = fe - fw, fn - fs
            h = hx + hy
            moved = moved or bool((outs[k] != x).any())
            for l in range(shape[0]):
                for lev in range(shape[3]):
                    p = (l, slice(None), slice(None), lev)
                    bound = u * exact(numpy.abs(outs[k][p]).astype(numpy.float64) + numpy.abs(h[p]) + numpy.abs(hx[p]) + numpy.abs(hy[p]))
                    change = exact(numpy.concatenate([outs[k][p].ravel().astype(numpy.float64), -x[p].ravel().astype(numpy.float64)]))
                    assert abs(change) <= bound * (1 + 1e-9), (k, l, lev, change, bound)
    assert moved or max(shape[1:3]) <= 1


@pytest.mark.parametrize("dtype", NPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_mixed_value_lies_between_the_cell_and_its_neighbours(shape, dtype):
    """at CAP = 0.5 the four face weights sum to at most a half, so out is a convex combination of the five values, up to
    4 eps max|x|; km lies in [0, kcap] and is capped somewhere in the long step"""
    eps = float(numpy.finfo(dtype).eps)
    for c, capped in zip(cases(shape, dtype), (False, True)):
        km, kmax, outs = lxr.oracle(c)
        cap = c["kcap"][:, None, None, None]
        assert (km >= 0).all() and (km <= cap).all() and not numpy.isnan(km).any() and not numpy.signbit(km).any()
        assert (kmax >= km.reshape(shape[0], -1).max(axis=1)).all()
        if capped and shape[3] > 3:
            assert (km == cap).any() and (kmax > c["kcap"]).any()
        for k in lxr.NAMES:
            x = lxr.field_of(c, k)
            five = numpy.stack([x] + [numpy.roll(x, s, axis=ax) for ax in (1, 2) for s in (1, -1)])
            tol = 4 * eps * numpy.abs(x).max()
            assert (outs[k] >= five.min(axis=0) - tol).all() and (outs[k] <= five.max(axis=0) + tol).all(), k


def test_constants_and_extents_of_one_and_two():
    """a constant finite field keeps its bits and a -0.0 constant comes out +0.0; an extent of 1 is its own neighbour, an extent
    of 2 has both neighbours the same cell: the differences across it are +0 and km sees no shear along it"""
    c = lxr.case((2, 4, 5, 6), numpy.float64)
    km = lxr.oracle(c, ())[0]
    for value in (3.25, -0.0):
        x = numpy.full_like(c["u"], value)
        assert_bits("constant", lxr.hmix(x, km, *c["coef"]["QT"]), x + 0)
    for shape in ((2, 1, 1, 5), (2, 2, 2, 5)):
        c = lxr.case(shape, numpy.float32)
        kmh = lxr.eddy(c["u"], c["v"], None, c["gx"], c["gy"], c["gz"], c["bz"], c["l2"], c["kcap"])[0]
        zero = numpy.zeros_like(c["gx"])
        assert_bits("no horizontal shear", kmh, lxr.eddy(c["u"], c["v"], None, zero, zero, c["gz"], c["bz"], c["l2"], c["kcap"])[0])


# -- mixing.py ---------------------------------------------------------------------------------------------------------------------
def test_coefficients_cap_and_profiles_against_hand_computed_values():
    gx, gy, wind, scalar = mixing.coefficients(10.0, 100.0, 200.0, prandtl=0.5, n=2)
    for got, want in ((gx, 0.005), (gy, 0.0025), (wind[0], 5e-4), (wind[1], 1.25e-4), (scalar[0], 1e-3), (scalar[1], 2.5e-4)):
        assert got.shape == (2,) and got.dtype == numpy.float64 and numpy.allclose(got, want, rtol=1e-15, atol=0)
    assert numpy.allclose(mixing.cap(wind, scalar), 100.0, rtol=1e-15) and numpy.allclose(mixing.cap(wind, scalar, cap=0.25), 50.0, rtol=1e-15)
    gx, _, wind, scalar = mixing.coefficients(10.0, numpy.array([100.0, 50.0]), 200.0)
    assert numpy.allclose(gx, [0.005, 0.01]) and numpy.allclose(scalar[0], wind[0] / mixing.PRANDTL) and numpy.allclose(wind[0], [5e-4, 2e-3])
    assert (mixing.CS, mixing.PRANDTL, mixing.KAPPA, mixing.THETA_REF, mixing.CAP) == (0.17, 1 / 3, 0.4, 300.0, 0.5)
    zh, zf = numpy.array([0.0, 20.0, 40.0]), numpy.array([10.0, 30.0, 50.0])
    gz, bz, l2 = mixing.profiles(zf, zh, 20.0, 20.0, cs=0.5, prandtl=0.5, theta_ref=250.0, n=2)
    assert gz.shape == bz.shape == l2.shape == (2, 3)
    assert numpy.allclose(gz, [[1 / 20, 1 / 40, 1 / 20]] * 2, rtol=1e-15)
    assert numpy.allclose(bz, sputils.grav / 125.0 * gz, rtol=1e-15)
    want = [1 / (1 / 100 + 1 / 16), 1 / (1 / 100 + 1 / 144), 1 / (1 / 100 + 1 / 400)]            # Delta = 20, cs Delta = 10, kappa zf = 4, 12, 20
    assert numpy.allclose(l2, [want] * 2, rtol=1e-14)
    gz, bz, l2 = mixing.profiles(numpy.array([10.0]), numpy.array([0.0]), 20.0, 20.0, cs=0.5)
    assert gz.tolist() == [[0.0]] and bz.tolist() == [[0.0]] and numpy.allclose(l2, want[0], rtol=1e-14)
    per_les = mixing.profiles(numpy.stack([zf, 2 * zf]), numpy.stack([zh, 2 * zh]), numpy.array([20.0, 40.0]), 20.0)
    assert numpy.allclose(per_les[0][1], 0.5 * per_les[0][0]) and (per_les[2][1] > per_les[2][0]).all()
    m = numpy.array([[1.0, 3.0, 7.0]])
    assert mixing.face_diffusivity(m, 0.1).tolist() == [[1.1, 2.1, 5.1]]


def test_refusals_of_the_host_module():
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for call in (lambda: mixing.coefficients(bad, 100.0, 100.0), lambda: mixing.coefficients(1.0, bad, 100.0),
                     lambda: mixing.coefficients(1.0, 100.0, bad), lambda: mixing.coefficients(1.0, 100.0, 100.0, prandtl=bad),
                     lambda: mixing.profiles([10.0, 30.0], [0.0, 20.0], 100.0, 100.0, cs=bad),
                     lambda: mixing.profiles([10.0, 30.0], [0.0, 20.0], 100.0, 100.0, prandtl=bad),
                     lambda: mixing.profiles([10.0, 30.0], [0.0, 20.0], bad, 100.0),
                     lambda: mixing.profiles([10.0, 30.0], [0.0, 20.0], 100.0, numpy.array([100.0, bad])),
                     lambda: mixing.cap((1.0, 1.0), (1.0, 1.0), cap=bad)):
            with pytest.raises(ValueError, match="K24"):
                call()
    with pytest.raises(ValueError):
        mixing.profiles([30.0, 10.0], [20.0, 0.0], 100.0, 100.0)          # levels that do not ascend


# -- Engine.les_mix: what the library is handed ------------------------------------------------------------------------------------
# (tests/fake_engine.py's OracleEngine computes with the oracle and has no argument block to look at; the checks that Engine.les_mix
# makes are looked at on ``Recorder`` of tests/test_engine_les_args_cpu.py, the real Engine on host tensors whose ``_call`` records
# the block and launches nothing, as for K10 to K23.  The oracle-backed engine of this kernel is tests/les_mix_ref.MixOracleEngine.)
def mix_case(dtype, shape=args_cpu.SHAPE):
    n, _, _, ktot = shape
    f4, prof, vec = args_cpu.f4, args_cpu.prof, lambda: torch.rand(n, dtype=dtype)            # noqa: E731
    t = dict(u=f4(dtype, shape), v=f4(dtype, shape), theta=f4(dtype, shape), gx=vec(), gy=vec(), gz=prof(dtype, n, ktot),
             bz=prof(dtype, n, ktot), l2=prof(dtype, n, ktot), kcap=vec(), km=f4(dtype, shape))
    fields = {"U": t["u"], "QT": f4(dtype, shape)}
    out = {k: f4(dtype, shape) for k in fields}
    wind, scalar = (vec(), vec()), (vec(), vec())
    return t, fields, out, {"U": wind[0], "QT": scalar[0]}, {"U": wind[1], "QT": scalar[1]}


@pytest.mark.parametrize("dtype", args_cpu.DTYPES)
def test_engine_argument_block_and_refusals(dtype):
    eng = args_cpu.Recorder(dtype)
    t, fields, out, ax, ay = mix_case(dtype)
    call = lambda fields=fields, out=out, ax=ax, ay=ay, kmax=True, **kw: eng.les_mix(                      # noqa: E731
        fields, out, *[dict(t, **kw)[k] for k in ("u", "v", "theta", "gx", "gy", "gz", "bz", "l2", "kcap", "km")], ax, ay, kmax=kmax)
    top = torch.zeros(2, dtype=dtype)
    assert call(kmax=top) is top
    ptr = lambda d: [d[k].data_ptr() for k in fields]                                           # noqa: E731
    want = dict(n_les=2, itot=2, jtot=3, ktot=8, n_fields=2, pitch_prof=args_cpu.PITCH, fields=ptr(fields), out=ptr(out), ax=ptr(ax), ay=ptr(ay),
                **{k: x.data_ptr() for k, x in t.items()})
    assert eng.last(_abi.LesMixArgs) == ("spc_les_mix_" + args_cpu.sfx(dtype), args_cpu.members(_abi.LesMixArgs, kmax=top.data_ptr(), **want))
    got = call()
    assert tuple(got.shape) == (2,) and got.dtype == dtype
    assert eng.last(_abi.LesMixArgs)[1] == args_cpu.members(_abi.LesMixArgs, kmax=got.data_ptr(), **want)
    assert call(kmax=False) is None
    assert eng.last(_abi.LesMixArgs)[1] == args_cpu.members(_abi.LesMixArgs, **want)
    assert call(theta=None, bz=None, kmax=None) is None
    assert eng.last(_abi.LesMixArgs)[1] == args_cpu.members(_abi.LesMixArgs, **dict(want, theta=None, bz=None))
    assert call(fields={}, out={}, ax={}, ay={}) is not None                                   # the probe
    probe = eng.last(_abi.LesMixArgs)[1]
    assert probe["n_fields"] == 0 and probe["fields"] == [None] * 6 and probe["km"] == t["km"].data_ptr()
    alias = "les_mix: km, kmax or an output is an input or another of them"
    seven = {str(i): fields["QT"] for i in range(7)}
    args_cpu.refused(eng, [lambda: call(fields=seven, out=seven, ax=seven, ay=seven), lambda: call(out={"U": out["U"]}),
                           lambda: call(ax={"U": ax["U"], "X": ax["QT"]}), lambda: call(bz=None), lambda: call(km=t["u"]),
                           lambda: call(km=fields["QT"]), lambda: call(out={"U": out["QT"], "QT": out["QT"]}),
                           lambda: call(out={"U": t["km"], "QT": out["QT"]}), lambda: call(kmax=t["gx"]), lambda: call(kmax=ay["QT"]),
                           lambda: call(kmax=torch.zeros(3, dtype=dtype)), lambda: call(gx=t["gx"][:1])],
                     ["les_mix takes at most 6 fields per launch, got 7", "les_mix: out holds ['U'], the fields are ['QT', 'U']",
                      "les_mix: ax holds ['U', 'X'], the fields are ['QT', 'U']", "les_mix: theta without bz", alias, alias, alias, alias, alias,
                      alias, "kmax must be a contiguous vector of 2, got (3,)", "gx must be a contiguous vector of 2, got (1,)"])


def test_row_blocks_of_a_multi_engine_equal_one_engine():
    """MultiDeviceEngine.les_mix over Sharded row blocks 4 + 3 and 1 + 1 + 0, on oracle-backed engines"""
    for engines, n, blocks in ((2, 7, [4, 3]), (3, 2, [1, 1, 0])):
        multi = MultiDeviceEngine([lxr.MixOracleEngine() for _ in range(engines)], min_cols_per_device=1)
        assert lxr.check_multi(lxr.MixOracleEngine(), multi, n) == blocks


# -- the ensemble ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vertical", [("plain", False), ("all", False), ("all", True), ("forced", True)])
def test_ensemble_equals_the_host_twin(variant, vertical):
    """three steps and a constantT nudge before the last, plain and with diffusion + radiation + thermo + microphysics +
    conservative second-order transport, with K15 taking K24's viscosity and without, and ("forced") with K19's strong forcing
    in front of the step and K21 in front of every substep: every profile, field, km (and K19's counts) bit-equal to
    the host twin after each of them; enable_mixing() changes U, and a run that never calls it is bit-equal to
    tests/les_full_ref's twin (both asserted in check_ensemble)"""
    host = lxr.check_ensemble(lxr.MixOracleEngine(), [lxr.MixOracleEngine()], 3, variant, vertical)
    assert host[-1]["k max"][1] in (0.0, 1.0)
    assert variant != "forced" or host[-1]["counts"].sum() > 0        # K19 ran, in the twin and (bit-equal) on the device


def test_vertical_changes_the_diffusion_and_only_then():
    plain = lxr.ensemble_run(lxr.MixOracleEngine(), 3, False, **lxr.VARIANTS["all"])[1]
    vert = lxr.ensemble_run(lxr.MixOracleEngine(), 3, False, vertical=True, **lxr.VARIANTS["all"])[1]
    assert (plain[-1]["field THL"] != vert[-1]["field THL"]).any()


def test_enable_mixing_refusals_and_defaults():
    eng = lxr.MixOracleEngine()
    ens = lxr.ensemble_run(eng, 2, True, mixing=None, steps=0)[0]
    with pytest.raises(ValueError, match="enable_diffusion"):
        ens.enable_mixing(vertical=True)
    for kw in (dict(cs=0.0), dict(prandtl=-1.0), dict(cap=0.0), dict(theta_ref=float("nan")), dict(dx=0.0), dict(dy=-5.0)):
        with pytest.raises(ValueError, match="K24"):
            ens.enable_mixing(**kw)
    assert ens.mixing is False and ens.get_eddy_viscosity_batched() is None
    ens.enable_mixing()
    assert (ens.mix_par["dx"], ens.mix_par["dy"], ens.mix_par["cs"], ens.mix_par["cap"]) == (200.0, 200.0, mixing.CS, mixing.CAP)
    ens.enable_advection(dx=150.0, dy=300.0)
    ens.enable_mixing()
    assert (ens.mix_par["dx"], ens.mix_par["dy"]) == (150.0, 300.0)
    ens.enable_mixing(dx=120.0)
    assert (ens.mix_par["dx"], ens.mix_par["dy"]) == (120.0, 300.0)
    bare = models.DeviceLESEnsemble.for_gcm(models.BatchedSyntheticGCM(4, 19, 21), numpy.arange(1, 3), nL=8, engine=eng)
    with pytest.raises(ValueError, match="U and V"):
        bare.enable_mixing()


def test_uploads_are_kept_until_their_inputs_change():
    """the profiles are uploaded once; the coefficients again when dt changes"""
    ens = lxr.ensemble_run(lxr.MixOracleEngine(), 2, True, steps=0)[0]
    ens.evolve_model_batched(ens.model_time + 60.0)
    prof, coef = ens._mix_prof, ens._mix_coef
    ens.evolve_model_batched(ens.model_time + 60.0)
    assert ens._mix_prof is prof and ens._mix_coef is coef
    ens.evolve_model_batched(ens.model_time + 30.0)
    assert ens._mix_prof is prof and ens._mix_coef is not coef
    ens.enable_mixing(cs=0.2)
    ens.evolve_model_batched(ens.model_time + 30.0)
    assert ens._mix_prof is not prof


# -- diffusion.profiles(kd=None) ---------------------------------------------------------------------------------------------------
def matrix_before(zh, zf, rhobf, dt, k_max, h_mix, k_bg):
    """diffusion.matrix as it was before the argument ``kd``"""
    rhobf = numpy.atleast_2d(numpy.asarray(rhobf, dtype=numpy.float64))
    shape = rhobf.shape
    dz = numpy.broadcast_to(microphysics.layer_thickness(zh, zf), shape)
    zh = numpy.broadcast_to(numpy.asarray(zh, dtype=numpy.float64), shape)
    zf = numpy.broadcast_to(numpy.asarray(zf, dtype=numpy.float64), shape)
    w = rhobf * dz
    g = numpy.zeros(shape)
    kd = df.diffusivity(zh[..., 1:], k_max, h_mix, k_bg)
    g[..., 1:] = 0.5 * (rhobf[..., 1:] + rhobf[..., :-1]) * kd / (zf[..., 1:] - zf[..., :-1])
    a = -float(dt) * g / w
    c = numpy.zeros(shape)
    c[..., :-1] = -float(dt) * g[..., 1:] / w[..., :-1]
    return a, 1.0 - a - c, c, w, dz


def test_diffusion_profiles_without_kd_are_what_they_were():
    rng = numpy.random.default_rng(5)
    rhobf, zh, zf, _, _ = lxr.lrr.grid(3, 12, rng)
    for got, want in zip(df.matrix(zh, zf, rhobf, 60.0), matrix_before(zh, zf, rhobf, 60.0, df.K_MAX, df.H_MIX, df.K_BG)):
        assert_bits("matrix", got, want)
    today = df.profiles(zh, zf, rhobf, 60.0)
    for tag, other in (("kd=None", df.profiles(zh, zf, rhobf, 60.0, kd=None)),
                       ("kd of the profile", df.profiles(zh, zf, rhobf, 60.0, kd=df.diffusivity(zh)))):
        for got, want in zip(other, today):
            assert_bits(tag, got, want)
    kd = df.diffusivity(zh)
    kd[:, 0] = -1.0                                                   # the ground's entry is not read
    assert_bits("face 0", df.profiles(zh, zf, rhobf, 60.0, kd=kd)[1], today[1])
    assert (df.profiles(zh, zf, rhobf, 60.0, kd=2.0 * df.diffusivity(zh))[1] != today[1]).any()
    with pytest.raises(ValueError, match="kd"):
        df.profiles(zh, zf, rhobf, 60.0, kd=-df.diffusivity(zh))


def test_never_enabled_is_the_full_twin():
    """a device run that never calls enable_mixing() launches no les_mix"""
    calls = []

    class Spy(lxr.MixOracleEngine):
        def les_mix(self, *a, **kw):
            calls.append("les_mix")
            return super().les_mix(*a, **kw)
    ens, log = lxr.ensemble_run(Spy(), 2, True, mixing=None, **lxr.VARIANTS["all"])
    assert not calls and ens.mixing is False
    lxr.lmr.same_logs(lxr.ensemble_run(lfr.FullOracleEngine(), 2, False, mixing=None, **lxr.VARIANTS["all"])[1], log)
    ens, log = lxr.ensemble_run(Spy(), 2, True, **lxr.VARIANTS["all"])
    assert calls == ["les_mix"] * 3


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vertical", [("plain", False), ("all", False), ("all", True), ("forced", True)])
def test_float32_ensemble_equals_the_host_twin(variant, vertical):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    host = lxr.check_ensemble(f32_of(lxr.MixOracleEngine)(), [f32_of(lxr.MixOracleEngine)()], 3, variant, vertical)
    assert host[-1]["k max"][1] in (0.0, 1.0)
    assert variant != "forced" or host[-1]["counts"].sum() > 0        # K19 ran, in the twin and (bit-equal) on the device
