"""K23 without a GPU: properties of the NumPy oracle of tests/les_transport2_ref.py (the lid budget, constants, the 1-D TVD
bound of the MC limiter, second-order accuracy on a sine, the stability of a 3-D closed cell, the reduction to K22 where every
slope is zero, the bit identity of the two cells of a face), the struct layout and the host-side refusals of
spc_les_transport2_*, and DeviceLESEnsemble's enable_advection(..., conservative=True, order=2) on an oracle-backed engine
against its host twins."""
import ctypes
import os
import subprocess

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import advection as adv
from tests import les_transport2_ref as lt2
from tests import les_transport_ref as ltr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {numpy.float64: 2.0 ** -52, numpy.float32: 2.0 ** -23}
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 1, 2), (2, 2, 7), (3, 5, 64), (4, 3, 5), (8, 8, 40), (5, 33, 9)]          # itot x jtot x ktot


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


def shaped(shape, dtype, n=2, seed=0, names=("THL", "QT")):
    itot, jtot, ktot = shape
    return lt2.case((n, itot, jtot, ktot), dtype, seed=seed, names=names)


# -- 1. the budget and constants ---------------------------------------------------------------------------------------------------
def budget_case(dtype, seed=0):
    """K22's budget case: 3 LES of 8 x 8 x 40, random winds of 3 m/s, hx = hy = 0.005, THL and QT; outflow sums of about 0.1"""
    T = numpy.dtype(dtype).type
    shape = (3, 8, 8, 40)
    rng = numpy.random.default_rng(220 + seed)
    u, v = (3.0 * rng.standard_normal(shape)).astype(T), (3.0 * rng.standard_normal(shape)).astype(T)
    g, r = ltr.profiles(3, 40, T)
    return dict(u=u, v=v, fields={k: lt2.field_like(k, shape, T, rng) for k in ("THL", "QT")}, hx=numpy.full(3, 0.005, dtype=T),
                hy=numpy.full(3, 0.005, dtype=T), g=g, r=r)


@pytest.mark.parametrize("limiter", lt2.LIMITERS)
@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_budget_with_random_winds(dtype, limiter):
    """|sum g x' + sum ftop - sum g x| <= 8 eps_T sum g |x| per LES and field, the bound of K22's CPU test, the sums in float64 by
    math.fsum (advection.lid_budget); the step is neither the identity nor K22's"""
    c = budget_case(dtype)
    new, cmax, _, ftop = lt2.oracle(c, limiter)
    first = ltr.oracle(c)[0]
    assert 0 < cmax.max() <= 1.0
    for k, x in c["fields"].items():
        res, scale = adv.lid_budget(c["g"], x, new[k], ftop[k])
        print("budget %s %s %s: %s eps of sum g |x|, cmax %.3g" % (limiter, numpy.dtype(dtype).name, k, numpy.abs(res) / scale / EPS[dtype], cmax.max()))
        assert (numpy.abs(res) <= 8 * EPS[dtype] * scale).all() and (new[k] != x).any() and (new[k] != first[k]).any() and ftop[k].any()


@pytest.mark.parametrize("limiter", lt2.LIMITERS)
@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_keeps_a_constant_to_rounding(shape, dtype, limiter):
    """Every difference of a constant is +0, so every slope and every correction is a zero and the step is K22's: at an outflow
    sum s <= 1 the value is x (1 - [(ce - cw) + (cn - cs)] - r (Mt - Mb)), whose bracket is zero up to the one rounding of
    Mt = Mb - e and the three of e.  Counted per cell: six flux products, five differences and sums of fluxes, the product with
    r and the two final subtractions, 14 roundings of relative size eps / 2 acting on terms of at most |x| (s <= 1), and at most
    two more from continuity: 16 (eps / 2) |x| = 8 eps |x|.  (The prototype saw 2 eps.)"""
    c = ltr.scaled(shaped(shape, dtype)) if min(shape[:2]) > 2 or shape[2] > 1 else shaped(shape, dtype)
    const = {"a": numpy.full_like(c["u"], 287.3), "b": numpy.full_like(c["u"], -1e-3)}
    kept, cmax, _, _ = lt2.les_transport2(const, c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"], limiter)
    first = ltr.les_transport(const, c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])[0]
    assert cmax.max() <= 1.0 and cmax.dtype == dtype
    for k, x in const.items():
        err = numpy.abs(kept[k].astype(numpy.float64) - x.astype(numpy.float64)).max() / abs(float(x.flat[0]))
        print("constant %s %s %s %s: %.3g eps" % (shape, numpy.dtype(dtype).name, limiter, k, err / EPS[dtype]))
        assert err <= 8 * EPS[dtype]
        assert numpy.array_equal(kept[k], first[k])                  # (equal values: the sign of a zero may differ)


# -- 2. the 1-D TVD bound ----------------------------------------------------------------------------------------------------------
def row_case(x, c, dtype=numpy.float64):
    """a periodic row carried by a uniform wind at the Courant number c: jtot = ktot = 1, cw = (u + u) hx = c"""
    T = numpy.dtype(dtype).type
    N = x.size
    u = numpy.ones((1, N, 1, 1), dtype=T)
    return dict(u=u, v=numpy.zeros_like(u), fields={"x": x.astype(T).reshape(1, N, 1, 1)}, hx=numpy.array([0.5 * c], dtype=T),
                hy=numpy.array([0.0], dtype=T), g=numpy.ones((1, 1), dtype=T), r=numpy.ones((1, 1), dtype=T))


def carry(case, steps, step):
    x = case["fields"]["x"]
    for _ in range(steps):
        x = step(dict(case, fields={"x": x}))["x"]
    return x[0, :, 0, 0]


DONOR = lambda c: ltr.oracle(c)[0]                                                         # noqa: E731
MC = lambda c: lt2.oracle(c, "mc")[0]                                                      # noqa: E731
NONE = lambda c: lt2.oracle(c, "none")[0]                                                  # noqa: E731


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("c", [0.25, 0.5, 0.8, -0.5])
def test_mc_creates_no_value_outside_the_cell_and_its_two_neighbours(c, dtype):
    """1-D, uniform wind, MC: every new value lies within the range of the cell and its two neighbours; 8 eps max|x| cover the
    roundings of the update (the float64 prototype needed 0).  A square wave, a spike and noise, 40 steps each"""
    rng = numpy.random.default_rng(3)
    N = 48
    x0 = numpy.where((numpy.arange(N) // 6) % 2 == 0, 1.0, -0.25) + numpy.where(numpy.arange(N) == 29, 5.0, 0.0)
    for x in (x0, rng.standard_normal(N)):
        case = row_case(x, c, dtype)
        cur = case["fields"]["x"]
        assert abs(float(lt2.face_numbers(case["u"], case["v"], case["hx"], case["hy"], case["g"], case["r"])["s"].max()) - abs(c)) < 1e-6
        worst = 0.0
        for _ in range(40):
            new = MC(dict(case, fields={"x": cur}))["x"]
            nb = numpy.stack([cur, numpy.roll(cur, 1, axis=1), numpy.roll(cur, -1, axis=1)])
            e = 8 * EPS[dtype] * numpy.abs(cur).max()
            worst = max(worst, float(numpy.maximum(new - nb.max(axis=0), nb.min(axis=0) - new).max()))
            assert (new <= nb.max(axis=0) + e).all() and (new >= nb.min(axis=0) - e).all()
            cur = new
        print("TVD c %g %s: largest excursion %.3g" % (c, numpy.dtype(dtype).name, worst))
        assert (cur != case["fields"]["x"]).any()


def test_the_unlimited_scheme_is_not_monotone():
    """what the limiter is for: the same square wave leaves its range without it"""
    x0 = numpy.where((numpy.arange(48) // 6) % 2 == 0, 1.0, -0.25)
    x = carry(row_case(x0, 0.5), 10, NONE)
    assert x.max() > 1.0 + 1e-3 and x.min() < -0.25 - 1e-3


# -- 3. accuracy ---------------------------------------------------------------------------------------------------------------
def sine_error(N, c, step):
    """the largest error after a sine was carried once round a periodic row of N cells in N / c steps"""
    steps = int(round(N / c))
    assert steps * c == N
    x0 = numpy.sin(2.0 * numpy.pi * numpy.arange(N) / N)
    return float(numpy.abs(carry(row_case(x0, c), steps, step) - x0).max())


@pytest.mark.parametrize("c", [0.25, 0.5])
def test_second_order_on_a_sine(c):
    """one period on rows of 32, 64 and 128 cells in float64: MC's error is at most a quarter of the donor cell's (the
    prototype's worst ratio was 1 / 7.1), and the unlimited scheme's error falls by at least 3.5 per doubling (4.1 to 8.0)"""
    err = {N: (sine_error(N, c, DONOR), sine_error(N, c, NONE), sine_error(N, c, MC)) for N in (32, 64, 128)}
    for N, (d, u, m) in err.items():
        print("sine N %d c %g: donor %.2e unlimited %.2e mc %.2e, mc / donor 1 / %.1f" % (N, c, d, u, m, d / m))
        assert m <= 0.25 * d and u < m
    for N in (32, 64):
        print("sine c %g: unlimited %d -> %d falls by %.2f" % (c, N, 2 * N, err[N][1] / err[2 * N][1]))
        assert err[N][1] >= 3.5 * err[2 * N][1]


# -- 4. stability in 3-D ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_closed_cell_stays_inside_its_initial_range(dtype):
    """the 3-D closed cell (n = 2, 8 x 8 x 40, v = 0.7 u transposed) at an outflow Courant sum of 0.5, the ensemble's default
    cfl, with MC: 400 steps stay finite and inside the initial range of the field"""
    c = lt2.closed_cell_3d(dtype)
    assert abs(float(lt2.face_numbers(c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])["s"].max()) - 0.5) < 1e-3
    x0 = c["fields"]["QT"]
    lo, hi = x0.min(), x0.max()
    x = x0
    for _ in range(400):
        x = lt2.les_transport2({"QT": x}, c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"], "mc")[0]["QT"]
    print("closed cell %s: [%.6g, %.6g] within [%.6g, %.6g]" % (numpy.dtype(dtype).name, x.min(), x.max(), lo, hi))
    assert numpy.isfinite(x).all() and x.min() >= lo and x.max() <= hi and (x != x0).any()


# -- 5. the smooth limit and the shared faces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_zero_slopes_give_the_donor_cell_result(dtype):
    """a field whose every cell is an extremum along each axis (a checkerboard) has MC slopes of +0 everywhere: every correction
    is a zero and the step is K22's up to the sign of zero; so is, with both limiters, the step of a plane of extent 1 or 2 with
    one level"""
    c = shaped((4, 6, 8), dtype, seed=3)
    n, i, j, k = numpy.indices(c["u"].shape)
    board = {"x": (290.0 + 3.0 * ((i + j + k) % 2)).astype(dtype)}
    si, sj, sk = lt2.slopes(board["x"], "mc")
    assert not si.any() and not sj.any() and not sk.any()
    args = (c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])
    got, first = lt2.les_transport2(board, *args, "mc"), ltr.les_transport(board, *args)
    assert numpy.array_equal(got[0]["x"], first[0]["x"]) and numpy.array_equal(got[3]["x"], first[3]["x"])
    for plane in ((1, 1), (1, 2), (2, 1), (2, 2)):
        c = shaped(plane + (1,), dtype, seed=4)
        args = (c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])
        want = ltr.les_transport(c["fields"], *args)[0]
        got = lt2.les_transport2(c["fields"], *args, "mc")[0]
        assert all(numpy.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("limiter", lt2.LIMITERS)
@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_bit_identities(shape, dtype, limiter):
    """cmax and mtop are K22's bit for bit; the second-order flux through a face has the same bits in both cells that share it;
    the ground is closed; the slope is +0 at the lowest and the highest level"""
    c = shaped(shape, dtype, seed=2)
    new, cmax, mtop, ftop = lt2.oracle(c, limiter)
    _, cmax1, mtop1, _ = ltr.oracle(c)
    assert_bits("cmax", cmax, cmax1)
    assert_bits("mtop", mtop, mtop1)
    nums = lt2.face_numbers(c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])
    for k, x in c["fields"].items():
        Fw, Fe, Fs, Fn, Fb, Ft = lt2.fluxes2(x, nums, c["r"], limiter)
        assert_bits("Fe2 of i is Fw2 of ip", Fe, numpy.roll(Fw, -1, axis=1))
        assert_bits("Fn2 of j is Fs2 of jp", Fn, numpy.roll(Fs, -1, axis=2))
        assert_bits("Ft2 of k is Fb2 of k + 1", Ft[..., :-1], Fb[..., 1:])
        assert not Fb[..., 0].any()
        assert_bits("ftop", ftop[k], Ft[..., -1])
        sk = lt2.slopes(x, limiter)[2]
        assert not sk[..., 0].any() and not sk[..., -1].any() and not numpy.signbit(sk[..., 0]).any() and not numpy.signbit(sk[..., -1]).any()


@pytest.mark.parametrize("limiter", lt2.LIMITERS)
@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_special_values(dtype, limiter):
    c, s, mask = lt2.special_case(dtype)
    clean, got = lt2.oracle(c, limiter), lt2.oracle(s, limiter)
    assert_bits("THL", got[0]["THL"][~mask], clean[0]["THL"][~mask])
    assert_bits("QT", got[0]["QT"], clean[0]["QT"])
    assert numpy.isnan(got[0]["THL"][0, 0, 0, 1]) and numpy.isfinite(got[1]).all()


# -- plumbing --------------------------------------------------------------------------------------------------------------------
def test_struct_layout_of_the_transport2_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror; K22's members come first, in K22's order"""
    cls, cname = _abi.LesTransport2Args, "spc_les_transport2_args"
    fields = [f[0] for f in _abi.LesTransportArgs._fields_] + ["limiter"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_LIMITER_NONE);', 'printf("%d\\n", SPC_LIMITER_MC);']
    want = [ctypes.sizeof(cls), _abi.SPC_LIMITER_NONE, _abi.SPC_LIMITER_MC]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    for f in fields[:-1]:
        lines.append('printf("%%zu\\n", offsetof(spc_les_transport_args, %s));' % f)
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and (_abi.SPC_LIMITER_NONE, _abi.SPC_LIMITER_MC) == (0, 1) and _abi.LIMITERS == {"none": 0, "mc": 1}


PTRS = ("u", "v", "hx", "hy", "cmax", "g", "r", "mtop", "ftop")


def _args(n=4, itot=8, jtot=8, ktot=20, n_fields=4, pitch_prof=None, limiter=1, fields=None, out=None, **ptrs):
    a = _abi.LesTransport2Args()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.limiter = n, itot, jtot, ktot, n_fields, limiter
    a.pitch_prof = ktot if pitch_prof is None else pitch_prof
    for i, k in enumerate(PTRS):                                  # distinct, 16-byte aligned, never dereferenced
        setattr(a, k, ptrs.get(k, 4096 * (i + 1)))
    for f in range(6):
        a.fields[f] = (fields or {}).get(f, 4096 * (f + 10))
        a.out[f] = (out or {}).get(f, 4096 * (f + 20))
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_transport2_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    for bad in (2, -1, 1 << 20):
        for nf in (4, 0):
            rc, text = call(limiter=bad, n_fields=nf)
            assert rc == E and b"limiter" in text
    for k in ("u", "v", "hx", "hy", "g", "r"):
        assert call(**{k: None}) == (E, b"required pointer %s is NULL" % k.encode())
    assert call(fields={1: None})[0] == E and b"fields" in lib.spc_last_error()
    assert call(out={3: None})[0] == E and b"out" in lib.spc_last_error()
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    for nf in (7, -1):
        rc, text = call(n_fields=nf)
        assert rc == E and b"field count" in text
    rc, text = call(n_fields=0, cmax=None, mtop=None)
    assert rc == E and b"nothing to do" in text
    rc, text = call(pitch_prof=19)
    assert rc == E and b"pitch_prof" in text
    rc, text = call(out={3: 4096 * 20})
    assert rc == E and b"same array" in text
    for ptr in (4096, 4096 * 10):
        for kw in (dict(out={2: ptr}), dict(mtop=ptr), dict(cmax=ptr), dict(ftop=ptr)):
            rc, text = call(**kw)
            assert rc == E and b"also an input" in text, kw
    rc, text = call(fields={0: 4100 if sfx == "f64" else 4098})
    assert rc == E and b"not aligned" in text
    for limiter in (0, 1):
        rc, text = call(n=1 << 40, ktot=3, limiter=limiter)
        assert rc == U and b"too many workgroups" in text
    rc, text = call(ktot=2560 if sfx == "f32" else 1280, pitch_prof=4000)
    assert rc == U and b"levels" in text
    a = _args(n=0, fields={f: None for f in range(6)}, out={f: None for f in range(6)}, **{k: None for k in PTRS})
    assert fn(ctypes.byref(a), None) == 0                         # an empty ensemble is a no-op


def test_columns_per_block_are_the_first_order_kernels(lib):
    for esize in (4, 8):
        for ktot in (1, 2, 63, 64, 65, 127, 128, 129, 160, 255, 256, 257, 511, 512, 513, 1279, 1280, 2559, 2560, 5000):
            assert lib.spc_les_transport2_cols_per_block(ktot, esize) == lib.spc_les_transport_cols_per_block(ktot, esize), (ktot, esize)
    assert lib.spc_les_transport2_cols_per_block(0, 8) == 0 and lib.spc_les_transport2_cols_per_block(160, 2) == 0


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    assert callable(Engine.les_transport2) and callable(MultiDeviceEngine.les_transport2) and callable(Engine.transport2_cols_per_block)
    assert not hasattr(ltr.TransportOracleEngine, "les_transport2")


# -- 6. the ensemble ---------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    for name in ("les_advect", "les_vadvect", "les_transport", "les_transport2", "les_buoyancy"):
        inner = getattr(engine, name)
        if name == "les_buoyancy":
            setattr(engine, name, lambda *a, _f=inner, **kw: (calls.append(("les_buoyancy", None, int(a[0].shape[0]))), _f(*a, **kw))[1])
        else:
            setattr(engine, name, lambda fields, *a, _n=name, _f=inner, **kw: (calls.append((_n, sorted(fields), int(a[1].shape[0]))), _f(fields, *a, **kw))[1])
    return engine


@pytest.mark.parametrize("variant,limiter", [("plain", "mc"), ("plain", "none"), ("buoyancy", "mc"), ("all buoyant", "mc")])
def test_ensemble_on_one_engine_equals_the_host_twin(variant, limiter):
    """three steps against the twin; per step ONE K22 probe, then per substep K21 where enabled and ONE K23: 1 + n_sub launches,
    and no K16, K17 or K22 field launch; order=1 afterwards is K22's path"""
    calls = []
    subs = lt2.check_ensemble(lt2.Transport2OracleEngine(), [_counted(lt2.Transport2OracleEngine(), calls)], 4, variant, limiter)
    kw = lt2.VARIANTS[variant]
    keys = sorted(["QT", "THL", "U", "V"] + (["QR"] if kw.get("micro") else []))
    assert len(subs) == 3 and all(s >= 1 for s in subs)
    want = []
    for n_sub in subs:
        want += [("les_transport", [], 4)] + (([("les_buoyancy", None, 4)] if kw.get("buoyancy") else []) + [("les_transport2", keys, 4)]) * n_sub
    assert calls[:len(want)] == want                               # the second-order run came first
    rest = calls[len(want):]                                       # then order=1 and the call without the arguments
    assert rest and all(c[0] in ("les_transport", "les_buoyancy") for c in rest) and any(c[0] == "les_transport" and c[1] for c in rest)


def test_ensemble_as_row_blocks_with_an_empty_device():
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(lt2.Transport2OracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    subs = lt2.check_ensemble(lt2.Transport2OracleEngine(), [multi], 2, "plain")
    assert all(c[2] == 1 for c in calls) and len([c for c in calls if c[0] == "les_transport2"]) == 2 * sum(subs)   # blocks 1 + 1 + 0


def _small(eng, n=2, nL=6):
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(n, nL=nL)
    ens = models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)
    rng = numpy.random.default_rng(1)
    ens.attach_fields({k: rng.standard_normal((2, 2, 3, 6)) + m for k, m in (("U", 5.0), ("V", -2.0), ("THL", 290.0), ("QT", 5.0))})
    return ens


def test_ensemble_arguments():
    """order=2 without conservative=True, an order that is neither 1 nor 2, an unknown limiter and an engine without
    les_transport2 are ValueErrors; order=1 is K22's path with K22's bits whatever the limiter; order=2 launches K23"""
    eng = lt2.Transport2OracleEngine()
    ens = _small(eng)
    kw = dict(dx=50000.0, dy=50000.0, vertical=True)
    with pytest.raises(ValueError, match="conservative=True"):
        ens.enable_advection(order=2, **kw)
    with pytest.raises(ValueError, match="conservative=True"):
        ens.enable_advection(dx=50000.0, dy=50000.0, order=2)
    with pytest.raises(ValueError, match="order"):
        ens.enable_advection(conservative=True, order=3, **kw)
    with pytest.raises(ValueError, match="order"):
        ens.enable_advection(conservative=True, order=0, **kw)
    with pytest.raises(ValueError, match="limiter"):
        ens.enable_advection(conservative=True, order=2, limiter="minmod", **kw)
    with pytest.raises(ValueError, match="limiter"):
        ens.enable_advection(conservative=True, limiter=None, **kw)
    old = _small(ltr.TransportOracleEngine())
    old.enable_advection(conservative=True, **kw)
    with pytest.raises(ValueError, match="les_transport2"):
        old.enable_advection(conservative=True, order=2, **kw)
    assert old.advect_order == 1 and old.advect_conservative              # (a refused call changes nothing)
    results = {}
    for tag, extra in (("default", {}), ("order 1", dict(order=1, limiter="none")), ("order 2", dict(order=2)), ("order 2 none", dict(order=2, limiter="none"))):
        calls = []
        ens = _small(_counted(lt2.Transport2OracleEngine(), calls))
        ens.enable_advection(conservative=True, cfl=0.004, **dict(kw, **extra))
        assert (ens.advect_order, ens.advect_limiter) == (extra.get("order", 1), extra.get("limiter", "mc"))
        ens.evolve_model_batched(100.0)
        names = [c[0] for c in calls]
        field = "les_transport2" if extra.get("order") == 2 else "les_transport"
        assert names == ["les_transport"] + [field] * ens.advect_substeps and ens.advect_substeps > 1 and not calls[0][1]
        results[tag] = {k: ens.get_fields_batched(k).numpy().copy() for k in ("U", "THL", "QT")}
        results[tag]["lid"] = ens.get_lid_flux_batched()["THL"].numpy().copy()
    for k, x in results["default"].items():
        assert_bits("order=1 is today's run: " + k, results["order 1"][k], x)
        assert (results["order 2"][k] != x).any() and (results["order 2 none"][k] != results["order 2"][k]).any()


def test_a_courant_sum_that_is_not_finite_raises():
    eng = lt2.Transport2OracleEngine()
    ens = _small(eng)
    ens.enable_advection(dx=50000.0, dy=50000.0, vertical=True, conservative=True, order=2)
    inner = eng.les_transport2
    eng.les_transport2 = lambda fields, *a, **kw: inner(fields, *a, **kw).fill_(float("inf"))
    with pytest.raises(RuntimeError, match="Courant sum"):
        ens.evolve_model_batched(100.0)
    assert ens.advect_courant == float("inf")


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant,limiter", [("plain", "mc"), ("plain", "none"), ("buoyancy", "mc"), ("all buoyant", "mc")])
def test_float32_ensemble_on_one_engine_equals_the_host_twin(variant, limiter):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    calls = []
    subs = lt2.check_ensemble(f32_of(lt2.Transport2OracleEngine)(), [_counted(f32_of(lt2.Transport2OracleEngine)(), calls)], 4, variant, limiter)
    kw = lt2.VARIANTS[variant]
    keys = sorted(["QT", "THL", "U", "V"] + (["QR"] if kw.get("micro") else []))
    assert len(subs) == 3 and all(s >= 1 for s in subs)
    want = []
    for n_sub in subs:
        want += [("les_transport", [], 4)] + (([("les_buoyancy", None, 4)] if kw.get("buoyancy") else []) + [("les_transport2", keys, 4)]) * n_sub
    assert calls[:len(want)] == want                               # the second-order run came first
    rest = calls[len(want):]                                       # then order=1 and the call without the arguments
    assert rest and all(c[0] in ("les_transport", "les_buoyancy") for c in rest) and any(c[0] == "les_transport" and c[1] for c in rest)


def test_float32_ensemble_as_row_blocks_with_an_empty_device():
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(lt2.Transport2OracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    subs = lt2.check_ensemble(f32_of(lt2.Transport2OracleEngine)(), [multi], 2, "plain")
    assert all(c[2] == 1 for c in calls) and len([c for c in calls if c[0] == "les_transport2"]) == 2 * sum(subs)   # blocks 1 + 1 + 0
