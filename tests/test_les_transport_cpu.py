"""K22 without a GPU: properties of the NumPy oracle of tests/les_transport_ref.py (the budget sum g x' + sum ftop = sum g x
that the split pair K16 + K17 misses, the closed overturning cell, constants, the local maximum principle, the bit identities
with K17 and between the two cells of a face, special values), the struct layout of spc_les_transport_args, the host-side
refusals of spc_les_transport_*, advection.lid_budget, and DeviceLESEnsemble's enable_advection(vertical=True,
conservative=True) on an oracle-backed engine against its host twins."""
import ctypes
import math
import os
import subprocess

import numpy
import pytest
import torch

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import advection as adv
from tests import les_transport_ref as ltr
from tests import les_vadvect_ref as lvr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {numpy.float64: 2.0 ** -52, numpy.float32: 2.0 ** -23}
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 1, 2), (2, 2, 7), (3, 5, 64), (8, 8, 40), (5, 33, 9)]          # itot x jtot x ktot


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


# -- the budget ------------------------------------------------------------------------------------------------------------------
def budget_case(dtype, seed=0):
    """3 LES of 8 x 8 x 40, random winds of 3 m/s, hx = hy = 0.005, THL and QT; outflow Courant sums of about 0.1"""
    T = numpy.dtype(dtype).type
    shape = (3, 8, 8, 40)
    rng = numpy.random.default_rng(220 + seed)
    u, v = (3.0 * rng.standard_normal(shape)).astype(T), (3.0 * rng.standard_normal(shape)).astype(T)
    g, r = ltr.profiles(3, 40, T)
    return dict(u=u, v=v, fields={k: ltr.field_like(k, shape, T, rng) for k in ("THL", "QT")}, hx=numpy.full(3, 0.005, dtype=T),
                hy=numpy.full(3, 0.005, dtype=T), g=g, r=r)


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_budget_with_random_winds(dtype):
    """|sum g x' + sum ftop - sum g x| <= 8 eps_T sum g |x| per LES and field (8: a worst-case count of the roundings per cell at
    s <= 1), the sums in float64 by math.fsum"""
    c = budget_case(dtype)
    new, cmax, _, ftop = ltr.oracle(c)
    assert 0 < cmax.max() <= 1.0
    for k, x in c["fields"].items():
        res, scale = adv.lid_budget(c["g"], x, new[k], ftop[k])
        print("budget %s %s: %s eps of sum g |x|, cmax %.3g" % (numpy.dtype(dtype).name, k, numpy.abs(res) / scale / EPS[dtype], cmax.max()))
        assert (numpy.abs(res) <= 8 * EPS[dtype] * scale).all() and (new[k] != x).any() and ftop[k].any()


def run_closed(dtype, steps, step):
    """the closed cell through ``steps`` calls of ``step(fields, c)`` -> (new fields, ftop or None); returns (the residual of
    the budget over all steps, its scale, the absolute sum of what passed the lid)"""
    c = ltr.closed_cell(dtype)
    x0 = c["fields"]["QT"]
    f, lid = dict(c["fields"]), numpy.zeros(x0.shape[:3], dtype=numpy.float64)
    for _ in range(steps):
        f, ft = step(f, c)
        if ft is not None:
            lid = lid + ft["QT"].astype(numpy.float64)
    res, scale = adv.lid_budget(c["g"], x0, f["QT"], lid)
    return res, scale, math.fsum(numpy.abs(lid).ravel())


K22 = lambda f, c: ltr.les_transport(f, c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])[0::3]                 # noqa: E731
PAIR = lambda f, c: (ltr.split_pair(f, c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"]), None)                 # noqa: E731


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_closed_cell_keeps_what_the_split_pair_loses(dtype):
    """8 x 8 x 40, u = 4 sin(2 pi i / itot) a(k) with sum_k g a = 0, fixed winds, 100 substeps at an outflow Courant sum of
    0.34.  K22 keeps sum g x within 8 eps sum g |x| per step, and (f64) what passes the lid stays below 1e-12 of the total.
    K16 followed by K17 on the same winds changes sum g x by more than the budget's bound 8 eps_T sum g |x|, in float32 too --
    what the feature fixes -- and by the same amount in both dtypes: it is the scheme, not rounding.
    Measured: K22 0.0009 (f64) and 0.0005 (f32) eps per step, lid 1.1e-16 of the total; the pair -2.36e-5 relative in both
    dtypes (25 bounds of float32, 1.3e10 of float64), more than a hundred times what K22 leaves in float32.  (With U and V
    transported alongside, as the ensemble does, the winds change, the lid opens and the pair's figure grows to -3e-3.)"""
    steps = 100
    c = ltr.closed_cell(dtype)
    assert abs(float(ltr.face_numbers(c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])["s"].max()) - 0.34) < 1e-3
    res, scale, lid = run_closed(dtype, steps, K22)
    print("closed cell %s K22: residual %.3g eps per step, lid %.3g of the total" % (numpy.dtype(dtype).name, abs(res[0]) / scale[0] / EPS[dtype] / steps, lid / scale[0]))
    assert abs(res[0]) <= steps * 8 * EPS[dtype] * scale[0]
    if dtype is numpy.float64:
        assert lid <= 1e-12 * scale[0]
    pair, pscale, _ = run_closed(dtype, steps, PAIR)
    print("closed cell %s K16 + K17: %.4g relative in %d steps, %.3g bounds" % (numpy.dtype(dtype).name, pair[0] / pscale[0], steps, abs(pair[0]) / (8 * EPS[dtype] * pscale[0])))
    assert abs(pair[0]) > 8 * EPS[dtype] * pscale[0]
    assert abs(pair[0]) > 100 * abs(res[0])
    wide, wscale, _ = run_closed(numpy.float64, steps, PAIR)
    assert abs(pair[0] / pscale[0] - wide[0] / wscale[0]) <= 0.01 * abs(wide[0] / wscale[0])


def test_split_pair_misses_the_budget_in_float32_with_random_winds():
    """the random-wind case of the budget test through K16 + K17 in float32: the pair has no lid flux of its own, so it is given
    K22's (both see the same mass flux through the lid); what remains is the pair's non-conservation.  For QT it is 1.4e-6 to
    1.9e-6 relative in the three LES against the bound 9.5e-7 that K22 keeps a hundredfold: above it, by a margin too small to
    ask of every LES (the closed cell above has the clear one), so the largest of the three is what is asserted"""
    c = budget_case(numpy.float32)
    new = ltr.split_pair(c["fields"], c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])
    ftop = ltr.oracle(c)[3]
    res, scale = adv.lid_budget(c["g"], c["fields"]["QT"], new["QT"], ftop["QT"])
    print("pair f32 QT: %s relative, the bound is %.3g" % (res / scale, 8 * EPS[numpy.float32]))
    assert (numpy.abs(res) / scale).max() > 8 * EPS[numpy.float32]


def test_lid_budget_is_exact_for_exact_inputs():
    g = numpy.array([[2.0, 4.0]])
    a = numpy.arange(8.0).reshape(1, 2, 2, 2)
    res, scale = adv.lid_budget(g, a, a - 0.5, numpy.full((1, 2, 2), 3.0))
    assert res[0] == -0.5 * 4 * 6.0 + 12.0 and scale[0] == (2.0 * a[..., 0]).sum() + (4.0 * a[..., 1]).sum()
    assert adv.lid_budget(g, a, a, None)[0][0] == 0.0


# -- the oracle's properties -----------------------------------------------------------------------------------------------------
def shaped(shape, dtype, n=2, seed=0, names=("THL", "QT")):
    itot, jtot, ktot = shape
    return ltr.case((n, itot, jtot, ktot), dtype, seed=seed, names=names)


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_keeps_a_constant_to_rounding(shape, dtype):
    """at s <= 1 a constant stays within 8 eps |x| (K16's own bound for its maximum principle); NOT bit for bit: the six fluxes
    of a constant cancel only as far as continuity holds in T"""
    c = ltr.scaled(shaped(shape, dtype)) if min(shape[:2]) > 2 or shape[2] > 1 else shaped(shape, dtype)
    const = {"a": numpy.full_like(c["u"], 287.3), "b": numpy.full_like(c["u"], -1e-3)}
    kept, cmax, _, _ = ltr.les_transport(const, c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])
    assert cmax.max() <= 1.0 and cmax.dtype == dtype and not numpy.isnan(cmax).any() and (cmax >= 0).all()
    for k, x in const.items():
        err = numpy.abs(kept[k].astype(numpy.float64) - x.astype(numpy.float64)).max() / abs(float(x.flat[0]))
        print("constant %s %s %s: %.3g eps" % (shape, numpy.dtype(dtype).name, k, err / EPS[dtype]))
        assert err <= 8 * EPS[dtype]


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", [(3, 5, 64), (8, 8, 40), (5, 33, 9), (1, 5, 3)])
def test_oracle_local_maximum_principle(shape, dtype):
    """s <= 1: x' is a convex combination of the cell and its six neighbours, so it lies in their range within 8 eps max|x|"""
    c = ltr.scaled(shaped(shape, dtype), target=1.0 - 1e-3)
    new, cmax, _, _ = ltr.oracle(c)
    assert 0.5 <= cmax.max() <= 1.0
    for k, x in c["fields"].items():
        xm = numpy.concatenate([x[..., :1], x[..., :-1]], axis=3)
        xp = numpy.concatenate([x[..., 1:], x[..., -1:]], axis=3)
        nb = numpy.stack([x, xm, xp, numpy.roll(x, 1, axis=1), numpy.roll(x, -1, axis=1), numpy.roll(x, 1, axis=2), numpy.roll(x, -1, axis=2)])
        e = 8 * EPS[dtype] * numpy.abs(x).max()
        assert (new[k] >= nb.min(axis=0) - e).all() and (new[k] <= nb.max(axis=0) + e).all() and new[k].dtype == dtype
        assert (new[k] != x).any()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_bit_identities(shape, dtype):
    """mtop is K17's bit for bit; the flux through a face has the same bits in both cells that share it; the ground is closed;
    an extent of 1 makes the two fluxes of its axis equal"""
    c = shaped(shape, dtype, seed=2)
    new, cmax, mtop, ftop = ltr.oracle(c)
    assert_bits("mtop", mtop, lvr.oracle(c)[2])
    nums = ltr.face_numbers(c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])
    assert not numpy.isnan(nums["s"]).any() and (nums["s"] >= 0).all() and not numpy.signbit(nums["s"]).any()
    for k, x in c["fields"].items():
        Fw, Fe, Fs, Fn, Fb, Ft = ltr.fluxes(x, nums)
        assert_bits("Fe of i is Fw of ip", Fe, numpy.roll(Fw, -1, axis=1))
        assert_bits("Fn of j is Fs of jp", Fn, numpy.roll(Fs, -1, axis=2))
        assert_bits("Ft of k is Fb of k + 1", Ft[..., :-1], Fb[..., 1:])
        assert not Fb[..., 0].any() and not numpy.signbit(Fb[..., 0]).any()
        assert_bits("ftop", ftop[k], Ft[..., -1])
        if shape[0] == 1:
            assert_bits("itot == 1", Fe, Fw)
        if shape[1] == 1:
            assert_bits("jtot == 1", Fn, Fs)


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_winds_uniform_per_level_are_horizontal_transport(dtype):
    c = shaped((3, 5, 9), dtype, seed=1)
    c["u"][...] = (3.0 + numpy.arange(9) % 5).astype(dtype)[None, None, None, :]
    c["v"][...] = (-2.0 + 0.37 * numpy.arange(9)).astype(dtype)[None, None, None, :]
    new, cmax, mtop, ftop = ltr.oracle(c)
    assert not mtop.any() and not numpy.signbit(mtop).any() and (cmax > 0).all() and not any(f.any() for f in ftop.values())
    for k, x in c["fields"].items():
        for l in range(2):                                      # the plane sums of every level are kept: nothing moves along k
            for lev in range(9):
                a, b = x[l, :, :, lev].astype(numpy.float64), new[k][l, :, :, lev].astype(numpy.float64)
                assert abs(math.fsum(b.ravel()) - math.fsum(a.ravel())) <= 8 * EPS[dtype] * numpy.abs(a).sum()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_special_values(dtype):
    c, s, mask = ltr.special_case(dtype)
    clean, got = ltr.oracle(c), ltr.oracle(s)
    assert_bits("THL", got[0]["THL"][~mask], clean[0]["THL"][~mask])
    assert_bits("QT", got[0]["QT"], clean[0]["QT"])
    assert numpy.isnan(got[0]["THL"][0, 0, 0, 1]) and numpy.isfinite(got[1]).all() and mask.sum() == 7 + 7 + 6 + 6
    w = dict(c, u=c["u"].copy())
    w["u"][2, 0, 4, 3] = numpy.nan
    _, cmax, mtop, _ = ltr.oracle(w)
    assert numpy.isfinite(cmax).all() and (cmax >= 0).all() and numpy.isnan(mtop[2, 0, 4, 3:]).all() and not numpy.isnan(mtop[2, 0, 4, :3]).any()


# -- plumbing --------------------------------------------------------------------------------------------------------------------
def test_struct_layout_of_the_transport_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.LesTransportArgs, "spc_les_transport_args"
    fields = ["n_les", "itot", "jtot", "ktot", "n_fields", "u", "v", "fields", "out", "hx", "hy", "cmax", "g", "r", "pitch_prof", "mtop", "ftop"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_TRANSPORT_MAX_FIELDS);']
    want = [ctypes.sizeof(cls), _abi.SPC_TRANSPORT_MAX_FIELDS]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and _abi.SPC_TRANSPORT_MAX_FIELDS == 6
    assert fields[:16] == [f[0] for f in _abi.LesVadvectArgs._fields_]          # K17's members come first, in K17's order


PTRS = ("u", "v", "hx", "hy", "cmax", "g", "r", "mtop", "ftop")


def _args(n=4, itot=8, jtot=8, ktot=20, n_fields=4, pitch_prof=None, fields=None, out=None, **ptrs):
    a = _abi.LesTransportArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields = n, itot, jtot, ktot, n_fields
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
    fn = getattr(lib, "spc_les_transport_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
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
    for kw in (dict(n_fields=0, cmax=None, mtop=None), dict(n_fields=0, cmax=None, mtop=None, ftop=None)):
        rc, text = call(**kw)
        assert rc == E and b"nothing to do" in text
    rc, text = call(pitch_prof=19)
    assert rc == E and b"pitch_prof" in text
    rc, text = call(out={3: 4096 * 20})
    assert rc == E and b"same array" in text
    inputs = [4096 * (1 + PTRS.index(k)) for k in ("u", "v", "hx", "hy", "g", "r")] + [4096 * 10, 4096 * 13]
    for ptr in inputs:
        for kw in (dict(out={2: ptr}), dict(mtop=ptr), dict(cmax=ptr), dict(ftop=ptr)):
            rc, text = call(**kw)
            assert rc == E and b"also an input" in text, kw
    for kw in (dict(mtop=4096 * 21), dict(cmax=4096 * 22), dict(cmax=4096 * 8), dict(ftop=4096 * 23), dict(ftop=4096 * 8), dict(ftop=4096 * 5),
               dict(out={0: 4096 * 5}), dict(out={5: 4096 * 8}, n_fields=6), dict(out={1: 4096 * 9})):
        rc, text = call(**kw)
        assert rc == E and b"same array" in text, kw
    for kw in (dict(fields={0: 4100 if sfx == "f64" else 4098}), dict(ftop=4096 * 9 + 2), dict(mtop=4096 * 8 + 1)):
        rc, text = call(**kw)
        assert rc == E and b"not aligned" in text, kw
    rc, text = call(n=1 << 40, ktot=3)
    assert rc == U and b"too many workgroups" in text
    assert call(fields={0: 4096, 1: 2 * 4096}, n=1 << 40, ktot=3)[0] == U      # (a field may be u or v: accepted up to the grid)
    assert call(n_fields=0, ftop=4096, n=1 << 40, ktot=3)[0] == U              # (the probe ignores ftop, even one that is u)
    rc, text = call(ktot=2560 if sfx == "f32" else 1280, pitch_prof=4000)
    assert rc == U and b"levels" in text
    assert call(ktot=1, n=1 << 40)[0] == U                                     # ktot == 1 is allowed (refused only for the grid)
    a = _args(n=0, fields={f: None for f in range(6)}, out={f: None for f in range(6)}, **{k: None for k in PTRS})
    assert fn(ctypes.byref(a), None) == 0                         # an empty ensemble is a no-op


def test_columns_per_block(lib):
    """K17's tile, K15's budget rule: the largest of 64, 32, 16 columns of ktot | 1 elements within 64 KiB, 16 may take 160 KiB"""
    f = lib.spc_les_transport_cols_per_block
    for esize in (4, 8):
        for ktot in (1, 2, 63, 64, 65, 127, 128, 129, 160, 255, 256, 257, 511, 512, 513, 1279, 1280, 2559, 2560, 5000):
            want = 0 if ktot > 163840 // 16 // esize else ltr.derived_cols(ktot, esize)
            assert f(ktot, esize) == want == lib.spc_les_vadvect_cols_per_block(ktot, esize), (ktot, esize)
    assert f(0, 8) == 0 and f(160, 2) == 0 and (f(160, 8), f(160, 4), f(1279, 8), f(1280, 8), f(2559, 4), f(2560, 4)) == (32, 64, 16, 0, 16, 0)


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    assert callable(Engine.les_transport) and callable(MultiDeviceEngine.les_transport) and callable(Engine.transport_cols_per_block)
    assert not hasattr(ltr.lbr.BuoyancyOracleEngine, "les_transport")


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    for name in ("les_advect", "les_vadvect", "les_transport", "les_buoyancy"):
        inner = getattr(engine, name)
        if name == "les_buoyancy":
            setattr(engine, name, lambda *a, _f=inner, **kw: (calls.append(("les_buoyancy", None, int(a[0].shape[0]))), _f(*a, **kw))[1])
        else:
            setattr(engine, name, lambda fields, *a, _n=name, _f=inner, **kw: (calls.append((_n, sorted(fields), int(a[1].shape[0]))), _f(fields, *a, **kw))[1])
    return engine


def _step_calls(keys, rows, n_sub, buoyant):
    sub = ([("les_buoyancy", None, rows)] if buoyant else []) + [("les_transport", keys, rows)]
    return [("les_transport", [], rows)] + sub * n_sub


@pytest.mark.parametrize("variant", ["plain", "buoyancy", "all", "all buoyant"])
def test_ensemble_on_one_engine_equals_the_host_twin(variant):
    """three steps against the twin; per step ONE probe, then per substep K21 where enabled and ONE K22: 1 + n_sub launches of
    K22 where the split mode has 2 + 2 n_sub of K16 and K17"""
    calls = []
    subs = ltr.check_ensemble(ltr.TransportOracleEngine(), [_counted(ltr.TransportOracleEngine(), calls)], 4, variant)
    kw = ltr.VARIANTS[variant]
    keys = sorted(["QT", "THL", "U", "V"] + (["QR"] if kw.get("micro") else []))
    assert len(subs) == 3 and all(s >= 1 for s in subs)
    want = []
    for n_sub in subs:
        want += _step_calls(keys, 4, n_sub, bool(kw.get("buoyancy")))
    assert calls[:len(want)] == want                               # the conservative run came first: no K16, no K17 in it
    assert all(c[0] != "les_transport" for c in calls[len(want):]) and any(c[0] == "les_vadvect" for c in calls[len(want):])


@pytest.mark.parametrize("variant", ["plain", "all buoyant"])
def test_ensemble_as_row_blocks_with_an_empty_device(variant):
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(ltr.TransportOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    subs = ltr.check_ensemble(ltr.TransportOracleEngine(), [multi], 2, variant)
    assert all(c[2] == 1 for c in calls) and len([c for c in calls if c[0] == "les_transport" and not c[1]]) == 6   # blocks 1 + 1 + 0, three steps
    assert len([c for c in calls if c[0] == "les_transport" and c[1]]) == 2 * sum(subs)


def _small(eng, n=2, nL=6):
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(n, nL=nL)
    return models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)


def _attach(ens, names=("U", "V", "THL", "QT")):
    rng = numpy.random.default_rng(1)
    ens.attach_fields({k: rng.standard_normal((2, 2, 3, 6)) + m for k, m in (("U", 5.0), ("V", -2.0), ("THL", 290.0), ("QT", 5.0)) if k in names})


def test_conservative_is_opt_in_and_follows_the_substep_rule():
    eng = ltr.TransportOracleEngine()
    ens = _small(eng)
    _attach(ens)
    with pytest.raises(ValueError, match="vertical=True"):
        ens.enable_advection(dx=50000.0, dy=50000.0, conservative=True)
    ens.enable_advection(dx=50000.0, dy=50000.0, vertical=True)
    assert not ens.advect_conservative and ens.get_lid_flux_batched() is None
    ens.evolve_model_batched(100.0)
    assert ens.advect_courant_z is not None and ens.get_lid_flux_batched() is None
    ens.enable_advection(dx=50000.0, dy=50000.0, vertical=True, conservative=True, cfl=0.004)
    assert ens.advect_conservative and ens.get_lid_flux_batched() is None and ens.get_vertical_wind_batched() is None
    f = {k: ens.get_fields_batched(k).numpy().copy() for k in ("U", "V")}
    T = f["U"].dtype
    hx, hy = (a.astype(T) for a in adv.coefficients(100.0, 50000.0, 50000.0, n=2))
    g, r = (a.astype(T) for a in adv.vertical_profiles(ens.water_path_weights()))
    c = float(ltr.face_numbers(f["U"], f["V"], hx, hy, g, r)["s"].max())
    ens.evolve_model_batched(200.0)
    assert ens.advect_substeps == adv.substeps(c, 0.004, adv.MAX_SUBSTEPS) > 1
    assert 0 < ens.advect_courant <= 0.004 * 1.5 and ens.advect_courant_z is None
    lid = ens.get_lid_flux_batched()
    assert list(lid) == ["U", "V", "THL", "QT"] and all(tuple(t.shape) == (2, 2, 3) for t in lid.values()) and bool(lid["THL"].any())
    w = ens.get_vertical_wind_batched()
    assert tuple(w.shape) == (2, 2, 3, 6) and bool(torch.isfinite(w).all()) and bool((w != 0).any())
    ens.enable_advection(dx=50000.0, dy=50000.0, vertical=True, conservative=True, max_substeps=2, cfl=0.004)
    before = {k: ens.get_fields_batched(k).numpy().copy() for k in ("U", "THL")}
    with pytest.raises(RuntimeError, match="max_substeps"):
        ens.evolve_model_batched(300.0)
    for k, x in before.items():                                    # nothing was transported (the step itself has no tendencies here)
        assert_bits(k, ens.get_fields_batched(k).numpy(), x)
    old = models.DeviceLESEnsemble(ens.grid_indices, ens.zf_cache, ens.zh_cache, ens.p, itot=2, jtot=3, engine=ltr.lbr.BuoyancyOracleEngine())
    old.attach_fields({"U": numpy.zeros((2, 2, 3, 6)), "V": numpy.zeros((2, 2, 3, 6))})
    old.enable_advection(vertical=True)
    with pytest.raises(ValueError, match="les_transport"):
        old.enable_advection(vertical=True, conservative=True)


def test_a_courant_sum_that_is_not_finite_raises():
    eng = ltr.TransportOracleEngine()
    ens = _small(eng)
    _attach(ens, names=("U", "V", "THL"))
    ens.enable_advection(dx=50000.0, dy=50000.0, vertical=True, conservative=True)
    inner = eng.les_transport

    def grown(fields, *a, **kw):
        res = inner(fields, *a, **kw)
        return res.fill_(float("inf")) if fields else res            # the probe passes; the substep's sum is not finite
    eng.les_transport = grown
    with pytest.raises(RuntimeError, match="K22"):
        ens.evolve_model_batched(100.0)
    assert ens.advect_courant == float("inf")


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "buoyancy", "all", "all buoyant"])
def test_float32_ensemble_on_one_engine_equals_the_host_twin(variant):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    calls = []
    subs = ltr.check_ensemble(f32_of(ltr.TransportOracleEngine)(), [_counted(f32_of(ltr.TransportOracleEngine)(), calls)], 4, variant)
    kw = ltr.VARIANTS[variant]
    keys = sorted(["QT", "THL", "U", "V"] + (["QR"] if kw.get("micro") else []))
    assert len(subs) == 3 and all(s >= 1 for s in subs)
    want = []
    for n_sub in subs:
        want += _step_calls(keys, 4, n_sub, bool(kw.get("buoyancy")))
    assert calls[:len(want)] == want                               # the conservative run came first: no K16, no K17 in it
    assert all(c[0] != "les_transport" for c in calls[len(want):]) and any(c[0] == "les_vadvect" for c in calls[len(want):])


@pytest.mark.parametrize("variant", ["plain", "all buoyant"])
def test_float32_ensemble_as_row_blocks_with_an_empty_device(variant):
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(ltr.TransportOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    subs = ltr.check_ensemble(f32_of(ltr.TransportOracleEngine)(), [multi], 2, variant)
    assert all(c[2] == 1 for c in calls) and len([c for c in calls if c[0] == "les_transport" and not c[1]]) == 6   # blocks 1 + 1 + 0, three steps
    assert len([c for c in calls if c[0] == "les_transport" and c[1]]) == 2 * sum(subs)
