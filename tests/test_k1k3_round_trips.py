"""K1's reach form and K3 with fewer dependent memory round trips per workgroup: phase A's first two
items, the held index entries and f_ps in the reach gap (k_forward, PRE = false); the second staging round on the waves
without a GCM item (k_backward, PRE = true, double).

Every check is bit for bit (NaN positions and the sign of zero included).  K1: the reach form forced at small size
(SPC_K1_PRE=0) against the one-phase kernel (SPC_K1_PRE=1) of the same library, and against the plain-C oracle on regular
columns (f_thl: 8 ulp of thl / dt, device pow against libm's); cols_per_block 1, 2, 4, 8 and n_cols = 3 cb + 1, so that
the last slab is ragged.  K3: cols_per_block forced at n_cols <= 1024 (the PRE = true, write-through instantiation)
against the oracle, at every relation of spare lanes to later staging items (the spare lanes take them all or none).
"""
import functools

import numpy
import pytest
import torch

from sp_coupler_amd import _abi, synthetic
from tests import oracle_c
from tests.gpu_util import EPS, assert_bits, host, to_dev
from tests.test_k1_reach import _adversarial, _pad

pytestmark = pytest.mark.gpu

FACTOR, DT = 0.85, 900.0
LEAN = ("f_u", "f_v", "f_thl", "f_qt", "f_ql", "ql_ref", "f_ps", "idx")
BWD = ("f_T", "f_SH", "f_QL", "f_QI", "f_U", "f_V", "f_A", "start_index")
CBS = (1, 2, 4, 8)
N_REF = 3 * max(CBS) + 1                 # every case is a prefix of one batch per geometry: ONE oracle run each


@functools.lru_cache(maxsize=None)
def _engine(dtype):
    from sp_coupler_amd.engine import Engine
    return Engine("cuda:0", dtype=dtype)


@functools.lru_cache(maxsize=None)
def _batch(nG, nL, per_column_grid, dtype):
    """(gcm, zf, zh, prof, forward oracle, backward oracle) of N_REF columns in ``dtype``; never modified"""
    gcm, zf, zh, prof = synthetic.make_batch(N_REF, nG, nL, seed=9100 + nG + nL, per_column_grid=per_column_grid)
    gcm, prof = ({k: numpy.ascontiguousarray(v, dtype) for k, v in d.items()} for d in (gcm, prof))
    zf, zh = numpy.ascontiguousarray(zf, dtype), numpy.ascontiguousarray(zh, dtype)
    ref_f = oracle_c.forward(gcm, zf, zh, prof, FACTOR, DT, couple_surface=True)
    ref_b = oracle_c.backward(gcm, None, zf, prof, FACTOR, DT)
    return gcm, zf, zh, prof, ref_f, ref_b


def _prefix(d, n):
    return {k: v[:n] for k, v in d.items()}


def _grid(z, n):
    return z if z.ndim == 1 else z[:n]


def _device_inputs(eng, gcm, zf, zh, prof, n, pad):
    tdt = eng.dtype
    g = {k: _pad(v, pad) for k, v in to_dev(_prefix(gcm, n), eng.device, tdt).items()}
    p = {k: _pad(v, pad) for k, v in to_dev(_prefix(prof, n), eng.device, tdt).items()}
    zf_d, zh_d = (torch.from_numpy(numpy.ascontiguousarray(_grid(z, n))).to(eng.device) for z in (zf, zh))
    if zf_d.dim() == 2:
        zf_d, zh_d = _pad(zf_d, pad), _pad(zh_d, pad)
    return g, p, zf_d, zh_d


def _forward_both_forms(eng, monkeypatch, g, p, zf_d, zh_d, cb, want_idx=True):
    """{form: (lean outputs, full outputs)} of the reach form and of the one-phase kernel at ``cb`` columns per workgroup"""
    esize = 8 if eng.dtype == torch.float64 else 4
    lean_in = {k: v for k, v in p.items() if k not in ("Rain", "rain_last")}
    got = {}
    for pre, form in (("0", "reach"), ("1", "whole")):
        monkeypatch.setenv("SPC_K1_PRE", pre)
        plan = eng.plan_forward(g, zf_d, lean_in, FACTOR, DT, zh=zh_d, want_profiles=False, want_heights=False,
                                want_idx=want_idx, cols_per_block=cb)
        desc = _abi.describe_launch(eng.lib, plan.dims, 0, 1 if want_idx else 0, esize)
        assert " form=%s" % form in desc and " cb=%d " % cb in desc, desc
        lean = {k: host(v).copy() for k, v in plan.launch().items()}
        full = eng.forward(g, zf_d, p, FACTOR, DT, zh=zh_d, want_profiles=True, couple_surface=True, want_idx=want_idx,
                           cols_per_block=cb)
        torch.cuda.synchronize()
        got[form] = (lean, {k: host(v).copy() for k, v in full.items()})
    monkeypatch.delenv("SPC_K1_PRE")
    return got


def _check_forms_agree(tag, got, want_idx=True):
    (lr, fr), (lw, fw) = got["reach"], got["whole"]
    assert ("idx" in lr) == want_idx and set(lr) == set(lw) and set(fr) == set(fw)
    for k in lr:
        assert_bits(tag + " lean reach/whole " + k, lr[k], lw[k])
    for k in fr:
        assert_bits(tag + " full reach/whole " + k, fr[k], fw[k])


def _check_oracle_f64(tag, lean, ref, rows):
    for k in lean:
        if k != "f_thl":
            assert_bits(tag + " oracle " + k, lean[k][rows], ref[k][rows])
    err = numpy.abs(lean["f_thl"][rows] - ref["f_thl"][rows])
    bound = 8 * EPS * numpy.abs(ref["thl"][rows]).max() * FACTOR / DT
    print("%s f_thl: max abs err %.3e, bound %.3e" % (tag, err.max(), bound))
    assert numpy.isfinite(err).all() and err.max() <= bound


# (nG, nL, pad, per-column grid, fused index map)
K1_CASES = {"91x160": (91, 160, 0, False, True),
            "137x512": (137, 512, 0, False, True),          # cb = 4: 548 phase-A items -> held AND leftover index entries
            "padded_pitch": (91, 160, 3, False, True),      # run-time geometry
            "per_column_grid": (91, 160, 0, True, True),
            "no_idx": (91, 160, 0, False, False)}


@pytest.mark.parametrize("cb", CBS)
@pytest.mark.parametrize("case", sorted(K1_CASES))
def test_k1_reach_form_against_the_one_phase_kernel_and_the_oracle(monkeypatch, case, cb):
    nG, nL, pad, per_col, want_idx = K1_CASES[case]
    eng = _engine(torch.float64)
    gcm, zf, zh, prof, ref_f, _ = _batch(nG, nL, per_col, numpy.float64)
    n = 3 * cb + 1
    g, p, zf_d, zh_d = _device_inputs(eng, gcm, zf, zh, prof, n, pad)
    got = _forward_both_forms(eng, monkeypatch, g, p, zf_d, zh_d, cb, want_idx)
    tag = "%s cb=%d" % (case, cb)
    _check_forms_agree(tag, got, want_idx)
    _check_oracle_f64(tag, got["reach"][0], ref_f, slice(0, n))


@pytest.mark.parametrize("cb", CBS)
def test_k1_scalar_float_reach_form(monkeypatch, cb):
    """float at a padded pitch: the scalar float K1 (the 8-byte-access kernel is not touched); the float oracle evaluates pow
    as the device does, so f_thl is bit-checked too"""
    eng = _engine(torch.float32)
    gcm, zf, zh, prof, ref_f, _ = _batch(91, 160, False, numpy.float32)
    n = 3 * cb + 1
    g, p, zf_d, zh_d = _device_inputs(eng, gcm, zf, zh, prof, n, 1)
    got = _forward_both_forms(eng, monkeypatch, g, p, zf_d, zh_d, cb)
    tag = "f32 cb=%d" % cb
    _check_forms_agree(tag, got)
    for k, v in got["reach"][0].items():
        assert_bits(tag + " oracle " + k, v, ref_f[k][:n])


@functools.lru_cache(maxsize=None)
def _adversarial_batch(per_column_grid, grid_nan):
    gcm, zf, zh, prof, regular = _adversarial(per_column_grid, grid_nan)
    ref = oracle_c.forward(gcm, zf, zh, prof, FACTOR, DT, couple_surface=True) if regular.size else None
    return gcm, zf, zh, prof, regular, ref


@pytest.mark.parametrize("cb", CBS)
@pytest.mark.parametrize("per_column_grid,grid_nan", [(False, False), (True, True), (False, True)])
def test_k1_adversarial_columns(monkeypatch, per_column_grid, grid_nan, cb):
    """the hostile columns of tests/test_k1_reach.py (non-monotone or NaN Zgfull, NaN grid levels, a grid entirely above or
    below the column) at every slab size: 1100 columns, ragged at 8 per workgroup"""
    eng = _engine(torch.float64)
    gcm, zf, zh, prof, regular, ref = _adversarial_batch(per_column_grid, grid_nan)
    g, p, zf_d, zh_d = _device_inputs(eng, gcm, zf, zh, prof, gcm["T"].shape[0], 0)
    got = _forward_both_forms(eng, monkeypatch, g, p, zf_d, zh_d, cb)
    tag = "adversarial per_col=%s grid_nan=%s cb=%d" % (per_column_grid, grid_nan, cb)
    _check_forms_agree(tag, got)
    if regular.size:
        _check_oracle_f64(tag, got["reach"][0], ref, regular)


# (cb, nG, nL): relation of the spare lanes (behind the last GCM item's wave) to the staging items >= 256
K3_CASES = {"spare_wave_takes_all_64": (2, 91, 160),        # 182 GCM items, 320 staging items
            "more_later_items_than_spare_lanes": (1, 137, 512),   # 64 spare lanes, 256 later items: the loop keeps them all
            "three_spare_waves": (2, 19, 160),              # 38 GCM items
            "spare_waves_nothing_to_take": (1, 91, 160),    # 160 staging items
            "no_spare_wave": (4, 91, 160)}                  # 364 GCM items


@pytest.mark.parametrize("variant", ["whole_slabs", "ragged", "ragged_per_column_grid", "ragged_padded_pitch"])
@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(K3_CASES))
def test_k3_prologue_form_against_the_oracle(case, dtype, variant):
    cb, nG, nL = K3_CASES[case]
    eng = _engine(torch.float64 if dtype == numpy.float64 else torch.float32)
    gcm, zf, zh, prof, _, ref_b = _batch(nG, nL, "per_column" in variant, dtype)
    n = 3 * cb + (0 if variant == "whole_slabs" else 1)
    g, p, zf_d, _ = _device_inputs(eng, gcm, zf, zh, prof, n, 2 if "padded" in variant else 0)
    plan = eng.plan_backward(g, zf_d, p, FACTOR, DT, Zf=None, want_start_index=True, cols_per_block=cb)
    desc = _abi.describe_launch(eng.lib, plan.dims, 1, 0, numpy.dtype(dtype).itemsize)
    assert "wt=1,blk=256,pre=1>" in desc and " cb=%d " % cb in desc, desc
    out = plan.launch()
    torch.cuda.synchronize()
    assert set(out) == set(BWD)
    for k in BWD:
        assert_bits("%s %s %s %s" % (case, variant, numpy.dtype(dtype).name, k), host(out[k]), ref_b[k][:n])
