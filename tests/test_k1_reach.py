"""K1's reach form: multi-round launches load T, SH, QL, QI, Pf, U, V only at the GCM levels the LES interpolation can
bracket (k_forward with PRE = false).

CPU: spc_describe_launch names the form of every size class.  -m gpu: levels outside each column's reach may hold
anything (NaN poison) without changing one output bit; adversarial columns (non-monotone / NaN heights, a LES grid
entirely above or below the column, NaN grid levels, per-column grids, padded pitches, a ragged last slab) give
exactly the bits of the one-phase kernel (SPC_K1_PRE=1, same library), and their regular columns those of the C oracle.
"""
import numpy
import pytest
import torch

from sp_coupler_amd import _abi, synthetic
from tests import oracle_c
from tests.gpu_util import EPS, assert_bits, host, to_dev

FACTOR, DT = 0.85, 900.0
GRAV = 9.81
LEAN = ("f_u", "f_v", "f_thl", "f_qt", "f_ql", "ql_ref", "f_ps", "idx")
FIELDS = ("T", "SH", "QL", "QI", "Pfull", "U", "V")       # what phase B loads only inside the reach


def _dims(n, nG=91, nL=160, pad=0):
    return _abi.Dims(n, nG, nL, nG + pad, nG + 1 + pad, nL + pad, 1, 0)


def test_describe_launch_names_the_k1_form(monkeypatch):
    """the reach form for the multi-round launches of configs 3 and 5, the one-phase kernel up to 1024 columns"""
    from sp_coupler_amd import _abi as abi
    monkeypatch.setenv("SPC_CUS", "256")
    lib = abi.load_library()

    def form(n, elem=8, **kw):
        fields = dict(kv.split("=") for kv in abi.describe_launch(lib, _dims(n, **kw), 0, 1, elem).split()[1:])
        return fields["form"]
    assert form(35718) == "reach"                        # config 3
    assert form(88838, nG=137, nL=512) == "reach"        # config 5
    assert form(35718, pad=3) == "reach"                 # run-time geometry
    assert form(1025) == "reach"
    for n in (1, 200, 300, 1024):                        # config 2 and below: one round, one phase
        assert form(n) == "whole"
        assert form(n, nG=137, nL=512) == "whole"
    assert form(35718, elem=4) == "vec"                  # k_forward_f32v: every level
    assert form(35718, elem=4, pad=1) == "reach"         # scalar float K1
    assert " form=" not in abi.describe_launch(lib, _dims(35718), 1, 0)
    monkeypatch.setenv("SPC_CUS", "64")                  # a smaller partition: one round ends at 256 columns
    assert form(257) == "reach" and form(256) == "whole"


def _reach_top(zf_col_rev, zf_grid):
    """largest ascending-order level numpy.interp reads for any LES height (monotone, NaN-free Zf)"""
    n = zf_col_rev.shape[0]
    x = zf_grid[~numpy.isnan(zf_grid)]
    j = numpy.searchsorted(zf_col_rev, x, side="right") - 1
    j1 = numpy.where(j >= n - 1, n - 1, numpy.where(j < 0, 0, numpy.where(zf_col_rev[numpy.clip(j, 0, n - 1)] == x, j, j + 1)))
    return int(j1.max()) if j1.size else 0


def _lean(eng, gcm_d, zf_d, zh_d, prof_d):
    fp, _ = eng.plan_exchange(gcm_d, zf_d, zh_d, prof_d, FACTOR, FACTOR, DT)
    desc = _abi.describe_launch(eng.lib, fp.dims, 0, 1)
    out = fp.launch()
    torch.cuda.synchronize()
    return {k: host(out[k]) for k in LEAN}, desc


@pytest.fixture(scope="module")
def eng():
    from sp_coupler_amd.engine import Engine
    return Engine("cuda:0")


@pytest.mark.gpu
def test_levels_outside_the_reach_are_never_read(eng):
    """config-3-sized batch: NaN in the 7 phase-B fields at every level above each column's reach -> identical bits;
    the control poisons one level INSIDE the reach and must change an output"""
    gcm, zf, zh, prof = synthetic.make_config(3)
    n, nG = gcm["T"].shape
    zfull = (gcm["Zgfull"] - gcm["Zghalf"][:, nG:nG + 1]) / GRAV          # spcpl.py:198, as the kernel forms it
    tops = numpy.array([_reach_top(zfull[c, ::-1], zf) for c in range(n)])
    assert tops.max() < nG - 1, "the batch must leave levels outside the reach"
    g, p = to_dev(gcm, eng.device), to_dev(prof, eng.device)
    zf_d, zh_d = torch.from_numpy(zf).to(eng.device), torch.from_numpy(zh).to(eng.device)
    clean, desc = _lean(eng, g, zf_d, zh_d, p)
    assert " form=reach" in desc, desc
    above = numpy.arange(nG)[None, :] < (nG - 1 - tops)[:, None]           # top-down index k above the reach
    mask = torch.from_numpy(above).to(eng.device)
    for f in FIELDS:
        g[f] = g[f].masked_fill(mask, float("nan"))
    poisoned, _ = _lean(eng, g, zf_d, zh_d, p)
    for k in LEAN:
        assert_bits("poisoned " + k, poisoned[k], clean[k])
    c = int(numpy.argmax(tops))                                             # control: the top level of one reach
    g["T"][c, nG - 1 - tops[c]] = float("nan")
    g["U"][c, nG - 1 - tops[c]] = float("nan")
    control, _ = _lean(eng, g, zf_d, zh_d, p)
    assert numpy.isnan(control["f_thl"][c]).any() and numpy.isnan(control["f_u"][c]).any()
    other = numpy.arange(n) != c
    assert_bits("control f_thl elsewhere", control["f_thl"][other], clean["f_thl"][other])


def _adversarial(per_column_grid, grid_nan):
    """1100 columns (a ragged last slab of 4 at 8 per workgroup) with a few hostile ones; returns the batch and the
    indices of the columns that stay monotone and NaN-free"""
    gcm, zf, zh, prof = synthetic.make_batch(1100, 91, 160, seed=606, per_column_grid=per_column_grid)
    nG = gcm["T"].shape[1]
    zg, zs = gcm["Zgfull"], gcm["Zghalf"][:, nG:nG + 1]
    zg[3, 40:70] = zg[3, 40:70][::-1].copy()                   # non-monotone, inside and across the reach
    zg[5, [nG - 3, nG - 2]] = zg[5, [nG - 2, nG - 3]]          # two lowest levels swapped
    zg[11, nG - 6] = numpy.nan                                 # NaN heights: in the reach ...
    zg[12, 10] = numpy.nan                                     # ... and far above it
    zg[20] = zs[20] + (zg[20] - zs[20]) * 1e-3                  # column under the whole LES grid: reach = every level
    zg[27] = zg[27] + 1e6                                      # column above the whole LES grid: reach = level 0, 1
    zg[1099] = zs[1099] + (zg[1099] - zs[1099]) * 0.05          # the last (ragged) slab reaches higher
    hostile = [3, 5, 11, 12]
    if grid_nan:
        if per_column_grid:
            zf[7, [0, 50]] = numpy.nan
            hostile.append(7)
        else:
            zf[[0, 50]] = numpy.nan
            hostile = list(range(1100))
    regular = numpy.setdiff1d(numpy.arange(1100), hostile)
    return gcm, zf, zh, prof, regular


def _pad(t, pad):
    if pad == 0 or t.dim() != 2:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=t.device, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("per_column_grid,grid_nan,pad", [(False, False, 0), (False, False, 3), (True, False, 0),
                                                           (True, True, 0), (False, True, 0)])
def test_adversarial_columns_match_the_one_phase_kernel(eng, monkeypatch, per_column_grid, grid_nan, pad):
    gcm, zf, zh, prof, regular = _adversarial(per_column_grid, grid_nan)
    g = {k: _pad(v, pad) for k, v in to_dev(gcm, eng.device).items()}
    p = {k: _pad(v, pad) for k, v in to_dev(prof, eng.device).items()}
    zf_d, zh_d = torch.from_numpy(zf).to(eng.device), torch.from_numpy(zh).to(eng.device)
    got = {}
    for pre, form in (("0", "reach"), ("1", "whole")):
        monkeypatch.setenv("SPC_K1_PRE", pre)
        lean, desc = _lean(eng, g, zf_d, zh_d, p)
        assert " form=%s" % form in desc, desc
        full = eng.forward(g, zf_d, p, FACTOR, DT, zh=zh_d, want_profiles=True, couple_surface=True)
        torch.cuda.synchronize()
        got[form] = (lean, {k: host(v) for k, v in full.items()})
    monkeypatch.delenv("SPC_K1_PRE")
    (lr, fr), (lw, fw) = got["reach"], got["whole"]
    for k in lean:
        assert_bits("lean " + k, lr[k], lw[k])
    for k in fr:
        assert_bits("full " + k, fr[k], fw[k])
    if regular.size == 0:
        return
    # the regular columns against the plain-C oracle
    ref = oracle_c.forward(gcm, zf, zh, prof, FACTOR, DT, couple_surface=True)
    for k in ("f_u", "f_v", "f_qt", "f_ql", "ql_ref", "f_ps", "idx"):
        assert_bits("oracle " + k, lr[k][regular], ref[k][regular])
    err = numpy.abs(lr["f_thl"][regular] - ref["f_thl"][regular])
    assert numpy.isfinite(err).all() and err.max() <= 8 * EPS * numpy.abs(ref["thl"][regular]).max() * FACTOR / DT
