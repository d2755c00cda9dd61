"""Random operation sequences of models.DeviceLESEnsemble on oracle-backed engines against its NumPy twin, without a GPU
(the body: tests/ensemble_sequences.py): all 48 valid combinations of the six old modes, 55 with the five of K19 to K23 and the
statistics of K20, 14 with the three mixing modes (K24, K25 and K24 with vertical=True) and the same 14 with "imix" (K26:
enable_mixing(implicit=True), switched off and on again) with two seeds, row blocks 1 + 1 + 0 of
a MultiDeviceEngine, the fused K11 step in front of every later stage, sequences of 30 operations, the three digests of the older
sequences (they are what they were before the modes that came after them), the named regression sequences of what the sequences found, and the state mutants: faults of the ensemble's caches, patched in, that a committed sequence has to notice.

Which committed sequence (seed, modes; n = 3 on one engine) notices which state mutant:
  1  _drop_water_paths does nothing                              seed 1 plain, seed 1 thermo
  2  set_fields_batched does not set _thermo_stale               seed 1 thermo+diffuse, seed 2 thermo+advect
  3  set_fields_batched does not clear _means                    seed 2 diffuse, seed 1 micro
  4  _diffuse's profile cache ignores dt                         seed 1 diffuse, seed 2 diffuse
  5  _microphysics' profile cache ignores presf                  seed 1 thermo+micro, seed 1 micro+advect+vertical
  6  _microphysics does not swap f["QR"] and _qr_spare           seed 1 micro, seed 2 thermo+micro
  7  get_water_paths_batched ignores a changed weight profile    seed 1 plain, seed 2 thermo
  8  the nudge's tail (the same tensor set again) keeps _means   seed 1 thermo+diffuse, seed 2 thermo+advect
  9  _drop_statistics does nothing                               seed 1 and seed 2 advect+vertical+stats
  10 _drop_statistics keeps _stats_host                          seed 1 and seed 2 advect+vertical+stats
  11 _qt_local leaves _means, _thermo_stale and the QL field     seed 1 and seed 2 qt
     as they were (no _follow_fields behind K19)
  12 _buoyancy_profiles' key ignores presf                       seed 2 advect+vertical+buoyancy+conservative, seed 1 old six+qt+buoyancy
  13 _transport keeps only the last substep's ftop               seed 2 advect+vertical+qt+conservative, seed 2 advect+vertical+buoyancy+conservative
  14 enable_qt_forcing keeps _qt_counts across a change of kind  seed 2 advect+vertical+qt+stats, seed 1 old six+qt+conservative+stats
  15 enable_advection keeps the lid flux of the earlier call     seed 2 advect+vertical+buoyancy+conservative+order2, seed 2 the same with qt
  16 enable_advection keeps the buoyancy enabled                 seed 2 advect+vertical+buoyancy, seed 2 advect+vertical+buoyancy+conservative+order2
  17 a new Rhobf keeps the host copies of the moments of W       seed 1 and seed 2 advect+vertical+buoyancy+stats
  18 the key of the statistics' W ignores Rhobf                  seed 1 and seed 2 advect+vertical+buoyancy+stats
  19 _mix does not swap the fields with _mix_spare               seed 1 mix, seed 2 mix+vmix
  20 _mix_coef's key ignores dt                                  seed 1 mix, seed 2 mix+vmix
  21 _vmix_coef's key ignores Rhobf                              seed 1 qt+stats+mix+vmix, seed 2 advect+vertical+buoyancy+stats+mix+vmix
  22 _vmix_drag keeps the z0m of its first upload                seed 2 mix+vmix, seed 1 advect+vertical+buoyancy+conservative+order2+mix+vmix
  23 _mix never runs the uncapped probe: K25 mixes by the        seed 1 and seed 2 mix+vmix
     capped km
  24 the probe reads f["U"], f["V"] after the swap               seed 1 and seed 2 mix+vmix
  25 enable_mixing keeps _mix_km of the earlier call             seed 1 mix, seed 2 diffuse+mix+kmix
  26 _diffuse keeps the kd of its first upload with one          seed 1 diffuse+mix+kmix, seed 2 diffuse+advect+vertical+buoyancy+conservative+order2+mix+kmix
  27 K26 mixes by the capped km: its probe runs under kcap,      seed 2 mix+imix, seed 2 mix+vmix+imix
     not under _hmix_huge
  28 _mix_implicit ends without _mix_tail()                      seed 1 mix+imix, seed 1 diffuse+mix+kmix+imix
  29 _mix_implicit does not set mixing_capped = False            seed 1 mix+imix, seed 1 mix+vmix+imix
  30 kh_cap ignored: the upload of kh2 uses the default          seed 1 mix+imix, seed 2 mix+vmix+imix
  31 enable_mixing never switches K26 off again                  seed 1 mix+imix, seed 2 diffuse+mix+kmix+imix
  32 _mix_implicit does not set mixing_k_max                     seed 1 mix+imix, seed 2 mix+vmix+imix
  (20 and 25 on the path of K26 as well: seed 2 mix+vmix+imix and seed 1 mix+imix)
(test_state_mutants_fail_a_committed_sequence asserts every line of this table.  Mutant 11 takes the call of _follow_fields
with the assignment: the assignment alone is redundant, every path behind K19 ends in _follow_fields, which sets both.  Mutant
12 reads the presf of the last upload into the key AND the profiles; a key that only COMPARES without presf never shows,
because the slab means in the same key change with every step.  Mutants 22 and 26 are widened the same way: a key that only
compares without z0m, or without kd, shows in ONE committed sequence each, because dt stands in the same key and two steps in a
row seldom share it; so mutant 22 reads the z0m of the first upload into the key and the drag, mutant 26 the kd of the first
upload with one into the key and the profiles.  Mutant 23 leaves the launch out and hands K24's capped km to K25; what fails
first is the count of les_mix launches of a step whose cap bound.  _mix's own _drop_statistics and _drop_water_paths are followed
by those of _follow_fields in every path and are no mutants of their own.  Mutant 29 fails first at check_step's own
``mixing_capped is False``; without that assertion K25 would mix by the stale second buffer.  Mutant 30 shows only where a
kh_cap other than the default is in force: its sequences hold one.  Three faults of K26's state are guarded twice and show in
NO committed sequence (TWICE_GUARDED; test_twice_guarded_faults_do_not_show runs every "imix" case with each planted):
enable_mixing keeping _hmix_kh2 (the key of the upload still compares kh_cap), keeping _hmix_huge (the value depends on the
engine's type and n alone, and neither changes) and keeping _mix_spare (``_scratch`` hands a spare buffer back only where it
still fits the field, and K24 overwrites every cell of it before the swap).)"""
import hashlib
import inspect
import itertools
import re
import textwrap

import numpy
import pytest
import torch

from sp_coupler_amd import advection as adv
from sp_coupler_amd import buoyancy as buo
from sp_coupler_amd import device_les, models, spcpl
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import ensemble_sequences as es
from tests import gpu_util
from tests import les_hmix_ref as lhr
from tests import les_micro_ref as lmr
from tests import les_thermo_ref as ltr
from tests import les_vadvect_ref as lvr
from tests import les_vmix_ref as lvm
from tests import slab_ref
from tests.les_harness import NP, f32_of

SEEDS = (1, 2)
COMBINATIONS = es.combinations()
SIX = [(), ("thermo", "micro"), ("diffuse", "advect", "vertical"), ("micro", "radiate"), ("thermo", "diffuse", "advect", "radiate"), es.OLD_MODES]
#: the 23 non-empty valid subsets of the five new modes over the smallest background that takes them all and over all six old
#: modes, and the two modes that need no advection over three backgrounds without it: 46 + 9 combinations
NEW_COMBINATIONS = es.new_combinations(("advect", "vertical")) + es.new_combinations(es.OLD_MODES) + \
    [bg + c for bg in ((), ("thermo",), ("diffuse", "micro")) for c in (("qt",), ("stats",), ("qt", "stats"))]
ALL_COMBINATIONS = COMBINATIONS + NEW_COMBINATIONS
NEW_SIX = [("advect", "vertical", "qt", "conservative"), ("advect", "vertical", "buoyancy", "order2", "conservative"), ("advect", "vertical", "stats"),
           ("thermo", "qt", "stats"), ("diffuse", "micro", "qt"), es.ELEVEN]
NEW_SIX = [tuple(m for m in es.MODES if m in c) for c in NEW_SIX]
#: sha256 over repr((seed, modes, generate(seed, modes, length))) of the 48 old combinations, seeds 1, 2 and 3 at length 14 and seed
#: 101 at length 30, computed from tests/ensemble_sequences.py as it was before the five new modes
OLD_SEQUENCES = "d5ab020b0faa71f622d7b6a095a2e44e9c9e763bb95676f71aad60aaf78766eb"
#: the same over the 55 NEW_COMBINATIONS, computed from tests/ensemble_sequences.py as it was before the three mixing modes
NEW_SEQUENCES = "ece619774f522f90b8fe31b246e58ff697b4d110f57a4c5aa31ef29ab48e4ae8"
TRANSPORT = ("advect", "vertical", "conservative", "order2", "buoyancy")
MOIST = ("thermo", "micro", "radiate", "qt", "stats")
#: K24, K25 and K24 with vertical=True: every valid non-empty subset of the three over the smallest background that takes it and
#: over the whole transport with K21 (the diffusion joins where vertical=True needs it; mix alone meets it as well: K15 behind K24
#: without its viscosity, and the refusal of K25 beside it), mix and mix+vmix over the moist modes with K19 and K20, and over two
#: smaller backgrounds in which the operations of K19, K20 and K21 are not crowded out by the late enables: 14 combinations
MIX_COMBINATIONS = [tuple(m for m in es.MODES if m in c) for bg in ((), ("diffuse",), TRANSPORT, TRANSPORT + ("diffuse",), MOIST, ("qt", "stats"),
                                                                      ("advect", "vertical", "buoyancy", "stats")) for c in es.mix_combinations(bg)]
MIX_SIX = [("mix",), ("mix", "vmix"), ("diffuse", "mix", "kmix"), TRANSPORT + ("mix", "vmix"), TRANSPORT + ("diffuse", "mix", "kmix"), MOIST + ("mix", "vmix")]
MIX_SIX = [tuple(m for m in es.MODES if m in c) for c in MIX_SIX]
#: the same over the 14 MIX_COMBINATIONS, computed from tests/ensemble_sequences.py as it was before "imix" (K26)
MIX_SEQUENCES = "e0fe19100e85e51b37b76e170d39e147c9e40aabd5056940320881c0965afef3"
#: K26: every mixing combination once more with "imix" (the first enable_mixing passes implicit=True, the mutation "implicit"
#: switches between K26 and K24's explicit path), and the counterparts of MIX_SIX
#: sha256 over the kind, limiter, cap, stability, drag and dx of ``params`` of all 117 older combinations, seeds 1, 2, 3 and 101,
#: computed from tests/ensemble_sequences.py as it was before ``params`` drew the kh_cap of K26
OLD_PARAMS = "dca1b238c3cd940b9a347b9964c9beb5799a2b4c43e30c65c69c0d1230676763"
IMIX_COMBINATIONS = [c + (es.IMIX,) for c in MIX_COMBINATIONS]
IMIX_SIX = [c + (es.IMIX,) for c in MIX_SIX]


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def _oracle():
    return lhr.HmixOracleEngine()


def test_the_combinations_and_the_generator():
    """48 combinations; the committed cases hold every kind of operation; a sequence is a pure function of (seed, modes)"""
    assert len(COMBINATIONS) == len(set(COMBINATIONS)) == 48 and all(set(c) <= set(es.MODES) for c in COMBINATIONS)
    es.check_kinds([(seed, modes) for modes in COMBINATIONS for seed in SEEDS])
    for modes in COMBINATIONS:
        for seed in SEEDS:
            ops = es.generate(seed, modes)
            assert ops == es.generate(seed, modes) and len(ops) == es.LENGTH
    share = numpy.mean([op[0] in es.OBSERVATIONS for modes in COMBINATIONS for seed in SEEDS for op in es.generate(seed, modes)[2:-1]])
    assert 0.3 < share < 0.5, share                               # observation is sparse: about 40 % behind the forced head
    assert any(op[0] == "enable" for modes in COMBINATIONS for op in es.generate(1, modes))


@pytest.mark.parametrize("modes", COMBINATIONS, ids=es.name_of)
def test_every_mode_combination(modes):
    for seed in SEEDS:
        es.run(_oracle(), _oracle(), seed, modes, 3)


def test_the_old_sequences_are_unchanged():
    """the five new modes stand behind the old ones in the generator's bit mask, their kinds of operation have weight 0 and
    consume no draw where their mode is absent: every sequence of the 48 old combinations is what it was (CAUGHT_BY rows 1 to 8
    and the named regressions depend on it)"""
    h = hashlib.sha256()
    for modes in COMBINATIONS:
        for seed, length in ((1, 14), (2, 14), (3, 14), (101, 30)):
            h.update(repr((seed, modes, es.generate(seed, modes, length))).encode())
    assert h.hexdigest() == OLD_SEQUENCES


def test_the_sequences_of_the_eleven_modes_are_unchanged():
    """the same for the 55 combinations with K19 to K23 and the statistics, now that the three mixing modes stand behind them
    (CAUGHT_BY rows 9 to 18 depend on it)"""
    h = hashlib.sha256()
    for modes in NEW_COMBINATIONS:
        for seed, length in ((1, 14), (2, 14), (3, 14), (101, 30)):
            h.update(repr((seed, modes, es.generate(seed, modes, length))).encode())
    assert h.hexdigest() == NEW_SEQUENCES


def test_the_sequences_of_the_mixing_modes_are_unchanged():
    """the same for the 14 combinations with K24 and K25, now that "imix" stands behind them: the mutation "implicit" has weight 0
    and consumes no draw without it, and the bound of K26 in ``params`` comes from a generator of its own (CAUGHT_BY rows 19 to 26
    depend on it)"""
    h = hashlib.sha256()
    for modes in MIX_COMBINATIONS:
        for seed, length in ((1, 14), (2, 14), (3, 14), (101, 30)):
            h.update(repr((seed, modes, es.generate(seed, modes, length))).encode())
    assert h.hexdigest() == MIX_SEQUENCES
    h = hashlib.sha256()                                           # the six older entries of ``params``: the draw of kh_cap is not among theirs
    for modes in ALL_COMBINATIONS + MIX_COMBINATIONS:
        for seed in (1, 2, 3, 101):
            par = es.params(seed, modes)
            h.update(repr((seed, modes, [(k, par[k]) for k in ("kind", "limiter", "cap", "stability", "drag", "dx")])).encode())
    assert h.hexdigest() == OLD_PARAMS


def test_the_new_combinations_and_their_generator():
    """46 + 9 combinations; over the committed cases every kind of operation, both kinds of K19 and both limiters of K23 occur;
    every "qt" sequence hands the forcing over between two steps; the gravity wave of K21 never asks for more substeps than
    max_substeps, whatever spacing, Courant limit and wave speed ``enable`` uses"""
    assert len(NEW_COMBINATIONS) == len(set(NEW_COMBINATIONS)) == 55 and not set(NEW_COMBINATIONS) & set(COMBINATIONS)
    assert all(es.valid(c) and c == tuple(m for m in es.MODES if m in c) for c in NEW_COMBINATIONS + NEW_SIX)
    assert all(c in NEW_COMBINATIONS for c in NEW_SIX) and len(set(NEW_SIX)) == 6
    assert len(es.new_combinations(("advect", "vertical"))) == len(es.new_combinations(es.OLD_MODES)) == 23
    es.check_kinds([(seed, modes) for modes in ALL_COMBINATIONS for seed in SEEDS])
    es.check_kinds([(seed, modes) for modes in NEW_COMBINATIONS for seed in SEEDS])
    for modes in NEW_COMBINATIONS:
        for seed, length in [(s, es.LENGTH) for s in SEEDS] + [(101, 30)]:
            ops = es.generate(seed, modes, length)
            assert ops == es.generate(seed, modes, length) and len(ops) == length and es.params(seed, modes) == es.params(seed, modes)
            assert ("qt" in modes) == any(op[0] == "qt_forcings" for op in ops)
    par = [es.params(seed, modes) for modes in NEW_COMBINATIONS for seed in SEEDS]
    assert {p["kind"] for p, (modes, seed) in zip(par, [(m, s) for m in NEW_COMBINATIONS for s in SEEDS]) if "qt" in modes} == {"local", "strong"}
    assert {p["limiter"] for p, (modes, seed) in zip(par, [(m, s) for m in NEW_COMBINATIONS for s in SEEDS]) if "order2" in modes} == {"mc", "none"}
    assert any(op == ("enable", mode) for mode in ("qt", "buoyancy", "advect") for modes in NEW_COMBINATIONS for op in es.generate(1, modes))
    for dx, cfl in ((lvr.DX, adv.CFL), (1.25 * lvr.DX, 0.4), (es.READVECT["dx"], es.READVECT["cfl"])):
        for speed in (buo.WAVE_SPEED, es.LATE_WAVE_SPEED):
            assert buo.wave_substeps(max(es.DTS), dx, 1.5 * dx, cfl, speed) <= 4 < adv.MAX_SUBSTEPS


@pytest.mark.parametrize("modes", NEW_COMBINATIONS, ids=es.name_of)
def test_every_new_mode_combination(modes):
    for seed in SEEDS:
        es.run(_oracle(), _oracle(), seed, modes, 3)


def _longest_run(calls, name):
    return max([len(list(g)) for k, g in itertools.groupby(calls) if k == name], default=0)


def test_a_conservative_step_sums_the_lid_flux_over_substeps():
    """a committed conservative sequence holds a step of two substeps and more (K23 stands alone between the probe and K10, so its
    launches in a row are the substeps): the sum of the lid flux has something to add"""
    modes = ("advect", "vertical", "conservative", "order2")
    assert modes in NEW_COMBINATIONS
    assert max(_longest_run(es.run(_oracle(), _oracle(), seed, modes, 3), "les_transport2") for seed in SEEDS) >= 2


@pytest.mark.parametrize("modes", NEW_SIX, ids=es.name_of)
def test_new_modes_on_row_blocks_with_an_empty_device(modes):
    """three oracle engines, n = 2: blocks 1 + 1 + 0 (the Sharded branch of get_lid_flux_batched, _device_max with an empty part)"""
    for seed in SEEDS:
        multi = MultiDeviceEngine([_oracle() for _ in range(3)], min_cols_per_device=1)
        es.run(_oracle(), multi, seed, modes, 2)


@pytest.mark.parametrize("modes", NEW_SIX, ids=es.name_of)
def test_new_modes_behind_the_fused_step(monkeypatch, modes):
    """FUSED_MIN_LES patched to 0: K11 steps the fields and K19 reads its cached means"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    for seed in SEEDS:
        calls = es.run(_oracle(), _oracle(), seed, modes, 3)
        assert "les_advance" in calls


@pytest.mark.parametrize("modes", NEW_SIX, ids=es.name_of)
def test_new_modes_in_longer_sequences(modes):
    es.run(_oracle(), _oracle(), 101, modes, 3, length=30)


def _capped_steps(seed, modes, length=es.LENGTH):
    """the twin's ``mixing_capped`` of every step of the sequence that K25 follows"""
    ops, par = es.generate(seed, modes, length), es.params(seed, modes)
    late = es.check_sequence(ops, modes, par=par)
    twin, on, out = es.build(_oracle(), False, 3, modes, late, par), es._on_at_start(modes, late), []
    for op in ops:
        before = twin.model_time
        es.apply(twin, op, False, modes, on, par)
        if es._is_step(op) and "vmix" in on and twin.model_time > before:
            out.append(bool(twin.mixing_capped))
    return out


def test_the_mixing_combinations_and_their_generator():
    """14 combinations; over the committed cases every kind of operation occurs that their modes allow; the generator and the
    parameters are pure functions of (seed, modes); with K25 every pair of {stability on, off} x {drag on, off} occurs, the
    spacings of enable_mixing are defaulted and given, and there are steps whose cap binds and steps whose cap does not (one
    sequence and more holds both: the switch between the two viscosity buffers); a sequence of K25 with the drag holds a
    roughness length between two steps; each of the three refusals and a late enable of each mode occur"""
    assert len(MIX_COMBINATIONS) == len(set(MIX_COMBINATIONS)) == 14 and not set(MIX_COMBINATIONS) & set(ALL_COMBINATIONS)
    assert all(es.valid(c) and "mix" in c for c in MIX_COMBINATIONS) and all(c in MIX_COMBINATIONS for c in MIX_SIX) and len(set(MIX_SIX)) == 6
    assert es.mix_combinations(()) == [("mix",), ("mix", "vmix")] and es.mix_combinations(("diffuse",)) == [("diffuse", "mix"), ("diffuse", "mix", "kmix")]
    assert not es.valid(("mix", "vmix", "kmix", "diffuse")) and not es.valid(("vmix",)) and not es.valid(("mix", "kmix")) and not es.valid(("diffuse", "mix", "vmix"))
    cases = [(seed, modes) for modes in MIX_COMBINATIONS for seed in SEEDS]
    es.check_kinds(cases)
    for modes in MIX_COMBINATIONS:
        for seed, length in [(s, es.LENGTH) for s in SEEDS] + [(101, 30)]:
            ops = es.generate(seed, modes, length)
            assert ops == es.generate(seed, modes, length) and len(ops) == length and es.params(seed, modes) == es.params(seed, modes)
    par = {case: es.params(*case) for case in cases}
    with_k25 = [case for case in cases if "vmix" in case[1]]
    assert {(par[c]["stability"], par[c]["drag"]) for c in with_k25} == {(s, d) for s in (True, False) for d in (True, False)}
    assert {par[c]["dx"] for c in cases} == set(es.MIX_DX) and {par[c]["cap"] for c in cases} == set(es.MIX_CAPS)
    capped = [_capped_steps(*c) for c in with_k25]
    assert all(capped) and any(True in c and False in c for c in capped) and any(all(c) for c in capped) and any(not any(c) for c in capped)
    for seed, modes in with_k25:
        ops = es.generate(seed, modes)
        assert par[seed, modes]["drag"] <= any(op[0] == "z0m" for op in ops)
    seen = [op for seed, modes in cases for op in es.generate(seed, modes)]
    assert {op[1] for op in seen if op[0] == "refused"} == set(es.REFUSED)
    assert set(es.MIX_MODES) <= {op[1] for op in seen if op[0] == "enable"}


@pytest.mark.parametrize("modes", MIX_COMBINATIONS, ids=es.name_of)
def test_every_mixing_combination(modes):
    for seed in SEEDS:
        es.run(_oracle(), _oracle(), seed, modes, 3)


@pytest.mark.parametrize("modes", MIX_SIX, ids=es.name_of)
def test_mixing_on_row_blocks_with_an_empty_device(modes):
    """three oracle engines, n = 2: blocks 1 + 1 + 0 (one les_vmix per engine that holds rows, les_mix once or twice per each)"""
    for seed in SEEDS:
        multi = MultiDeviceEngine([_oracle() for _ in range(3)], min_cols_per_device=1)
        es.run(_oracle(), multi, seed, modes, 2)


@pytest.mark.parametrize("modes", MIX_SIX, ids=es.name_of)
def test_mixing_behind_the_fused_step(monkeypatch, modes):
    """FUSED_MIN_LES patched to 0: K11 steps the fields, K24 and K25 follow"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    for seed in SEEDS:
        calls = es.run(_oracle(), _oracle(), seed, modes, 3)
        assert "les_advance" in calls


@pytest.mark.parametrize("modes", MIX_SIX, ids=es.name_of)
def test_mixing_in_longer_sequences(modes):
    es.run(_oracle(), _oracle(), 101, modes, 3, length=30)


def test_the_implicit_combinations_and_their_generator():
    """14 combinations with "imix" and the six of the other runs; over the committed cases every kind of operation occurs; the
    generator and the parameters are pure; K26 is switched off and on again, one sequence and more holds steps of both paths and
    most switch; mix is enabled late with implicit=True and kmix behind an implicit mix; with K25 one sequence and more holds
    a step whose explicit cap binds (two les_mix) and an implicit step (one); there are implicit steps whose largest viscosity
    lies above the kh_cap in force and steps below it (ensemble_sequences.implicit_conditions asserts every count >= 1 and that
    more than half of the sequences switch; the counts observed with SEEDS over the 28 cases: 23 switches to explicit, 5 to
    implicit, 23 sequences that switch and 21 with steps of both paths, 9 late mix and 2 late kmix, 2 with K25 on both paths, 20
    implicit steps above the bound and 18 below)"""
    assert len(IMIX_COMBINATIONS) == len(set(IMIX_COMBINATIONS)) == 14 and not set(IMIX_COMBINATIONS) & set(ALL_COMBINATIONS + MIX_COMBINATIONS)
    assert all(es.valid(c) and c == tuple(m for m in es.MODES if m in c) for c in IMIX_COMBINATIONS) and not es.valid(("imix",)) and not es.valid(("diffuse", "imix"))
    assert all(c in IMIX_COMBINATIONS for c in IMIX_SIX) and len(set(IMIX_SIX)) == 6 and es.MODES[-1] == es.IMIX
    cases = [(seed, modes) for modes in IMIX_COMBINATIONS for seed in SEEDS]
    es.check_kinds(cases)
    es.check_kinds([(seed, modes) for modes in MIX_COMBINATIONS + IMIX_COMBINATIONS for seed in SEEDS])
    for modes in IMIX_COMBINATIONS:
        ops = es.generate(101, modes, 30)
        assert ops == es.generate(101, modes, 30) and len(ops) == 30
    assert {es.params(*c)["kh_cap"] for c in cases} == set(es.KH_CAPS)
    assert all(es.params(seed, modes)["kh_cap"] is None for modes in MIX_COMBINATIONS for seed in SEEDS)
    es.implicit_conditions(cases, _oracle())


@pytest.mark.parametrize("modes", IMIX_COMBINATIONS, ids=es.name_of)
def test_every_implicit_combination(modes):
    for seed in SEEDS:
        es.run(_oracle(), _oracle(), seed, modes, 3)


@pytest.mark.parametrize("modes", IMIX_SIX, ids=es.name_of)
def test_implicit_mixing_on_row_blocks_with_an_empty_device(modes):
    """three oracle engines, n = 2: blocks 1 + 1 + 0 (one les_mix and one les_hmix per engine that holds rows)"""
    for seed in SEEDS:
        multi = MultiDeviceEngine([_oracle() for _ in range(3)], min_cols_per_device=1)
        es.run(_oracle(), multi, seed, modes, 2)


@pytest.mark.parametrize("modes", IMIX_SIX, ids=es.name_of)
def test_implicit_mixing_behind_the_fused_step(monkeypatch, modes):
    """FUSED_MIN_LES patched to 0: K11 steps the fields, K26 and K25 follow"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    for seed in SEEDS:
        calls = es.run(_oracle(), _oracle(), seed, modes, 3)
        assert "les_advance" in calls


@pytest.mark.parametrize("modes", IMIX_SIX, ids=es.name_of)
def test_implicit_mixing_in_longer_sequences(modes):
    es.run(_oracle(), _oracle(), 101, modes, 3, length=30)


@pytest.mark.parametrize("modes", SIX, ids=es.name_of)
def test_row_blocks_with_an_empty_device(modes):
    """three oracle engines, n = 2: blocks 1 + 1 + 0"""
    for seed in SEEDS:
        multi = MultiDeviceEngine([_oracle() for _ in range(3)], min_cols_per_device=1)
        es.run(_oracle(), multi, seed, modes, 2)


@pytest.mark.parametrize("modes", SIX, ids=es.name_of)
def test_fused_step_then_every_later_stage(monkeypatch, modes):
    """FUSED_MIN_LES patched to 0: K11 steps the fields, whatever is enabled follows"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    for seed in SEEDS:
        calls = es.run(_oracle(), _oracle(), seed, modes, 3)
        assert "les_advance" in calls


@pytest.mark.parametrize("modes", SIX, ids=es.name_of)
def test_longer_sequences(modes):
    """30 operations: more caches meet each other (sequences of this length found two of the named cases below)"""
    es.run(_oracle(), _oracle(), 101, modes, 3, length=30)


# -- what the sequences found: named regression cases ----------------------------------------------------------------------------
#: thermo, a first step that no read precedes: the twin's p["QL"] (and so p["QL_ice"]) has to be the mean of its QL field
UNOBSERVED_FIRST_STEP = (("thermo",), [("step", 300.0), ("step0",), ("profiles", ("QL_ice",)), ("record",)])
#: a row getter behind a nudge (or set_fields_batched): row i of get_profiles_batched, not the means of the old fields
ROW_AFTER_NUDGE = ((), [("forcings", 1), ("step", 900.0), ("nudge", True, 11), ("row", 1, "get_profile_THL"), ("record",)])
ROW_AFTER_SET_FIELDS = (("thermo",), [("step", 450.0), ("set_field", "QT", 3), ("row", 2, "get_profile_T"), ("record",)])
#: a row's get_field("TWP") on both sides of a new Rhobf: the host copy of the water path is that of the new weights
ROW_WATER_PATH_AFTER_RHOBF = ((), [("forcings", 1), ("step", 900.0), ("row_wp", 0, "TWP"), ("rhobf",), ("row_wp", 0, "TWP"), ("record",)])
#: thermo, the microphysics enabled behind a new presf: K12 runs again (K14 needs the cells' temperature), in the twin as well
LATE_MICRO_AFTER_PRESF = (("thermo", "micro"), [("step", 300.0), ("presf",), ("enable", "micro"), ("field", "QL"), ("step", 300.0), ("record",)])
#: the statistics of W on both sides of a new Rhobf: get_vertical_wind_batched() is that of the new density, so are its moments
W_STATISTICS_AFTER_RHOBF = (("advect", "vertical", "stats"), [("forcings", 1), ("step", 300.0), ("stats", ("W",), ()), ("rhobf",), ("stats", ("W",), ()),
                                                             ("record",)])
#: ... and a new Rhobf costs only what holds W: the moments of U and the pair (THL, QT) are still cached and launch nothing
ONLY_W_STATISTICS_AFTER_RHOBF = (("advect", "vertical", "stats"), [
    ("forcings", 1), ("step", 300.0), ("stats", ("U", "W"), (("W", "THL"), ("THL", "QT"))), ("rhobf",), ("stats", ("U",), (("THL", "QT"),)),
    ("row_stats", 2, ("U", "W"), (("W", "THL"),)), ("record",)])
#: enable_mixing() a second time forgets the last step of the first: both viscosities, mixing_k_max and mixing_capped are None
#: until the next step (the twin kept them; a third element: the parameters that differ from es.DEFAULT)
SECOND_ENABLE_MIXING = (("mix", "vmix"), [("step", 300.0), ("remix", 0.1, 0.8), ("viscosity",), ("z0m", 3), ("step", 300.0), ("viscosity",), ("record",)])
#: enable_vertical_mixing() behind a step of K24 whose cap did not bind: there is no viscosity K25 mixed by before its first step
#: (the device ensemble returned K24's km there, and None where the cap had bound)
LATE_VERTICAL_MIXING = (("mix", "vmix"), [("step", 300.0), ("enable", "vmix"), ("viscosity",), ("z0m", 3), ("step", 300.0), ("viscosity",), ("record",)],
                        {"dx": 20000.0})
#: ... and the same behind enable_vertical_mixing() called again
SECOND_ENABLE_VERTICAL_MIXING = (("mix", "vmix"), [("step", 300.0), ("z0m", 3), ("revmix", 0.3, 400.0, True), ("viscosity",), ("step", 300.0), ("viscosity",),
                                                    ("record",)], {"dx": 20000.0})
#: the Courant numbers of engines that launch on streams of their own: _device_max read each engine's maximum on torch's current
#: stream, which does not wait for the engine's, so under a MultiDeviceEngine whose engines share a card the substeps and the
#: recorded sums were now and then those of recycled memory (seen at 130 LES, where the launches are long enough; the GPU module
#: replays this case there, test_the_courant_maximum_is_read_on_the_stream_that_made_it holds the ordering without a GPU)
COURANT_ON_OWN_STREAMS = (("advect", "vertical", "buoyancy"), [("forcings", 1), ("step", 900.0), ("courant",), ("step", 900.0), ("courant",), ("w",), ("record",)])
REGRESSIONS = {"courant on own streams": COURANT_ON_OWN_STREAMS, "second enable_mixing": SECOND_ENABLE_MIXING, "late vertical mixing": LATE_VERTICAL_MIXING,
               "second enable_vertical_mixing": SECOND_ENABLE_VERTICAL_MIXING, "unobserved first step": UNOBSERVED_FIRST_STEP, "row after nudge": ROW_AFTER_NUDGE, "row after set_fields": ROW_AFTER_SET_FIELDS,
               "row water path after Rhobf": ROW_WATER_PATH_AFTER_RHOBF, "late microphysics after presf": LATE_MICRO_AFTER_PRESF,
               "statistics of W after Rhobf": W_STATISTICS_AFTER_RHOBF, "only the statistics of W after Rhobf": ONLY_W_STATISTICS_AFTER_RHOBF}


@pytest.mark.parametrize("name", sorted(REGRESSIONS))
def test_named_regressions(name):
    modes, ops, par = _regression(name)
    es.replay(ops, modes, 3, _oracle(), _oracle(), what=name, par=par)


def _regression(name):
    modes, ops = REGRESSIONS[name][:2]
    return modes, ops, dict(es.DEFAULT, **(REGRESSIONS[name][2] if len(REGRESSIONS[name]) > 2 else {}))


def test_the_courant_maximum_is_read_on_the_stream_that_made_it():
    """_device_max forms every engine's maximum AND reads it to the host inside that engine's on_stream(): a read on torch's
    current stream would not wait for an engine that launches on a stream of its own"""
    import contextlib
    active, events = [], []

    class Scalar:
        def __init__(self, owner, value):
            self.owner, self.value = owner, value

        def item(self):
            events.append(("item", self.owner.name, list(active)))
            return self.value

    class Part:
        def __init__(self, owner, value):
            self.owner, self.value = owner, value

        def numel(self):
            return 1

        def max(self):
            events.append(("max", self.owner.name, list(active)))
            return Scalar(self.owner, self.value)

    class StreamEngine:
        def __init__(self, name):
            self.name = name

        @contextlib.contextmanager
        def on_stream(self):
            active.append(self.name)
            try:
                yield
            finally:
                active.pop()
    a, b = StreamEngine("a"), StreamEngine("b")
    ens = models.DeviceLESEnsemble.__new__(models.DeviceLESEnsemble)
    ens.engine = type("Two", (), {"engines": [a, b]})()
    got = ens._device_max(type("Blocks", (), {"parts": [Part(a, 0.25), Part(b, 0.75)]})())
    assert got == 0.75 and sorted(e[:2] for e in events) == [("item", "a"), ("item", "b"), ("max", "a"), ("max", "b")]
    assert all(on == [name] for _, name, on in events), events


def test_without_the_twin_fix_a_second_enable_mixing_keeps_the_last_step(monkeypatch):
    inner = lvm._HostVmix.enable_mixing

    def old(self, *a, **kw):
        kept = self.mixing_k_max, self.mixing_capped, self._kv
        inner(self, *a, **kw)
        self.mixing_k_max, self.mixing_capped, self._kv = kept
    monkeypatch.setattr(lvm._HostVmix, "enable_mixing", old)
    modes, ops, par = _regression("second enable_mixing")
    with pytest.raises(AssertionError, match=r"operation 2 .*kv"):
        es.replay(ops, modes, 3, _oracle(), _oracle(), par=par)


@pytest.mark.parametrize("name", ["late vertical mixing", "second enable_vertical_mixing"])
def test_without_the_flag_k24s_viscosity_is_taken_for_that_of_k25(monkeypatch, name):
    """get_vertical_viscosity_batched() as it was: K24's km of a step that ran before enable_vertical_mixing()"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "get_vertical_viscosity_batched",
                        _edited("get_vertical_viscosity_batched", "self.vertical_mixing and self._vmix_stepped", "self.vertical_mixing"))
    modes, ops, par = _regression(name)
    with pytest.raises(AssertionError, match=r"operation 3 .*kv" if name.startswith("second") else r"operation 2 .*kv"):
        es.replay(ops, modes, 3, _oracle(), _oracle(), par=par)


def test_without_the_twin_fix_the_unobserved_first_step_fails(monkeypatch):
    monkeypatch.setattr(ltr.HostThermoLESEnsemble, "_slab_means", slab_ref.HostFieldLESEnsemble._slab_means)
    modes, ops = UNOBSERVED_FIRST_STEP
    with pytest.raises(AssertionError, match="QL_ice"):
        es.replay(ops, modes, 3, _oracle(), _oracle())


@pytest.mark.parametrize("name", ["row after nudge", "row after set_fields"])
def test_without_the_row_getter_fix_property_a_fails(monkeypatch, name):
    """the device rows read the raw p again: the row is not that of get_profiles_batched"""
    for method, key in es.ROW_GETTERS.items():
        monkeypatch.setattr(models._DeviceLESRow, method, models._row_getter(key))
    modes, ops = REGRESSIONS[name]
    with pytest.raises(AssertionError, match=r"\(a\) row"):
        es.replay(ops, modes, 3, _oracle(), _oracle())


def test_without_the_host_copy_fix_the_row_water_path_is_that_of_the_old_weights(monkeypatch):
    def old(self, name):
        if name not in self._wp_host or self._wp is None or name not in self._wp:
            t = self.get_water_paths_batched((name,))[name]
            with self._eng().on_stream():
                self._wp_host[name] = numpy.asarray(self._host(t))
        return self._wp_host[name]
    monkeypatch.setattr(models.DeviceLESEnsemble, "_water_path_host", old)
    modes, ops = ROW_WATER_PATH_AFTER_RHOBF
    with pytest.raises(AssertionError, match=r"operation 4 .* TWP"):
        es.replay(ops, modes, 3, _oracle(), _oracle())


def test_without_the_twin_fix_the_late_microphysics_keeps_the_old_presf(monkeypatch):
    inner = lmr._HostMicro.enable_microphysics

    def old(self, **kw):
        stale = self._stale
        inner(self, **kw)
        self._stale = stale
    monkeypatch.setattr(lmr._HostMicro, "enable_microphysics", old)
    modes, ops = LATE_MICRO_AFTER_PRESF
    with pytest.raises(AssertionError, match=r"operation 3 .* QL"):
        es.replay(ops, modes, 3, _oracle(), _oracle())


def test_without_the_key_the_statistics_of_w_are_those_of_the_old_density(monkeypatch):
    """W taken once per change of the fields, whatever p["Rhobf"] is by now: the cached moments of the old W come back"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "_statistics_fields",
                        _edited("_statistics_fields", "_kept(old, key, ", "_kept(old, key if old is None else old[0], "))
    modes, ops = W_STATISTICS_AFTER_RHOBF
    with pytest.raises(AssertionError, match=r"operation 4 .*stat mean W"):
        es.replay(ops, modes, 3, _oracle(), _oracle())


def test_without_the_partial_drop_a_new_rhobf_costs_every_moment(monkeypatch):
    """a new Rhobf that drops the whole cache gives the right numbers and launches K20 for moments that W does not enter"""
    def everything(self):
        self._stats, self._stats_host = None, {}
    monkeypatch.setattr(models.DeviceLESEnsemble, "_drop_w_statistics", everything)
    modes, ops = W_STATISTICS_AFTER_RHOBF
    es.replay(ops, modes, 3, _oracle(), _oracle())
    modes, ops = ONLY_W_STATISTICS_AFTER_RHOBF
    with pytest.raises(AssertionError, match=r"operation 4 .*\(c\) K20 launched"):
        es.replay(ops, modes, 3, _oracle(), _oracle())


# -- state mutants ---------------------------------------------------------------------------------------------------------------
def _edited(method, old, new):
    """``method`` of DeviceLESEnsemble with ``old`` (which occurs exactly once in its source) replaced by ``new``; of a method
    under ``models._timed`` the function inside the wrapper is edited and wrapped again (its source holds the decorator)"""
    fn = getattr(models.DeviceLESEnsemble, method)
    fn = next((c.cell_contents for c in fn.__closure__ or () if getattr(c.cell_contents, "__name__", None) == method), fn)
    src = textwrap.dedent(inspect.getsource(fn))
    assert src.count(old) == 1, (method, old, src.count(old))
    ns = dict(vars(device_les))
    exec(compile(src.replace(old, new), "<state mutant of %s>" % method, "exec"), ns)
    return ns[method]


MUTANTS = {
    1: ("_drop_water_paths", None, None),
    2: ("set_fields_batched", "    self._thermo_stale = True", "    pass"),
    3: ("set_fields_batched", "    self._means = None\n", "    pass\n"),
    4: ("_diffuse", "_kept(self._diffuse_prof, key, ", "_kept(self._diffuse_prof, key if self._diffuse_prof is None else self._diffuse_prof[0][:1] + key[1:], "),
    5: ("_microphysics", "_kept(self._micro_prof, key, ",
        "_kept(self._micro_prof, key if self._micro_prof is None else key[:2] + self._micro_prof[0][2:3] + key[3:], "),
    6: ("_microphysics", 'f["QR"], self._qr_spare = self._qr_spare, f["QR"]', "pass"),
    7: ("get_water_paths_batched", "_kept(old, w, ", "_kept(old, w if old is None else old[0], "),
    8: ("set_fields_batched", "    self.fields3d[name] = values\n    self._means = None\n",
        "    same = self.fields3d.get(name) is values\n    self.fields3d[name] = values\n    self._means = self._means if same else None\n"),
    9: ("_drop_statistics", None, None),
    10: ("_drop_statistics", "self._stats, self._stats_host, self._stats_w = None, {}, None", "self._stats, self._stats_w = None, None"),
    11: ("_qt_local", "self._thermo_stale, self._means = True, None      # thermo: K12 runs on the new QT before its next use\n"
                      "    if not (self.advection or self.diffusion):", "if False:"),
    12: ("_buoyancy_profiles", 'p["presf"], self.zh_cache)', '(p["presf"] if self._buoyancy_prof is None else self._buoyancy_prof[0][3]), self.zh_cache)'),
    13: ("_transport", "self._per_device(torch.add, total, ftop)", "self._per_device(torch.clone, ftop)"),
    14: ("enable_qt_forcing", "self.qt_forcing_kind, self._qt_counts = kind, None", "self.qt_forcing_kind = kind"),
    15: ("enable_advection", "self.advect_conservative, self._transport_ftop, self._transport_lid = bool(conservative), None, None",
         "self.advect_conservative, self._transport_ftop = bool(conservative), None"),
    16: ("enable_advection", "self.buoyancy = False", "pass"),
    17: ("_drop_w_statistics", "self._stats_host = {kk: a for kk, a in self._stats_host.items() if not holds(kk[1])}", "pass"),
    18: ("_statistics_fields", "_kept(old, key, ", "_kept(old, key if old is None else old[0], "),
    19: ("_mix", "        f[k], spare[k] = spare[k], f[k]\n", "        pass\n"),
    20: ("_mix", "_kept(self._mix_coef, ckey, ", "_kept(self._mix_coef, ckey if self._mix_coef is None else self._mix_coef[0][:1] + ckey[1:], "),
    21: ("_vmix", "_kept(self._vmix_coef, key, ", "_kept(self._vmix_coef, key if self._vmix_coef is None else key[:4] + self._vmix_coef[0][4:5] + key[5:], "),
    22: ("_vmix", "_f64(numpy.asarray(self.tend[self.VMIX_Z0M], dtype=numpy.float64).reshape(self.n), ",
         "_f64(numpy.asarray(self.tend[self.VMIX_Z0M], dtype=numpy.float64).reshape(self.n) if self._vmix_drag is None else self._vmix_drag[0][1], "),
    23: ("_mix", "eng.les_mix({}, {}, u, v, theta, gx, gy, gz, bz if theta is not None else None, l2, self._vmix_huge, self._vmix_km, {}, {}, kmax=False)",
         "self._vmix_km = self._mix_km"),
    24: ("_mix", "eng.les_mix({}, {}, u, v, theta, ", 'eng.les_mix({}, {}, f["U"], f["V"], theta, '),
    25: ("enable_mixing", "self._mix_prof = self._mix_coef = self._mix_km = self._mix_kd = None", "self._mix_prof = self._mix_coef = self._mix_kd = None"),
    26: ("_diffuse", "        key += (kd,)\n",
         "        kd = kd if self._diffuse_prof is None or len(self._diffuse_prof[0]) == len(key) else self._diffuse_prof[0][-1]\n        key += (kd,)\n"),
    27: ("_mix_implicit", "l2, self._hmix_huge, self._mix_km, ", "l2, self._mix_coef[3], self._mix_km, "),
    28: ("_mix_implicit", "    self._mix_tail()\n", "    pass\n"),
    29: ("_mix_implicit", "self.mixing_capped = False", "pass"),
    30: ("_mix_implicit", 'self._upload(hmx.bound(self.n, par["kh_cap"]))', "self._upload(hmx.bound(self.n))"),
    31: ("enable_mixing", '"implicit": bool(implicit),', '"implicit": bool(implicit) or bool(self.mix_par and self.mix_par["implicit"]),'),
    32: ("_mix_implicit", "self.mixing_k_max = self._device_max(top)", "pass"),
}
#: faults of K26's state that are guarded twice and show in NO committed sequence (test_twice_guarded_faults_do_not_show)
TWICE_GUARDED = {
    "enable_mixing keeps _hmix_kh2": ("enable_mixing", "self._hmix_huge = self._hmix_kh2 = None", "self._hmix_huge = None"),
    "enable_mixing keeps _hmix_huge": ("enable_mixing", "self._hmix_huge = self._hmix_kh2 = None", "self._hmix_kh2 = None"),
    "enable_mixing keeps _mix_spare": ("enable_mixing", "    self._mix_spare = {}\n", "    self._mix_spare = self._mix_spare or {}\n"),
}
AV = ("advect", "vertical")
CAUGHT_BY = {
    1: [(1, ()), (1, ("thermo",))],
    2: [(1, ("thermo", "diffuse")), (2, ("thermo", "advect"))],
    3: [(2, ("diffuse",)), (1, ("micro",))],
    4: [(1, ("diffuse",)), (2, ("diffuse",))],
    5: [(1, ("thermo", "micro")), (1, ("micro", "advect", "vertical"))],
    6: [(1, ("micro",)), (2, ("thermo", "micro"))],
    7: [(1, ()), (2, ("thermo",))],
    8: [(1, ("thermo", "diffuse")), (2, ("thermo", "advect"))],
    9: [(1, AV + ("stats",)), (2, AV + ("stats",))],
    10: [(1, AV + ("stats",)), (2, AV + ("stats",))],
    11: [(1, ("qt",)), (2, ("qt",))],
    12: [(2, AV + ("buoyancy", "conservative")), (1, es.OLD_MODES + ("qt", "buoyancy"))],
    13: [(2, AV + ("qt", "conservative")), (2, AV + ("buoyancy", "conservative"))],
    14: [(2, AV + ("qt", "stats")), (1, es.OLD_MODES + ("qt", "conservative", "stats"))],
    15: [(2, AV + ("buoyancy", "conservative", "order2")), (2, AV + ("qt", "buoyancy", "conservative", "order2"))],
    16: [(2, AV + ("buoyancy",)), (2, AV + ("buoyancy", "conservative", "order2"))],
    17: [(1, AV + ("buoyancy", "stats")), (2, AV + ("buoyancy", "stats"))],
    18: [(1, AV + ("buoyancy", "stats")), (2, AV + ("buoyancy", "stats"))],
    19: [(1, ("mix",)), (2, ("mix", "vmix"))],
    20: [(1, ("mix",)), (2, ("mix", "vmix")), (2, ("mix", "vmix", "imix"))],
    21: [(1, ("qt", "stats", "mix", "vmix")), (2, AV + ("buoyancy", "stats", "mix", "vmix"))],
    22: [(2, ("mix", "vmix")), (1, AV + ("buoyancy", "conservative", "order2", "mix", "vmix"))],
    23: [(1, ("mix", "vmix")), (2, ("mix", "vmix"))],
    24: [(1, ("mix", "vmix")), (2, ("mix", "vmix"))],
    25: [(1, ("mix",)), (2, ("diffuse", "mix", "kmix")), (1, ("mix", "imix"))],
    26: [(1, ("diffuse", "mix", "kmix")), (2, ("diffuse",) + AV + ("buoyancy", "conservative", "order2", "mix", "kmix"))],
    27: [(2, ("mix", "imix")), (2, ("mix", "vmix", "imix"))],
    28: [(1, ("mix", "imix")), (1, ("diffuse", "mix", "kmix", "imix"))],
    29: [(1, ("mix", "imix")), (1, ("mix", "vmix", "imix"))],
    30: [(1, ("mix", "imix")), (2, ("mix", "vmix", "imix"))],
    31: [(1, ("mix", "imix")), (2, ("diffuse", "mix", "kmix", "imix"))],
    32: [(1, ("mix", "imix")), (2, ("mix", "vmix", "imix"))],
}


def plant(monkeypatch, mutant):
    method, old, new = MUTANTS[mutant]
    monkeypatch.setattr(models.DeviceLESEnsemble, method, (lambda self: None) if old is None else _edited(method, old, new))


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_state_mutants_fail_a_committed_sequence(monkeypatch, mutant):
    """each fault of the ensemble's caches, patched into DeviceLESEnsemble, fails the sequences the table names (all of them
    among those of test_every_mode_combination, those of the mutants 9 to 18 among those of test_every_new_mode_combination,
    those of the mutants 19 to 26 among those of test_every_mixing_combination, those of the mutants 27 and up among those of
    test_every_implicit_combination, two and more each; the rows of the mutants 20 and 25 hold a third with "imix": the same fault
    shows on the path of K26); the same sequences pass without it"""
    assert all(seed in SEEDS and modes in (COMBINATIONS if mutant <= 8 else NEW_COMBINATIONS if mutant <= 18 else MIX_COMBINATIONS if mutant <= 26 else
                                           IMIX_COMBINATIONS) for seed, modes in CAUGHT_BY[mutant][:2])
    assert all(seed in SEEDS and modes in IMIX_COMBINATIONS for seed, modes in CAUGHT_BY[mutant][2:])
    assert len(CAUGHT_BY[mutant]) == (3 if mutant in (20, 25) else 2) or mutant <= 8
    assert len(set(CAUGHT_BY[mutant])) == len(CAUGHT_BY[mutant]) >= (1 if mutant <= 8 else 2)
    for seed, modes in CAUGHT_BY[mutant]:
        es.run(_oracle(), _oracle(), seed, modes, 3)
    plant(monkeypatch, mutant)
    for seed, modes in CAUGHT_BY[mutant]:
        with pytest.raises(AssertionError, match="operation"):
            es.run(_oracle(), _oracle(), seed, modes, 3)


@pytest.mark.parametrize("name", sorted(TWICE_GUARDED))
def test_twice_guarded_faults_do_not_show(monkeypatch, name):
    """what the docstring of this module says of them: every committed sequence with "imix" passes with the fault planted"""
    method, old, new = TWICE_GUARDED[name]
    monkeypatch.setattr(models.DeviceLESEnsemble, method, _edited(method, old, new))
    for modes in IMIX_COMBINATIONS:
        for seed in SEEDS:
            es.run(_oracle(), _oracle(), seed, modes, 3)


def test_a_failure_names_its_sequence_and_replay_reproduces_it(monkeypatch):
    """the message of a failing sequence holds the seed, the modes, the index of the operation and the operations up to it;
    that list, pasted into replay, fails at the same operation"""
    seed, modes = CAUGHT_BY[6][0]
    plant(monkeypatch, 6)
    with pytest.raises(AssertionError) as first:
        es.run(_oracle(), _oracle(), seed, modes, 3)
    text = str(first.value)
    at = int(re.search(r"operation (\d+) ", text).group(1))
    ops = es.generate(seed, modes)
    assert "seed %d" % seed in text and "modes %s" % es.name_of(modes) in text and repr(list(ops[:at + 1])) in text
    printed = eval(text.split("\n")[2])                            # the list as it was printed
    assert printed == list(ops[:at + 1])
    with pytest.raises(AssertionError, match="operation %d " % at):
        es.replay(ops, modes, 3, _oracle(), _oracle())


# -- float32: the same sequences on float32 engines against the float32 twin ------------------------------------------------------
#: The twin has a dtype T (tests/slab_ref.HostFieldLESEnsemble states the rule: fields and kernel outputs are T; what the host forms
#: is float64 and rounded once where a kernel takes it; the step is (tend.astype(T) * T(dt)).astype(T) and one add; what comes back
#: enters p widened exactly; a comparison of the host uses the rounded value on both sides).  ensemble_sequences.build hands the
#: twin the dtype of the engine its nudge runs on, and every comparison of a device tensor requires one dtype (assert_bits(...,
#: dtypes=True)).  The generator, the seeds and the 24 combinations are those of the float64 runs above.
F32_CASES = SIX + NEW_SIX + MIX_SIX + IMIX_SIX
OracleEngine32 = f32_of(lhr.HmixOracleEngine)


def _oracle32():
    return OracleEngine32()


def test_the_float32_twin_is_float32_and_is_not_the_float64_twin():
    """the fields of the float32 twin are float32 at the end of a sequence, its profiles float64 holding float32 values where a
    kernel made them, and they differ from the float64 twin's; with dtype=float64 every astype of the rule is the identity"""
    modes = ("thermo", "diffuse", "micro", "advect", "vertical", "radiate")
    ops, par = es.generate(1, modes), es.params(1, modes)
    late = es.check_sequence(ops, modes, par=par)
    rec = {}
    for eng in (_oracle(), _oracle32()):
        twin, on = es.build(eng, False, 3, modes, late, par), es._on_at_start(modes, late)
        assert twin.dtype == NP[eng.dtype]
        for op in ops:
            got = es.apply(twin, op, False, modes, on, par)
        rec[eng.dtype] = got
        assert all(a.dtype == NP[eng.dtype] for a in twin.fields3d.values()) and twin.rain2d.dtype == NP[eng.dtype]
    lo, hi = rec[torch.float32], rec[torch.float64]
    assert list(lo) == list(hi)
    for k in ("field U", "field QT", "field QL", "field QR", "LWP", "rain2d", "flux", "W"):
        assert lo[k].dtype == numpy.float32 and hi[k].dtype == numpy.float64, k
        assert not numpy.array_equal(lo[k], hi[k]) and numpy.allclose(lo[k], hi[k], rtol=1e-2, atol=1e-5 * numpy.abs(hi[k]).max()), k
    for k in ("p THL", "p QT", "p QR", "p Rain", "got U", "mean TWP"):
        assert numpy.asarray(lo[k]).dtype in (numpy.float64, numpy.float32) and numpy.array_equal(lo[k], numpy.asarray(lo[k]).astype(numpy.float32)), k
    assert lo["p PS"].dtype == numpy.float64 and not numpy.array_equal(lo["p PS"], lo["p PS"].astype(numpy.float32))    # host arithmetic stays float64


def test_float32_generator_conditions():
    """measured on the float32 twin alone and asserted (ensemble_sequences.dtype_conditions): the float32 runs of F32_CASES with
    SEEDS reach steps of more than one substep and of one, a cap of K24 that binds and one that does not, both signs of K19's a,
    implicit steps above and below kh_cap and rain on the ground.  The counts observed, the same on the float64 twin: 30 steps of
    more than one substep and 31 of one, 37 capped and 11 uncapped, 285 levels with a > 0 and 563 with a < 0, 10 implicit steps
    above the bound and 8 below, 38 steps of K14 with rain on the ground: no committed seed loses a condition in float32"""
    cases = [(seed, modes) for modes in F32_CASES for seed in SEEDS]
    assert len(set(F32_CASES)) == 24
    count = es.dtype_conditions(cases, _oracle32())
    assert all(v >= 1 for v in count.values()), count
    for table in (SIX, NEW_SIX, MIX_SIX, IMIX_SIX):               # (each family alone reaches what its modes allow: asserted inside)
        es.dtype_conditions([(seed, modes) for modes in table for seed in SEEDS], _oracle32())


@pytest.mark.parametrize("modes", F32_CASES, ids=es.name_of)
def test_float32_sequences_equal_the_float32_twin(modes):
    for seed in SEEDS:
        es.run(_oracle32(), _oracle32(), seed, modes, 3)


@pytest.mark.parametrize("modes", F32_CASES, ids=es.name_of)
def test_float32_on_row_blocks_with_an_empty_device(modes):
    """three float32 oracle engines, n = 2: blocks 1 + 1 + 0"""
    for seed in SEEDS:
        multi = MultiDeviceEngine([_oracle32() for _ in range(3)], min_cols_per_device=1)
        es.run(_oracle32(), multi, seed, modes, 2)


@pytest.mark.parametrize("name", sorted(REGRESSIONS))
def test_float32_named_regressions(name):
    modes, ops, par = _regression(name)
    es.replay(ops, modes, 3, _oracle32(), _oracle32(), what=name + " (float32)", par=par)


def test_a_float64_array_of_float32_values_is_no_float32_field():
    """assert_bits(..., dtypes=True), the comparison of every device tensor of a sequence: equal values of another dtype fail"""
    a = numpy.arange(6, dtype=numpy.float32) / 3
    gpu_util.assert_bits("same", a, a.copy(), dtypes=True)
    gpu_util.assert_bits("values alone", a.astype(numpy.float64), a)
    with pytest.raises(AssertionError, match="dtype float64, expected float32"):
        gpu_util.assert_bits("widened", a.astype(numpy.float64), a, dtypes=True)
    with pytest.raises(AssertionError, match="W: dtype"):
        es._compare("W", a.astype(numpy.float64), a)


# -- slips of the rounding rule ----------------------------------------------------------------------------------------------------
#: (method, old, new) edits of device_les.py as in MUTANTS.  Each leaves every float64 bit where it is (the float64 sequences of
#: its DTYPE_CAUGHT_BY entry pass with it planted: asserted) and fails those sequences in float32 (asserted).
#:   1  the step as (tend64 * dt).to(T): the product formed in float64 and rounded once
#:   2  K15's face diffusivity from a float64 mean of km (the launch of K10 still runs; its result is not used)
#:   3  K21's profiles t0, lex and s from a presf that was rounded to T first
#:   4  the weights Rhobf dz (K13's w, K17's g and r) as the product of two rounded factors
#:   5  K12's Exner factor from a presf that was rounded to T first
#:   6  K15's a, m, cp and s0 from a Rhobf that was rounded to T first
#:   7  K14's profiles from a presf that was rounded to T first
_ROUNDED = "numpy.asarray(self._host(self._upload(%s)), dtype=numpy.float64)"
DTYPE_MUTANTS = {
    1: ("evolve_model_batched", "self._per_device(step, f[key], self._upload(self.tend[key]))",
        "self._per_device(lambda field, inc: field.add_(inc[:, None, None, :]), f[key], self._upload(numpy.asarray(self.tend[key], dtype=numpy.float64) * dt))"),
    2: ("_mix_tail", 'm = self._to_host(eng.slab_means({"km": self._mix_km}))["km"]',
        'm = self._to_host(eng.slab_means({"km": self._mix_km}))["km"]\n'
        '        m = numpy.stack([x.mean(axis=(0, 1)) for x in numpy.asarray(self._host(self._mix_km), dtype=numpy.float64)])'),
    3: ("_buoyancy_profiles", "key[0], key[1], key[2] if has_ql else None, key[3], key[4]",
        "key[0], key[1], key[2] if has_ql else None, " + _ROUNDED % "key[3]" + ", key[4]"),
    4: ("water_path_weights", 'return numpy.asarray(self.p["Rhobf"], dtype=numpy.float64) * dz',
        "return " + _ROUNDED % 'numpy.asarray(self.p["Rhobf"], dtype=numpy.float64)' + " * " + _ROUNDED % "dz"),
    5: ("_ensure_thermo", "self._upload(th.exner(presf))", "self._upload(th.exner(" + _ROUNDED % "presf" + "))"),
    6: ("_diffuse", "df.profiles(key[5], key[6], key[4], dt, ", "df.profiles(key[5], key[6], " + _ROUNDED % "key[4]" + ", dt, "),
    7: ("_microphysics", "mp.profiles(key[4], key[5], key[3], key[2], dt, ", "mp.profiles(key[4], key[5], key[3], " + _ROUNDED % "key[2]" + ", dt, "),
}
KMIX = ("diffuse", "mix", "kmix")
DTYPE_CAUGHT_BY = {
    1: [(1, ()), (2, ("micro", "radiate"))],
    2: [(1, KMIX), (2, KMIX + (es.IMIX,))],
    3: [(1, AV + ("buoyancy", "conservative", "order2")), (2, es.ELEVEN)],
    4: [(1, ()), (2, ("diffuse", "advect", "vertical"))],
    5: [(1, ("thermo", "micro")), (2, ("thermo", "diffuse", "advect", "radiate"))],
    6: [(1, ("diffuse", "advect", "vertical")), (2, ("diffuse", "micro", "qt"))],
    7: [(2, ("diffuse", "micro", "qt")), (1, es.ELEVEN)],
}
#: edits that are NOT counted among the slips.  The first changes no float32 bit: under K26 the probe's cap becomes +inf in
#: float32 (finfo(float64).max rounds to it), and min(k, +inf) is k for every k the closure forms; NaN passes either cap.  The
#: second is a slip that no committed sequence shows: ``mixing_capped`` differs only where the largest viscosity of a step lies
#: between the float64 cap and its rounding, an interval of half an ulp.
DTYPE_EQUIVALENT = {
    "the cap that never binds from finfo(float64)": ("_mix_implicit", "float(torch.finfo(eng.dtype).max)", "float(torch.finfo(torch.float64).max)"),
    "lowest from the float64 mix.cap": ("_mix", "float(self._host(kcap).min())", 'float(mix.cap(wind, scalar, par["cap"]).min())'),
}


@pytest.mark.parametrize("mutant", sorted(DTYPE_MUTANTS))
def test_rounding_slips_pass_float64_and_fail_float32(monkeypatch, mutant):
    """each slip of the rounding rule, patched into DeviceLESEnsemble: the float64 sequences of its DTYPE_CAUGHT_BY entry stay
    bit-equal to the twin, the same sequences in float32 fail; without it both pass (all among F32_CASES and SEEDS)"""
    method, old, new = DTYPE_MUTANTS[mutant]
    cases = [(seed, tuple(m for m in es.MODES if m in modes)) for seed, modes in DTYPE_CAUGHT_BY[mutant]]
    assert len(set(cases)) >= 2 and all(seed in SEEDS and modes in F32_CASES for seed, modes in cases)
    for seed, modes in cases:
        es.run(_oracle32(), _oracle32(), seed, modes, 3)
    monkeypatch.setattr(models.DeviceLESEnsemble, method, _edited(method, old, new))
    for seed, modes in cases:
        es.run(_oracle(), _oracle(), seed, modes, 3)
        with pytest.raises(AssertionError, match="operation"):
            es.run(_oracle32(), _oracle32(), seed, modes, 3)


@pytest.mark.parametrize("name", sorted(DTYPE_EQUIVALENT))
def test_equivalent_edits_change_no_committed_bit(monkeypatch, name):
    """what DTYPE_EQUIVALENT says of them: every float32 and float64 sequence with the mixing passes with the edit planted"""
    method, old, new = DTYPE_EQUIVALENT[name]
    monkeypatch.setattr(models.DeviceLESEnsemble, method, _edited(method, old, new))
    for modes in MIX_SIX + IMIX_SIX:
        for seed in SEEDS:
            es.run(_oracle32(), _oracle32(), seed, modes, 3)
            es.run(_oracle(), _oracle(), seed, modes, 3)
