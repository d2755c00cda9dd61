"""Random operation sequences of models.DeviceLESEnsemble on oracle-backed engines against its NumPy twin, without a GPU
(the body: tests/ensemble_sequences.py): all 48 valid combinations of the six old modes and 55 with the five new ones (K19
to K23 and the statistics of K20) with two seeds, row blocks 1 + 1 + 0 of a MultiDeviceEngine, the fused K11 step in front of
every later stage, sequences of 30 operations, the digest of the old sequences (they are what they were before the new modes),
the named regression sequences of what the sequences found, and the state mutants: faults of the ensemble's caches, patched in, that a committed sequence has to notice.

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
(test_state_mutants_fail_a_committed_sequence asserts every line of this table.  Mutant 11 takes the call of _follow_fields
with the assignment: the assignment alone is redundant, every path behind K19 ends in _follow_fields, which sets both.  Mutant
12 reads the presf of the last upload into the key AND the profiles; a key that only COMPARES without presf never shows,
because the slab means in the same key change with every step.)"""
import hashlib
import inspect
import itertools
import re
import textwrap

import numpy
import pytest

from sp_coupler_amd import advection as adv
from sp_coupler_amd import buoyancy as buo
from sp_coupler_amd import device_les, models, spcpl
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import ensemble_sequences as es
from tests import les_full_ref as lfr
from tests import les_micro_ref as lmr
from tests import les_thermo_ref as ltr
from tests import les_vadvect_ref as lvr
from tests import slab_ref

SEEDS = (1, 2)
COMBINATIONS = es.combinations()
SIX = [(), ("thermo", "micro"), ("diffuse", "advect", "vertical"), ("micro", "radiate"), ("thermo", "diffuse", "advect", "radiate"), es.OLD_MODES]
#: the 23 non-empty valid subsets of the five new modes over the smallest background that takes them all and over all six old
#: modes, and the two modes that need no advection over three backgrounds without it: 46 + 9 combinations
NEW_COMBINATIONS = es.new_combinations(("advect", "vertical")) + es.new_combinations(es.OLD_MODES) + \
    [bg + c for bg in ((), ("thermo",), ("diffuse", "micro")) for c in (("qt",), ("stats",), ("qt", "stats"))]
ALL_COMBINATIONS = COMBINATIONS + NEW_COMBINATIONS
NEW_SIX = [("advect", "vertical", "qt", "conservative"), ("advect", "vertical", "buoyancy", "order2", "conservative"), ("advect", "vertical", "stats"),
           ("thermo", "qt", "stats"), ("diffuse", "micro", "qt"), es.MODES]
NEW_SIX = [tuple(m for m in es.MODES if m in c) for c in NEW_SIX]
#: sha256 over repr((seed, modes, generate(seed, modes, length))) of the 48 old combinations, seeds 1, 2 and 3 at length 14 and seed
#: 101 at length 30, computed from tests/ensemble_sequences.py as it was before the five new modes
OLD_SEQUENCES = "d5ab020b0faa71f622d7b6a095a2e44e9c9e763bb95676f71aad60aaf78766eb"


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def _oracle():
    return lfr.FullOracleEngine()


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
REGRESSIONS = {"unobserved first step": UNOBSERVED_FIRST_STEP, "row after nudge": ROW_AFTER_NUDGE, "row after set_fields": ROW_AFTER_SET_FIELDS,
               "row water path after Rhobf": ROW_WATER_PATH_AFTER_RHOBF, "late microphysics after presf": LATE_MICRO_AFTER_PRESF,
               "statistics of W after Rhobf": W_STATISTICS_AFTER_RHOBF, "only the statistics of W after Rhobf": ONLY_W_STATISTICS_AFTER_RHOBF}


@pytest.mark.parametrize("name", sorted(REGRESSIONS))
def test_named_regressions(name):
    modes, ops = REGRESSIONS[name]
    es.replay(ops, modes, 3, _oracle(), _oracle(), what=name)


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
    """``method`` of DeviceLESEnsemble with ``old`` (which occurs exactly once in its source) replaced by ``new``"""
    src = textwrap.dedent(inspect.getsource(getattr(models.DeviceLESEnsemble, method)))
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
}


def plant(monkeypatch, mutant):
    method, old, new = MUTANTS[mutant]
    monkeypatch.setattr(models.DeviceLESEnsemble, method, (lambda self: None) if old is None else _edited(method, old, new))


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_state_mutants_fail_a_committed_sequence(monkeypatch, mutant):
    """each fault of the ensemble's caches, patched into DeviceLESEnsemble, fails the sequences the table names (all of them
    among those of test_every_mode_combination, those of the mutants 9 and up among those of test_every_new_mode_combination,
    two and more each); the same sequences pass without it"""
    assert all(seed in SEEDS and modes in (COMBINATIONS if mutant <= 8 else NEW_COMBINATIONS) for seed, modes in CAUGHT_BY[mutant])
    assert len(set(CAUGHT_BY[mutant])) == len(CAUGHT_BY[mutant]) >= (1 if mutant <= 8 else 2)
    for seed, modes in CAUGHT_BY[mutant]:
        es.run(_oracle(), _oracle(), seed, modes, 3)
    plant(monkeypatch, mutant)
    for seed, modes in CAUGHT_BY[mutant]:
        with pytest.raises(AssertionError, match="operation"):
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
