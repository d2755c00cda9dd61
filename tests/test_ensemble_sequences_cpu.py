"""Random operation sequences of models.DeviceLESEnsemble on oracle-backed engines against its NumPy twin, without a GPU
(the body: tests/ensemble_sequences.py): all 48 valid mode combinations with two seeds, row blocks 1 + 1 + 0 of a
MultiDeviceEngine, the fused K11 step in front of every later stage, the named regression sequences of what the sequences
found, and the state mutants: faults of the ensemble's caches, patched in, that a committed sequence has to notice.

Which committed sequence (seed, modes; n = 3 on one engine) notices which state mutant:
  1  _drop_water_paths does nothing                              seed 1 plain, seed 1 thermo
  2  set_fields_batched does not set _thermo_stale               seed 1 thermo+diffuse, seed 2 thermo+advect
  3  set_fields_batched does not clear _means                    seed 2 diffuse, seed 1 micro
  4  _diffuse's profile cache ignores dt                         seed 1 diffuse, seed 2 diffuse
  5  _microphysics' profile cache ignores presf                  seed 1 thermo+micro, seed 1 micro+advect+vertical
  6  _microphysics does not swap f["QR"] and _qr_spare           seed 1 micro, seed 2 thermo+micro
  7  get_water_paths_batched ignores a changed weight profile    seed 1 plain, seed 2 thermo
  8  the nudge's tail (the same tensor set again) keeps _means   seed 1 thermo+diffuse, seed 2 thermo+advect
(test_state_mutants_fail_a_committed_sequence asserts every line of this table.)"""
import inspect
import re
import textwrap

import numpy
import pytest

from sp_coupler_amd import device_les, models, spcpl
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import ensemble_sequences as es
from tests import les_micro_ref as lmr
from tests import les_radiate_ref as lrr
from tests import les_thermo_ref as ltr
from tests import slab_ref

SEEDS = (1, 2)
COMBINATIONS = es.combinations()
SIX = [(), ("thermo", "micro"), ("diffuse", "advect", "vertical"), ("micro", "radiate"), ("thermo", "diffuse", "advect", "radiate"), es.MODES]


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def _oracle():
    return lrr.RadiateOracleEngine()


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
REGRESSIONS = {"unobserved first step": UNOBSERVED_FIRST_STEP, "row after nudge": ROW_AFTER_NUDGE, "row after set_fields": ROW_AFTER_SET_FIELDS,
               "row water path after Rhobf": ROW_WATER_PATH_AFTER_RHOBF, "late microphysics after presf": LATE_MICRO_AFTER_PRESF}


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
}
CAUGHT_BY = {
    1: [(1, ()), (1, ("thermo",))],
    2: [(1, ("thermo", "diffuse")), (2, ("thermo", "advect"))],
    3: [(2, ("diffuse",)), (1, ("micro",))],
    4: [(1, ("diffuse",)), (2, ("diffuse",))],
    5: [(1, ("thermo", "micro")), (1, ("micro", "advect", "vertical"))],
    6: [(1, ("micro",)), (2, ("thermo", "micro"))],
    7: [(1, ()), (2, ("thermo",))],
    8: [(1, ("thermo", "diffuse")), (2, ("thermo", "advect"))],
}


def plant(monkeypatch, mutant):
    method, old, new = MUTANTS[mutant]
    monkeypatch.setattr(models.DeviceLESEnsemble, method, (lambda self: None) if old is None else _edited(method, old, new))


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_state_mutants_fail_a_committed_sequence(monkeypatch, mutant):
    """each fault of the ensemble's caches, patched into DeviceLESEnsemble, fails the sequences the table names (all of them
    among those of test_every_mode_combination); the same sequences pass without it"""
    assert all(seed in SEEDS and modes in COMBINATIONS for seed, modes in CAUGHT_BY[mutant]) and len(CAUGHT_BY[mutant]) >= 1
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
