"""K9 on the MI355X: spcpl.set_les_state_batched / Engine.les_state against the unchanged host spcpl.set_les_state, run on
recording LES after re-seeding.  Every test asks for equal bits and an equal numpy.random.get_state() tuple.  The helpers
and the bodies that tools/mutation_control.py --lesstate also runs on its mutant libraries live in tests/les_state_ref.py."""
import copy

import numpy
import pytest
import torch

from sp_coupler_amd import driver, models, spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_state_ref
from tests.les_state_ref import RecLES, _odd_start, _profiles, _run_both, _same_state

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def test_mixed_shapes_odd_start_cached_gauss():
    les_state_ref.check_mixed_shapes(Engine("cuda:0"))


@pytest.mark.parametrize("gens", les_state_ref.FORCED_GENS)
def test_forced_short_substreams(gens):
    """many substream boundaries, doubles whose two words straddle them, the prefix from an odd pos"""
    les_state_ref.check_forced_short_substreams(Engine("cuda:0"), (gens,))


def test_start_at_twist_boundary_and_no_twist():
    les_state_ref.check_twist_boundary(Engine("cuda:0"))


def test_engine_les_state_equals_host_jump():
    """Engine.les_state on one shape: [n x itot x jtot x ktot] fields and the state NumPy (and the host jump) reach"""
    les_state_ref.check_engine_level(Engine("cuda:0"))


def test_an_les_begins_on_the_first_element_of_a_substream():
    """an LES of one cell, of several cells and the last LES of the list on the first element a substream emits, from an even
    and from an odd pos, with 1 and 2 generations per substream"""
    les_state_ref.check_seek_boundaries(Engine("cuda:0"))


def test_substream_counts_that_are_no_power_of_two():
    """3, 5 and 7 substreams, the last one whole and one generation short, launches that end at pos 624"""
    les_state_ref.check_odd_substream_counts(Engine("cuda:0"))


def test_small_chunks_and_engines_sharing_a_card(monkeypatch):
    shapes = [(7, 5, 19), (16, 16, 40), (5, 3, 11), (16, 16, 40), (7, 5, 19), (9, 9, 33), (2, 2, 2)]
    monkeypatch.setattr(spcpl, "_les_state_budget", lambda eng: 4 * 8 * (16 * 16 * 40 + 40))     # about one LES per launch
    spcpl.set_engine(Engine("cuda:0"))
    _run_both(shapes, _odd_start(17))
    spcpl.set_engine(MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")),
                                        Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")),
                                        Engine("cuda:0")], min_cols_per_device=1))
    _run_both(shapes, _odd_start(18))
    monkeypatch.undo()
    _run_both(shapes, _odd_start(19), gens_per_substream=2)


def _reference_init(gcm, les_models, start):
    numpy.random.set_state(start)
    spcpl.gather_gcm_data(gcm, les_models, True)
    for les in les_models:
        u, v, thl, qt, ps, ql = spcpl.convert_profiles(les)
        spcpl.set_les_state(les, u, v, thl, qt, ps)
    return numpy.random.get_state()


class RecSyntheticLES(models.SyntheticLES):
    def set_field(self, name, values):
        self.__dict__.setdefault("calls", []).append((name, numpy.array(getattr(values, "number", values))))
        super().set_field(name, values)

    def set_surface_pressure(self, ps):
        self.__dict__.setdefault("calls", []).append(("PS", float(ps)))
        super().set_surface_pressure(ps)


def _rec_models(n, seed=1):
    gcm, les_models = models.make_models(n, nL=160, seed=seed)
    rec = []
    for les in les_models:
        r = RecSyntheticLES.__new__(RecSyntheticLES)
        r.__dict__.update(copy.deepcopy(les.__dict__))
        rec.append(r)
    return gcm, rec


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_profiles_from_the_forward_launch(dtype):
    """no profiles given: u, v, thl, qt, ps from convert_profiles' forward launch, on float64 and float32 engines"""
    spcpl.set_engine(Engine("cuda:0", dtype=dtype))
    start = _odd_start(23)
    gcm, want = _rec_models(6)
    s_want = _reference_init(gcm, want, start)
    gcm2, got = _rec_models(6)
    numpy.random.set_state(start)
    spcpl.gather_gcm_data(gcm2, got, True)
    spcpl.set_les_state_batched(got)
    _same_state(numpy.random.get_state(), s_want)
    for g, w in zip(got, want):
        assert [c[0] for c in g.calls] == [c[0] for c in w.calls] == ["U", "V", "THL", "QT", "PS"]
        for (_, x), (_, y) in zip(g.calls, w.calls):
            assert numpy.array_equal(x, y)
        assert numpy.array_equal(numpy.asarray(g.gcm_Zf), numpy.asarray(w.gcm_Zf))


def test_ensemble_path():
    spcpl.set_engine(Engine("cuda:0"))
    start = _odd_start(29)
    gcm = models.SyntheticGCM(12, 91, 1)
    want = models.SyntheticLESEnsemble.for_gcm(gcm, [1, 3, 4, 7, 9], nL=160, seed=2)
    s_want = _reference_init(gcm, list(want), start)          # per-row faces: set_field / set_surface_pressure of _LESRow
    gcm2 = models.SyntheticGCM(12, 91, 1)
    got = models.SyntheticLESEnsemble.for_gcm(gcm2, [1, 3, 4, 7, 9], nL=160, seed=2)
    numpy.random.set_state(start)
    spcpl.gather_gcm_data(gcm2, got, True)
    assert got.fields3d is None
    spcpl.set_les_state_batched(got)
    _same_state(numpy.random.get_state(), s_want)
    for name in ("U", "V", "THL", "QT"):
        assert got.fields3d[name].shape == (5, 8, 8, 160)
        assert numpy.array_equal(got.fields3d[name], want.fields3d[name]), name
    assert numpy.array_equal(got.p["PS"], want.p["PS"])


def test_ktot_mismatch_raises_before_drawing():
    spcpl.set_engine(Engine("cuda:0"))
    start = _odd_start(31)
    u, v, thl, qt = _profiles([(4, 4, 10), (4, 4, 12)])
    les = [RecLES((4, 4, 10)), RecLES((4, 4, 11))]
    with pytest.raises(ValueError):
        spcpl.set_les_state_batched(les, u, v, thl, qt)
    _same_state(numpy.random.get_state(), start)
    assert not les[0].calls and not les[1].calls


def _restated_splib_init(gcm, les_models, seed, spinup, steps):
    """splib.initialize (splib/splib.py:180-206) and run_spinup (233-250) restated on the per-LES spcpl functions"""
    numpy.random.seed(seed)
    gcm.evolve_model_until_cloud_scheme()
    gcm.evolve_model_cloud_scheme()
    gcm.first_half_step_done = True
    spcpl.gather_gcm_data(gcm, les_models, True)
    for les in les_models:
        u, v, thl, qt, ps, ql = spcpl.convert_profiles(les)
        spcpl.set_les_state(les, u, v, thl, qt, ps)
    cpl = driver.Coupler(gcm, les_models, qt_forcing="sp")
    iteration_length = spinup / steps
    for s in range(steps):
        if s == steps - 1:
            iteration_length = spinup - (steps - 1) * iteration_length
        cpl.step_spinup(spinup_length=iteration_length)
    return cpl


def test_coupler_init_les_state_and_run_spinup():
    spcpl.set_engine(Engine("cuda:0"))
    gcm, want = _rec_models(5, seed=4)
    ref = _restated_splib_init(gcm, want, 42, 1000.0, 3)
    s_want = numpy.random.get_state()
    R_want = numpy.random.normal(size=(8, 8))                # the variability nudge's next draw (spcpl.py:620)
    gcm2, got = _rec_models(5, seed=4)
    cpl = driver.Coupler(gcm2, got, qt_forcing="sp")
    cpl.init_les_state()
    cpl.run_spinup(1000.0, 3)
    _same_state(numpy.random.get_state(), s_want)
    assert numpy.array_equal(numpy.random.normal(size=(8, 8)), R_want)
    for g, w in zip(got, want):
        assert [c[0] for c in g.calls] == [c[0] for c in w.calls]
        for (_, x), (_, y) in zip(g.calls, w.calls):
            assert numpy.array_equal(x, y)
        for k in ("U", "V", "THL", "QT", "PS"):
            assert numpy.array_equal(g.p[k], w.p[k]), k
        assert g.model_time == w.model_time
    assert gcm2.first_half_step_done and cpl.firststep is False and ref.firststep is False


class Tagged:
    """what a unit wrapper hands the models (an AMUSE quantity in the OMUSE set-up): the name it was wrapped under and the
    number"""

    def __init__(self, name, value):
        self.name, self.number = name, numpy.array(value)

    def __bool__(self):
        return bool(self.number)


class WrapRecLES(models.SyntheticLES):
    def set_field(self, name, values):
        self.__dict__.setdefault("calls", []).append((name, type(values).__name__, values.name, numpy.array(values.number)))
        super().set_field(name, values)

    def set_surface_pressure(self, ps):
        self.__dict__.setdefault("calls", []).append(("PS", type(ps).__name__, getattr(ps, "name", None), numpy.array(ps.number)))
        super().set_surface_pressure(ps)


def _wrap_models(n):
    gcm, les_models = models.make_models(n, nL=160, seed=6)
    rec = []
    for les in les_models:
        r = WrapRecLES.__new__(WrapRecLES)
        r.__dict__.update(copy.deepcopy(les.__dict__))
        rec.append(r)
    return gcm, rec


@pytest.fixture
def tagging_wrapper():
    spcpl.set_unit_wrapper(Tagged)
    yield
    spcpl.set_unit_wrapper(None)


def test_unit_wrapper_reaches_the_models_as_in_the_loop(tagging_wrapper):
    """under a unit wrapper every setter, set_surface_pressure included, gets the wrapped object the per-LES path hands it"""
    spcpl.set_engine(Engine("cuda:0"))
    start = _odd_start(37)
    gcm, want = _wrap_models(4)
    s_want = _reference_init(gcm, want, start)
    gcm2, got = _wrap_models(4)
    numpy.random.set_state(start)
    spcpl.gather_gcm_data(gcm2, got, True)
    spcpl.set_les_state_batched(got)
    _same_state(numpy.random.get_state(), s_want)
    for g, w in zip(got, want):
        assert [c[:3] for c in g.calls] == [c[:3] for c in w.calls]
        assert [c[:3] for c in w.calls][-1] == ("PS", "Tagged", "ps")
        for x, y in zip(g.calls, w.calls):
            assert numpy.array_equal(x[3], y[3])


def test_unit_wrapper_ensemble_ps(tagging_wrapper, monkeypatch):
    """the ensemble branch: each row's set_surface_pressure gets the wrapped ps, as the per-row loop gives it"""
    seen = []
    orig = models._LESRow.set_surface_pressure
    monkeypatch.setattr(models._LESRow, "set_surface_pressure",
                        lambda self, ps: (seen.append((self._i, type(ps).__name__, ps.name, float(ps.number))), orig(self, ps)))
    spcpl.set_engine(Engine("cuda:0"))
    start = _odd_start(41)
    gcm = models.SyntheticGCM(10, 91, 1)
    want = models.SyntheticLESEnsemble.for_gcm(gcm, [1, 2, 5], nL=160, seed=3)
    _reference_init(gcm, list(want), start)
    ref, seen[:] = list(seen), []
    gcm2 = models.SyntheticGCM(10, 91, 1)
    got = models.SyntheticLESEnsemble.for_gcm(gcm2, [1, 2, 5], nL=160, seed=3)
    numpy.random.set_state(start)
    spcpl.gather_gcm_data(gcm2, got, True)
    spcpl.set_les_state_batched(got)
    assert seen == ref and len(ref) == 3 and ref[0][1:3] == ("Tagged", "ps")
    for name in ("U", "V", "THL", "QT"):
        assert numpy.array_equal(got.fields3d[name], want.fields3d[name]), name
