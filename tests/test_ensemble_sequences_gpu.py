"""Random operation sequences of models.DeviceLESEnsemble on the MI355X against its NumPy twin (the body:
tests/ensemble_sequences.py; the conditions, the properties (a) and (b) and the list of state mutants are in its docstring and
in tests/test_ensemble_sequences_cpu.py).  The device ensemble runs on Engine("cuda:0") in float64 and (the last
section) in float32 at n = 3, 4 x 5 x 20; the twin computes in NumPy on the host in the same dtype (its variability nudge alone goes
through an engine, of that dtype).  Everything is bit-equality
(gpu_util.assert_bits), W alone keeps the bound of les_vadvect_ref.check_w, and the moments that hold W are compared bit for
bit with NumPy's moments of the device's own W: there is no tolerance to choose and nothing is measured.  Every case runs two
seeds; nothing but the ensemble is mutated.  Twelve cases of the six old modes, twelve with the five of K19 to K23 and the
statistics of K20, twelve with the three mixing modes (K24, K25, K24 with vertical=True) and the same twelve with "imix" (K26:
enable_mixing(implicit=True), switched off and on again and its kh_cap changed by the mutation "implicit"); four of each through
two and three engines that share the card and behind the fused step.  4 x 5 x 20 at n = 3 is the smallest shape at which every
cache and launch switch of the ensemble is still reached; K24's row walk, K25's LDS tiles and K26's line lengths and LDS edges
have their edge shapes in tests/test_les_mix_gpu.py, tests/test_les_vmix_gpu.py and tests/test_les_hmix_gpu.py."""
import numpy
import pytest
import torch

from sp_coupler_amd import models, spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import ensemble_sequences as es
from tests import les_hmix_ref as lhr
from tests.les_harness import f32_of

pytestmark = pytest.mark.gpu

SEEDS = (1, 3)                                                    # (over these every kind of operation occurs in the twelve cases: asserted)
#: all six modes, each mode alone (the vertical advection with the horizontal it needs), the pairs and triples that share a
#: cache (K12's temperature for K14, the spare buffers of K16 / K17 in front of K15, QL for K18 and K14), and two mixes
TWELVE = [es.OLD_MODES, ("thermo",), ("diffuse",), ("micro",), ("advect",), ("advect", "vertical"), ("radiate",), ("thermo", "micro"),
          ("diffuse", "advect", "vertical"), ("micro", "radiate"), ("thermo", "diffuse", "advect", "radiate"), ("thermo", "micro", "advect", "vertical")]
FOUR = [es.OLD_MODES, ("thermo", "micro"), ("diffuse", "advect", "vertical"), ("micro", "radiate")]
AV = ("advect", "vertical")
#: each new mode alone over its smallest valid background, the pairs that share state (K19's QT under K22, K21 in front of K23, W
#: and its moments, K19 dropping K20's cache), K12 on both sides of K19, K19 and K21 under the statistics, and everything at once
NEW_TWELVE = [("qt",), AV + ("buoyancy",), AV + ("conservative",), AV + ("conservative", "order2"), ("stats",), AV + ("qt", "conservative"),
              AV + ("buoyancy", "conservative", "order2"), AV + ("stats",), ("qt", "stats"), ("thermo", "qt"), AV + ("qt", "buoyancy", "stats"), es.ELEVEN]
NEW_FOUR = [es.ELEVEN, AV + ("qt", "conservative"), AV + ("buoyancy", "conservative", "order2"), ("qt", "stats")]
TRANSPORT = ("advect", "vertical", "conservative", "order2", "buoyancy")
MOIST = ("thermo", "micro", "radiate", "qt", "stats")
#: K24 alone, with K25, in front of K15 without and with its viscosity (vertical=True); the same behind the split advection (the
#: default spacings are the advection's) and behind the whole transport with K21; K25 with K12 and K18, with every moist mode,
#: with K19 and K20 alone, and with K21 under the statistics
MIX_TWELVE = [("mix",), ("mix", "vmix"), ("diffuse", "mix"), ("diffuse", "mix", "kmix"), AV + ("mix",), AV + ("mix", "vmix"), TRANSPORT + ("mix", "vmix"),
              ("diffuse",) + TRANSPORT + ("mix", "kmix"), ("thermo", "radiate", "mix", "vmix"), MOIST + ("mix", "vmix"), ("qt", "stats", "mix", "vmix"),
              AV + ("buoyancy", "stats", "mix", "vmix")]
MIX_TWELVE = [tuple(m for m in es.MODES if m in c) for c in MIX_TWELVE]
MIX_FOUR = [MIX_TWELVE[i] for i in (1, 3, 6, 9)]
#: K26 in the place of K24's second launch in each of them: alone, with K25, in front of K15 without and with its viscosity, behind
#: the split advection and behind the whole transport with K21, with K12 and K18, with every moist mode, with K19 and K20 and with
#: K21 under the statistics
IMIX_TWELVE = [c + (es.IMIX,) for c in MIX_TWELVE]
IMIX_FOUR = [IMIX_TWELVE[i] for i in (1, 3, 6, 9)]


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def _sharing(engines):
    return MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)


def test_the_cases_are_valid_combinations():
    valid = es.combinations()
    assert len(TWELVE) == len(set(TWELVE)) == 12 and all(c in valid for c in TWELVE + FOUR)
    es.check_kinds([(seed, modes) for modes in TWELVE for seed in SEEDS])
    assert len(NEW_TWELVE) == len(set(NEW_TWELVE)) == 12 and all(es.valid(c) and c == tuple(m for m in es.MODES if m in c) and c not in valid
                                                                  for c in NEW_TWELVE)
    assert all(c in NEW_TWELVE for c in NEW_FOUR) and len(set(NEW_FOUR)) == 4
    es.check_kinds([(seed, modes) for modes in NEW_TWELVE for seed in SEEDS])
    par = [(modes, es.params(seed, modes)) for modes in NEW_TWELVE for seed in SEEDS]
    assert {p["kind"] for modes, p in par if "qt" in modes} == {"local", "strong"}
    assert {p["limiter"] for modes, p in par if "order2" in modes} == {"mc", "none"}
    assert len(MIX_TWELVE) == len(set(MIX_TWELVE)) == 12 and all(es.valid(c) and "mix" in c for c in MIX_TWELVE) and len(set(MIX_FOUR)) == 4
    assert {"vmix" in c for c in MIX_FOUR} == {"kmix" in c for c in MIX_FOUR} == {True, False}
    es.check_kinds([(seed, modes) for modes in MIX_TWELVE for seed in SEEDS])
    par = [es.params(seed, modes) for modes in MIX_TWELVE for seed in SEEDS if "vmix" in modes]
    assert {(p["stability"], p["drag"]) for p in par} == {(s, d) for s in (True, False) for d in (True, False)}
    assert {p["dx"] for p in par} == set(es.MIX_DX)
    assert len(IMIX_TWELVE) == len(set(IMIX_TWELVE)) == 12 and all(es.valid(c) and c == tuple(m for m in es.MODES if m in c) for c in IMIX_TWELVE)
    assert not set(IMIX_TWELVE) & set(MIX_TWELVE) and len(set(IMIX_FOUR)) == 4 and all(c in IMIX_TWELVE for c in IMIX_FOUR)
    assert {"vmix" in c for c in IMIX_FOUR} == {"kmix" in c for c in IMIX_FOUR} == {True, False}
    cases = [(seed, modes) for modes in IMIX_TWELVE for seed in SEEDS]
    es.check_kinds(cases)
    assert {es.params(*c)["kh_cap"] for c in cases} == set(es.KH_CAPS)
    es.implicit_conditions(cases, lhr.HmixOracleEngine())         # (the twin alone, in NumPy: switches both ways, late enables, kh_cap on both sides)


@pytest.mark.parametrize("modes", TWELVE, ids=es.name_of)
def test_sequences_equal_the_twin(modes):
    for seed in SEEDS:
        es.run(Engine("cuda:0"), Engine("cuda:0"), seed, modes, 3)


@pytest.mark.parametrize("modes", FOUR, ids=es.name_of)
def test_two_engines_sharing_the_card(modes):
    """n = 5: Sharded row blocks 3 + 2, each engine on its own stream"""
    for seed in SEEDS:
        es.run(Engine("cuda:0"), _sharing(2), seed, modes, 5)


@pytest.mark.parametrize("modes", FOUR, ids=es.name_of)
def test_three_engines_sharing_the_card_one_without_rows(modes):
    """n = 2: row blocks 1 + 1 + 0"""
    for seed in SEEDS:
        es.run(Engine("cuda:0"), _sharing(3), seed, modes, 2)


@pytest.mark.parametrize("modes", FOUR, ids=es.name_of)
def test_fused_step_then_every_later_stage(monkeypatch, modes):
    """FUSED_MIN_LES patched to 0: K11 steps the fields, whatever is enabled follows"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    for seed in SEEDS:
        assert "les_advance" in es.run(Engine("cuda:0"), Engine("cuda:0"), seed, modes, 3)


@pytest.mark.parametrize("modes", NEW_TWELVE, ids=es.name_of)
def test_sequences_of_the_new_modes_equal_the_twin(modes):
    for seed in SEEDS:
        es.run(Engine("cuda:0"), Engine("cuda:0"), seed, modes, 3)


@pytest.mark.parametrize("modes", NEW_FOUR, ids=es.name_of)
def test_new_modes_on_two_engines_sharing_the_card(modes):
    """n = 5: Sharded row blocks 3 + 2, each engine on its own stream"""
    for seed in SEEDS:
        es.run(Engine("cuda:0"), _sharing(2), seed, modes, 5)


@pytest.mark.parametrize("modes", NEW_FOUR, ids=es.name_of)
def test_new_modes_on_three_engines_sharing_the_card_one_without_rows(modes):
    """n = 2: row blocks 1 + 1 + 0"""
    for seed in SEEDS:
        es.run(Engine("cuda:0"), _sharing(3), seed, modes, 2)


@pytest.mark.parametrize("modes", NEW_FOUR, ids=es.name_of)
def test_new_modes_behind_the_fused_step(monkeypatch, modes):
    """FUSED_MIN_LES patched to 0: K11 steps the fields and K19 reads its cached means"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    for seed in SEEDS:
        assert "les_advance" in es.run(Engine("cuda:0"), Engine("cuda:0"), seed, modes, 3)


@pytest.mark.parametrize("modes", MIX_TWELVE, ids=es.name_of)
def test_sequences_of_the_mixing_modes_equal_the_twin(modes):
    for seed in SEEDS:
        es.run(Engine("cuda:0"), Engine("cuda:0"), seed, modes, 3)


@pytest.mark.parametrize("modes", MIX_FOUR, ids=es.name_of)
def test_mixing_on_two_engines_sharing_the_card(modes):
    """n = 5: Sharded row blocks 3 + 2, each engine on its own stream"""
    for seed in SEEDS:
        es.run(Engine("cuda:0"), _sharing(2), seed, modes, 5)


@pytest.mark.parametrize("modes", MIX_FOUR, ids=es.name_of)
def test_mixing_on_three_engines_sharing_the_card_one_without_rows(modes):
    """n = 2: row blocks 1 + 1 + 0"""
    for seed in SEEDS:
        es.run(Engine("cuda:0"), _sharing(3), seed, modes, 2)


@pytest.mark.parametrize("modes", MIX_FOUR, ids=es.name_of)
def test_mixing_behind_the_fused_step(monkeypatch, modes):
    """FUSED_MIN_LES patched to 0: K11 steps the fields, K24 and K25 follow"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    for seed in SEEDS:
        assert "les_advance" in es.run(Engine("cuda:0"), Engine("cuda:0"), seed, modes, 3)


@pytest.mark.parametrize("modes", IMIX_TWELVE, ids=es.name_of)
def test_sequences_of_the_implicit_mixing_equal_the_twin(modes):
    for seed in SEEDS:
        es.run(Engine("cuda:0"), Engine("cuda:0"), seed, modes, 3)


@pytest.mark.parametrize("modes", IMIX_FOUR, ids=es.name_of)
def test_implicit_mixing_on_two_engines_sharing_the_card(modes):
    """n = 5: Sharded row blocks 3 + 2, each engine on its own stream"""
    for seed in SEEDS:
        es.run(Engine("cuda:0"), _sharing(2), seed, modes, 5)


@pytest.mark.parametrize("modes", IMIX_FOUR, ids=es.name_of)
def test_implicit_mixing_on_three_engines_sharing_the_card_one_without_rows(modes):
    """n = 2: row blocks 1 + 1 + 0"""
    for seed in SEEDS:
        es.run(Engine("cuda:0"), _sharing(3), seed, modes, 2)


@pytest.mark.parametrize("modes", IMIX_FOUR, ids=es.name_of)
def test_implicit_mixing_behind_the_fused_step(monkeypatch, modes):
    """FUSED_MIN_LES patched to 0: K11 steps the fields, K26 and K25 follow"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    for seed in SEEDS:
        assert "les_advance" in es.run(Engine("cuda:0"), Engine("cuda:0"), seed, modes, 3)


# -- float32: Engine("cuda:0", dtype=torch.float32) against the float32 twin --------------------------------------------------------
# The twin takes its dtype from the engine its nudge runs on (ensemble_sequences.build), a float32 engine too, so K6's powf is
# common to both sides; tests/slab_ref.HostFieldLESEnsemble states the rule of T.  Everything stays bit for bit, and every device
# tensor has to be of the twin's dtype (assert_bits(..., dtypes=True)); the bound of W is 4 eps of float32.
def _f32(**kw):
    return Engine("cuda:0", dtype=torch.float32, **kw)


def _sharing32(engines):
    return MultiDeviceEngine([_f32(stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)


F32_TWELVES = TWELVE + NEW_TWELVE + MIX_TWELVE + IMIX_TWELVE
F32_FOURS = FOUR + NEW_FOUR + MIX_FOUR + IMIX_FOUR


def test_the_float32_cases_reach_what_the_float64_cases_reach():
    """the float32 twin alone, in NumPy (ensemble_sequences.dtype_conditions asserts every count of a mode the cases hold): more
    than one substep, a cap that binds and one that does not, both signs of K19's a, implicit steps on both sides of kh_cap, rain
    on the ground, in each of the four families at the seeds of this module"""
    assert len(set(F32_TWELVES)) == 48 and len(set(F32_FOURS)) == 16
    for table in (TWELVE, NEW_TWELVE, MIX_TWELVE, IMIX_TWELVE):
        es.dtype_conditions([(seed, modes) for modes in table for seed in SEEDS], f32_of(lhr.HmixOracleEngine)())


@pytest.mark.parametrize("modes", F32_TWELVES, ids=es.name_of)
def test_float32_sequences_equal_the_float32_twin(modes):
    for seed in SEEDS:
        es.run(_f32(), _f32(), seed, modes, 3)


@pytest.mark.parametrize("modes", F32_FOURS, ids=es.name_of)
def test_float32_on_two_engines_sharing_the_card(modes):
    """n = 5: Sharded row blocks 3 + 2, each engine on its own stream"""
    for seed in SEEDS:
        es.run(_f32(), _sharing32(2), seed, modes, 5)


@pytest.mark.parametrize("modes", F32_FOURS, ids=es.name_of)
def test_float32_behind_the_fused_step(monkeypatch, modes):
    """FUSED_MIN_LES patched to 0: K11 steps the float32 fields, whatever is enabled follows"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    for seed in SEEDS:
        assert "les_advance" in es.run(_f32(), _f32(), seed, modes, 3)


@pytest.mark.parametrize("modes", [es.ELEVEN, MIX_FOUR[3], IMIX_FOUR[2]], ids=es.name_of)
def test_a_float64_and_a_float32_ensemble_step_alternately_in_one_process(modes):
    """two device ensembles alive at once, one on a float64 and one on a float32 engine (each engine has its own workspaces, plan
    caches and LDS limits), take the operations of one sequence in turn, the float64 one first; each is compared with its own
    twin at every observation, bit for bit and dtype for dtype"""
    seed = SEEDS[0]
    modes = tuple(m for m in es.MODES if m in modes)
    ops, par = es.generate(seed, modes), es.params(seed, modes)
    late = es.check_sequence(ops, modes, par=par)
    engines = {numpy.float64: Engine("cuda:0"), numpy.float32: _f32()}
    want = {}
    for T, eng in engines.items():                                 # the twins first, one after the other
        twin, on = es.build(eng, False, 3, modes, late, par), es._on_at_start(modes, late)
        want[T] = [es.apply(twin, op, False, modes, on, par) for op in ops]
    side = {}
    for T, eng in engines.items():
        state = numpy.random.get_state()
        side[T] = [es.build(eng, True, 3, modes, late, par), es._on_at_start(modes, late), state]
    for i, op in enumerate(ops):
        for T, eng in engines.items():
            ens, on, state = side[T]
            spcpl.set_engine(eng)                                  # (what ``build`` sets: the nudge of this ensemble runs on its engine)
            numpy.random.set_state(state)
            got = es.apply(ens, op, True, modes, on, par)
            side[T][2] = numpy.random.get_state()
            assert (got is None) == (want[T][i] is None)
            if got is not None:
                ref = es._of_the_own_w(ens, got, want[T][i], row=op[1] % 3 if op[0] == "row_stats" else None)
                for k in got:
                    try:
                        es._compare(k, got[k], ref[k])
                    except AssertionError as e:
                        raise AssertionError("%s operation %d %r: %s" % (numpy.dtype(T).name, i, op, e)) from e
                for k in ("field U", "field QL", "LWP"):
                    assert k not in got or got[k].dtype == T, (k, got[k].dtype)
    assert side[numpy.float64][0].model_time == side[numpy.float32][0].model_time


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_the_courant_numbers_of_two_engines_at_130_les(dtype):
    """the named regression "courant on own streams" of tests/test_ensemble_sequences_cpu.py where it showed: 130 LES as row blocks
    65 + 65 on two engines that share the card, each on a stream of its own, the Courant numbers read behind every step"""
    from tests import test_ensemble_sequences_cpu as cpu
    modes, ops, par = cpu._regression("courant on own streams")
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=dtype, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    es.replay(ops, modes, 130, Engine("cuda:0", dtype=dtype), multi, what="courant on own streams", par=par)
