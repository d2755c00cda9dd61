"""Random operation sequences of models.DeviceLESEnsemble on the MI355X against its NumPy twin (the body:
tests/ensemble_sequences.py; the conditions, the properties (a) and (b) and the list of state mutants are in its docstring and
in tests/test_ensemble_sequences_cpu.py).  The device ensemble runs on Engine("cuda:0") in float64 at n = 3, 4 x 5 x 20; the
twin computes in NumPy on the host (its variability nudge alone goes through an engine).  Everything is bit-equality
(gpu_util.assert_bits), W alone keeps the bound of les_vadvect_ref.check_w: there is no tolerance to choose and nothing is
measured.  Every case runs two seeds; nothing but the ensemble is mutated."""
import numpy
import pytest
import torch

from sp_coupler_amd import models, spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import ensemble_sequences as es

pytestmark = pytest.mark.gpu

SEEDS = (1, 3)                                                    # (over these every kind of operation occurs in the twelve cases: asserted)
#: all six modes, each mode alone (the vertical advection with the horizontal it needs), the pairs and triples that share a
#: cache (K12's temperature for K14, the spare buffers of K16 / K17 in front of K15, QL for K18 and K14), and two mixes
TWELVE = [es.MODES, ("thermo",), ("diffuse",), ("micro",), ("advect",), ("advect", "vertical"), ("radiate",), ("thermo", "micro"),
          ("diffuse", "advect", "vertical"), ("micro", "radiate"), ("thermo", "diffuse", "advect", "radiate"), ("thermo", "micro", "advect", "vertical")]
FOUR = [es.MODES, ("thermo", "micro"), ("diffuse", "advect", "vertical"), ("micro", "radiate")]


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
