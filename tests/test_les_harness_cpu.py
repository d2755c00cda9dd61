"""tests/les_harness.py itself, without a GPU: the poisoned buffers see one write in front of an array, behind it and between
its rows; the loop over the bodies collects assertions only and refuses a job list that is not the module's BODIES; the
argument struct is filled in the stated order; and the registry of tools/mutation_control.py names what exists."""
import ctypes
import importlib
import types

import numpy
import pytest
import torch

from tests import les_harness as lh
from tools import mutation_control as mc

ENG = types.SimpleNamespace(device=torch.device("cpu"), dtype=torch.float64)
NAN = float("nan")


def _poisoned(poison):
    mem = lh.Poisoned(ENG)
    a = numpy.arange(6.0).reshape(2, 3)
    plain = mem.put("plain", a, poison, lead=1)
    pitched = mem.rows("pitched", a, poison, lead=1, pad=2)
    assert plain.shape == pitched.shape == (2, 3) and pitched.stride(0) == 5
    assert lh.Poisoned.read_only(plain, a) and lh.Poisoned.read_only(pitched, a)
    return mem, a, plain, pitched


@pytest.mark.parametrize("poison", [NAN, 1e30])
def test_poisoned_sees_a_write_around_an_array_and_between_its_rows(poison):
    _poisoned(poison)[0].check_around("untouched")
    for tag, where, text in (("plain", lambda buf: buf[0:1], "written around the array"),            # the lead
                             ("plain", lambda buf: buf[1 + 6:1 + 7], "written around the array"),       # the tail
                             ("pitched", lambda buf: buf[-1:], "written around the array"),
                             ("pitched", lambda buf: buf[1 + 3:1 + 4], "written between the rows")):    # the pad behind row 0
        mem = _poisoned(poison)[0]
        where(mem.bufs[tag][1])[...] = 7.0
        with pytest.raises(AssertionError) as e:
            mem.check_around("one write")
        assert e.value.args[0] == ("one write", tag, text)


def test_read_only_compares_bytes():
    mem, a, plain, _ = _poisoned(NAN)
    z = mem.put("zeros", numpy.zeros(4), NAN)
    assert lh.Poisoned.read_only(z, numpy.zeros(4))
    z[2] = -0.0
    assert bool((z == 0).all()) and not lh.Poisoned.read_only(z, numpy.zeros(4))
    plain[1, 2] = NAN
    b = a.copy()
    b[1, 2] = NAN
    assert lh.Poisoned.read_only(plain, b) and not lh.Poisoned.read_only(plain, a)


def test_run_bodies_collects_assertions_by_name_and_nothing_else():
    ran = []

    def job(name, exc=None):
        def run():
            ran.append(name)
            if exc:
                raise exc
        return name, run
    assert lh.run_bodies(("a", "b", "c"), [job("a", AssertionError("x")), job("b"), job("c", AssertionError())]) == ["a", "c"]
    assert ran == ["a", "b", "c"]
    with pytest.raises(ValueError):
        lh.run_bodies(("a", "b"), [job("a"), job("b", ValueError("not an assertion"))])
    del ran[:]
    for jobs in ([job("a")], [job("b"), job("a")], [job("a"), job("b"), job("c")], [job("a"), job("x")]):
        with pytest.raises(AssertionError):
            lh.run_bodies(("a", "b"), jobs)
    assert ran == []                                              # refused before anything ran


def test_fill_args_applies_its_four_steps_in_order():
    class Args(ctypes.Structure):
        _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("z", ctypes.c_void_p), ("n", ctypes.c_int), ("pitch", ctypes.c_int)]
    t = {k: torch.zeros(4) for k in ("x", "y", "z", "spare")}
    a = Args(n=3, pitch=5)
    lh.fill_args(a, t, ("x", "y", "z"))
    assert (a.x, a.y, a.z, a.n, a.pitch) == (t["x"].data_ptr(), t["y"].data_ptr(), t["z"].data_ptr(), 3, 5)
    a = Args(n=3, pitch=5)
    lh.fill_args(a, t, ("x", "y"), alias=(("y", "spare"), ("z", "x")), extents=dict(n=0, y=17), null=("x", "y"))
    assert a.x is None and a.y is None                            # null wins over the member, the alias and the extent
    assert a.z == t["x"].data_ptr() and (a.n, a.pitch) == (0, 5)
    a = Args()
    lh.fill_args(a, {"x": t["x"]}, alias=(("x", "x"),), extents=dict(x=t["y"].data_ptr()))
    assert a.x == t["y"].data_ptr() and a.y is None               # members default to every key; an extent overrides an alias


def test_cols_table_finds_the_first_ktot_the_changes_and_the_end():
    cols_of = lambda k: 64 if k <= 10 else 32 if k <= 25 else 16 if k <= 40 else 0          # noqa: E731
    assert lh.cols_table(cols_of) == ({64: 1, 32: 11, 16: 26}, [11, 26], 41)
    assert lh.cols_table(lambda k: 8 if k < 3 else 0) == ({8: 1}, [], 3)
    with pytest.raises(AssertionError):
        lh.cols_table(lambda k: 64, top=50)


def test_registry_names_what_exists():
    flags = [t.flag for t in mc.TABLES]
    assert flags[0] is None and len(set(flags)) == len(flags) == 17
    tags = [mc._tag(t) for e in mc.TABLES for t in (e.table, e.equivalent) if t is not None]
    assert len(set(tags)) == len(tags) == 19 and len({lib for lib, _ in tags}) == 19 and len({src for _, src in tags}) == 19
    for e in mc.TABLES:
        module = importlib.import_module("tests." + e.module)
        importlib.import_module("tests." + e.gpu_test)
        for n, (what, guard, edits) in e.table.items():
            if callable(guard):
                mod, name = guard.__name__.split(".", 1)
                assert mod == e.module and name in module.BODIES and callable(getattr(module, "check_" + name)), (e.flag, n)
        assert set(e.old_guards or ()) <= set(e.table) and all(what and edits for what, edits in (e.equivalent or {}).values())


@pytest.mark.parametrize("module", ["slab_edges", "geo_edges", "vnudge_edges", "les_state_ref", "les_advance_ref", "les_thermo_ref",
                                    "les_water_paths_ref"])
def test_every_body_is_run_by_the_control(module):
    lh.check_jobs_are_bodies(importlib.import_module("tests." + module))
