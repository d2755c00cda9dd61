"""The mutation control's table (tools/mutation_control.py) against the current kernel sources, on the CPU: the shipped
sources carry no mutant switch, every mutant is present and guarded by a property of tests/semantic_props.py (K10's by a
body of tests/slab_edges.py, K8's by one of tests/geo_edges.py, K9's by one of tests/les_state_ref.py, K6's own table by
one of tests/vnudge_edges.py), and every
edit still finds its line -- a kernel edit that drops or moves a mutant's line fails here, not as a SURVIVED mutant on the
GPU box."""
import os
import re

import pytest

from tests import semantic_props as sp
from tools import mutation_control as mc


def test_no_mutant_switch_in_the_shipped_sources(repo_root):
    hits = []
    for d in (mc.CSRC, os.path.join(repo_root, "include")):
        for name in sorted(os.listdir(d)):
            with open(os.path.join(d, name)) as f:
                hits += ["%s:%d" % (name, i + 1) for i, line in enumerate(f) if re.search(r"\bSPC_MUT", line)]
    assert not hits, hits


def test_every_mutant_is_guarded_by_a_property():
    assert sorted(mc.MUTANTS) == list(range(1, 36))
    names = {p.__name__[5:] for p in sp.PROPERTIES}
    from tests import slab_edges
    for n, (what, guard, edits) in mc.MUTANTS.items():
        assert what and edits, n
        if n < 28:
            assert guard in names, (n, guard)
        else:                                        # K10: a body of tests/slab_edges.py, run on the engines of the mutant library
            assert callable(guard) and all(e[0] == mc.SLAB for e in edits), n
            assert hasattr(slab_edges, "check_" + guard.__name__.split(".", 1)[1]), (n, guard.__name__)


@pytest.mark.parametrize("n", sorted(mc.MUTANTS))
def test_mutant_edits_apply_to_the_tree(n):
    files = mc.patched(n)        # raises when an edit's old text does not occur the expected number of times
    for name, text in files.items():
        with open(os.path.join(mc.CSRC, name)) as f:
            assert text != f.read(), (n, name)


NEW_TABLES = [(mc.GEO_MUTANTS, mc.GEO, "geo_edges", 15), (mc.LESSTATE_MUTANTS, mc.LESSTATE, "les_state_ref", 13)]


@pytest.mark.parametrize("table,source,module,count", NEW_TABLES, ids=["geo", "lesstate"])
def test_k8_k9_mutants_are_guarded_by_a_body(table, source, module, count):
    import importlib
    bodies = importlib.import_module("tests." + module)
    assert sorted(table) == list(range(1, count + 1))
    for n, (what, guard, edits) in table.items():
        assert what and edits and callable(guard) and all(e[0] in (source, source.replace(".hpp", "_host.hpp")) for e in edits), n
        mod, name = guard.__name__.split(".", 1)
        assert mod == module and hasattr(bodies, "check_" + name) and name in bodies.OLD_BODIES + bodies.NEW_BODIES, (n, guard.__name__)
    assert set(mc.GEO_OLD_GUARDS) <= set(mc.GEO_MUTANTS) and set(mc.LESSTATE_OLD_GUARDS) <= set(mc.LESSTATE_MUTANTS)


@pytest.mark.parametrize("table,n", [(t, n) for t in (mc.GEO_MUTANTS, mc.GEO_EQUIVALENT, mc.LESSTATE_MUTANTS, mc.LESSTATE_EQUIVALENT)
                                     for n in sorted(t)],
                         ids=lambda v: str(v) if not isinstance(v, dict) else
                         {id(mc.GEO_MUTANTS): "geo", id(mc.GEO_EQUIVALENT): "geo_eq", id(mc.LESSTATE_MUTANTS): "lesstate",
                          id(mc.LESSTATE_EQUIVALENT): "lesstate_eq"}[id(v)])
def test_k8_k9_mutant_edits_apply_to_the_tree(table, n):
    files = mc.patched(n, table=table)      # raises when an edit's old text does not occur exactly as often as stated
    for name, text in files.items():
        with open(os.path.join(mc.CSRC, name)) as f:
            assert text != f.read(), (n, name)


def test_k6_mutants_are_guarded_by_a_body():
    from tests import vnudge_edges
    assert sorted(mc.VNUDGE_MUTANTS) == list(range(1, len(mc.VNUDGE_MUTANTS) + 1)) and len(mc.VNUDGE_MUTANTS) >= 10
    guards = set()
    for n, (what, guard, edits) in mc.VNUDGE_MUTANTS.items():
        assert what and edits and callable(guard) and all(e[0] in (mc.VN, mc.VN2, mc.VN_HOST) for e in edits), n
        mod, name = guard.__name__.split(".", 1)
        assert mod == "vnudge_edges" and name in vnudge_edges.BODIES and callable(getattr(vnudge_edges, "check_" + name)), (n, guard.__name__)
        guards.add(name)
    assert guards == set(vnudge_edges.BODIES)                 # no body without a mutant written for it
    assert mc.VNUDGE_MIN_SURVIVORS >= 6


@pytest.mark.parametrize("n", sorted(mc.VNUDGE_MUTANTS))
def test_k6_mutant_edits_apply_to_the_tree(n):
    files = mc.patched(n, table=mc.VNUDGE_MUTANTS)      # raises when an edit's old text does not occur exactly as often as stated
    for name, text in files.items():
        with open(os.path.join(mc.CSRC, name)) as f:
            assert text != f.read(), (n, name)


def test_k7_mutants_are_guarded_by_a_slab_body():
    from tests import sputils_slabs
    assert sorted(mc.SPUTILS_MUTANTS) == list(range(1, len(mc.SPUTILS_MUTANTS) + 1)) and len(mc.SPUTILS_MUTANTS) >= 10
    for n, (what, guard, edits) in mc.SPUTILS_MUTANTS.items():
        assert what and edits and callable(guard) and all(e[0] in (mc.SU, mc.SU_HOST) for e in edits), n
        mod, name = guard.__name__.split(".", 1)
        assert mod == "sputils_slabs" and name in sputils_slabs.BODIES and callable(getattr(sputils_slabs, "check_" + name)), (n, guard.__name__)


@pytest.mark.parametrize("n", sorted(mc.SPUTILS_MUTANTS))
def test_k7_mutant_edits_apply_to_the_tree(n):
    files = mc.patched(n, table=mc.SPUTILS_MUTANTS)      # raises when an edit's old text does not occur exactly as often as stated
    for name, text in files.items():
        with open(os.path.join(mc.CSRC, name)) as f:
            assert text != f.read(), (n, name)


def test_libraries_of_the_tables_do_not_collide():
    libs = [mc.lib_of(n, t) for t in (mc.MUTANTS, mc.ADVANCE_MUTANTS, mc.THERMO_MUTANTS, mc.GEO_MUTANTS, mc.GEO_EQUIVALENT,
                                      mc.LESSTATE_MUTANTS, mc.LESSTATE_EQUIVALENT, mc.VNUDGE_MUTANTS) for n in t]
    assert len(set(libs)) == len(libs)
    assert mc.lib_of(9, mc.VNUDGE_MUTANTS).endswith("libspc_vnudge_mutant9.so")
    assert mc.lib_of(3).endswith("libspc_mutant3.so") and mc.lib_of(2, mc.ADVANCE_MUTANTS).endswith("libspc_advance_mutant2.so")
    assert mc.lib_of(4, mc.THERMO_MUTANTS).endswith("libspc_thermo_mutant4.so")
