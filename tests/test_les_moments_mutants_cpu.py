"""The K20 table of tools/mutation_control.py (--moments) without a GPU: every edit still applies to the tree, every guard
names a body of tests/les_moments_ref.py, and the mutant libraries' names collide with no other table's, K19's included."""
import os

from tests import les_moments_ref as mr
from tools import mutation_control as mc


def test_moments_mutants_apply_to_the_tree_and_name_their_guards():
    table = mc.MOMENTS_MUTANTS
    assert sorted(table) == list(range(1, 9))
    for n, (what, guard, edits) in table.items():
        assert what and edits and callable(guard) and all(e[0] == mc.MOMENTS for e in edits), n
        mod, name = guard.__name__.split(".", 1)
        assert mod == "les_moments_ref" and name in mr.BODIES and hasattr(mr, "check_" + name), (n, guard.__name__)
        files = mc.patched(n, table=table)
        for fname, text in files.items():
            with open(os.path.join(mc.CSRC, fname)) as f:
                assert text != f.read(), (n, fname)


def test_library_names_do_not_collide():
    tables = (mc.MUTANTS, mc.ADVANCE_MUTANTS, mc.THERMO_MUTANTS, mc.WATERPATH_MUTANTS, mc.MICRO_MUTANTS, mc.DIFFUSE_MUTANTS, mc.ADVECT_MUTANTS,
              mc.VADVECT_MUTANTS, mc.RADIATE_MUTANTS, mc.QTLOCAL_MUTANTS, mc.MOMENTS_MUTANTS, mc.GEO_MUTANTS, mc.LESSTATE_MUTANTS,
              mc.VNUDGE_MUTANTS)
    libs = [mc.lib_of(n, t) for t in tables for n in t]
    assert len(set(libs)) == len(libs) and mc.lib_of(2, mc.MOMENTS_MUTANTS).endswith("libspc_moments_mutant2.so")
    assert mc.lib_of(2, mc.MOMENTS_MUTANTS) != mc.lib_of(2, mc.QTLOCAL_MUTANTS)


def test_every_body_is_run_by_the_control():
    """check_everything runs each name of BODIES (a body left out would guard nothing)"""
    import inspect
    src = inspect.getsource(mr.check_everything)
    assert all('("%s",' % name in src for name in mr.BODIES)
