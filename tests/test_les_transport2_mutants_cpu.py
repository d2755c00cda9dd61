"""The K23 table of tools/mutation_control.py (--transport2) without a GPU: every edit still applies to the tree, every guard
names a body of tests/les_transport2_ref.py, and the mutant libraries' names collide with no other table's."""
import os

from tests import les_transport2_ref as lt2
from tools import mutation_control as mc


def test_transport2_mutants_apply_to_the_tree_and_name_their_guards():
    table = mc.TRANSPORT2_MUTANTS
    assert sorted(table) == list(range(1, 9))
    for n, (what, guard, edits) in table.items():
        assert what and edits and callable(guard) and all(e[0] == mc.TRANSPORT2 for e in edits), n
        mod, name = guard.__name__.split(".", 1)
        assert mod == "les_transport2_ref" and name in lt2.BODIES and hasattr(lt2, "check_" + name), (n, guard.__name__)
        files = mc.patched(n, table=table)
        for fname, text in files.items():
            with open(os.path.join(mc.CSRC, fname)) as f:
                assert text != f.read(), (n, fname)


def test_library_names_do_not_collide():
    tables = (mc.MUTANTS, mc.ADVANCE_MUTANTS, mc.THERMO_MUTANTS, mc.WATERPATH_MUTANTS, mc.MICRO_MUTANTS, mc.DIFFUSE_MUTANTS, mc.ADVECT_MUTANTS,
              mc.VADVECT_MUTANTS, mc.RADIATE_MUTANTS, mc.QTLOCAL_MUTANTS, mc.MOMENTS_MUTANTS, mc.BUOYANCY_MUTANTS, mc.TRANSPORT_MUTANTS,
              mc.TRANSPORT2_MUTANTS, mc.GEO_MUTANTS, mc.LESSTATE_MUTANTS, mc.VNUDGE_MUTANTS)
    libs = [mc.lib_of(n, t) for t in tables for n in t]
    assert len(set(libs)) == len(libs) and mc.lib_of(2, mc.TRANSPORT2_MUTANTS).endswith("libspc_transport2_mutant2.so")
    assert mc.lib_of(2, mc.TRANSPORT_MUTANTS).endswith("libspc_transport_mutant2.so")


def test_every_body_is_run_by_the_control():
    """check_everything runs each name of BODIES (a body left out would guard nothing)"""
    import inspect
    src = inspect.getsource(lt2.check_everything)
    assert all('("%s",' % name in src for name in lt2.BODIES)
