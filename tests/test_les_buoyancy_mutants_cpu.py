"""The K21 table of tools/mutation_control.py (--buoyancy) without a GPU: every edit's pattern occurs exactly once in the kernel
text and changes it, every guard names a body of tests/les_buoyancy_ref.py, and the mutant libraries' names collide with no
other table's."""
import os

from tests import les_buoyancy_ref as lbr
from tools import mutation_control as mc


def test_buoyancy_mutants_apply_to_the_tree_and_name_their_guards():
    table = mc.BUOYANCY_MUTANTS
    assert sorted(table) == list(range(1, 9))
    with open(os.path.join(mc.CSRC, mc.BUOYANCY)) as f:
        shipped = f.read()
    for n, (what, guard, edits) in table.items():
        assert what and edits and callable(guard) and all(e[0] == mc.BUOYANCY and len(e) == 3 for e in edits), n
        assert all(shipped.count(e[1]) == 1 and e[1] != e[2] for e in edits), n
        mod, name = guard.__name__.split(".", 1)
        assert mod == "les_buoyancy_ref" and name in lbr.BODIES and hasattr(lbr, "check_" + name), (n, guard.__name__)
        files = mc.patched(n, table=table)
        assert list(files) == [mc.BUOYANCY] and files[mc.BUOYANCY] != shipped, n


def test_edits_change_values_only():
    """no edit touches an index expression in brackets other than the profile reads it replaces, a loop, a barrier or a launch"""
    for n, (_, _, edits) in mc.BUOYANCY_MUTANTS.items():
        for _, old, new in edits:
            for word in ("for (", "__syncthreads", "hipLaunchKernelGGL", "blockIdx", "threadIdx"):
                assert word not in old and word not in new, (n, word)


def test_library_names_do_not_collide():
    tables = (mc.MUTANTS, mc.ADVANCE_MUTANTS, mc.THERMO_MUTANTS, mc.WATERPATH_MUTANTS, mc.MICRO_MUTANTS, mc.DIFFUSE_MUTANTS, mc.ADVECT_MUTANTS,
              mc.VADVECT_MUTANTS, mc.RADIATE_MUTANTS, mc.QTLOCAL_MUTANTS, mc.MOMENTS_MUTANTS, mc.BUOYANCY_MUTANTS, mc.GEO_MUTANTS, mc.LESSTATE_MUTANTS)
    libs = [mc.lib_of(n, t) for t in tables for n in t]
    assert len(set(libs)) == len(libs) and mc.lib_of(2, mc.BUOYANCY_MUTANTS).endswith("libspc_buoyancy_mutant2.so")


def test_every_body_is_run_by_the_control():
    """check_everything runs each name of BODIES (a body left out would guard nothing)"""
    import inspect
    src = inspect.getsource(lbr.check_everything)
    assert all('("%s",' % name in src for name in lbr.BODIES)
