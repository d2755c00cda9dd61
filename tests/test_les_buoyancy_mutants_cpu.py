"""The K21 table of tools/mutation_control.py (--buoyancy) without a GPU: every edit's pattern occurs exactly once in the kernel
text and changes it, every guard names a body of tests/les_buoyancy_ref.py, and the mutant libraries' names collide with no
other table's."""
import os

from tests import les_buoyancy_ref as lbr
from tests.les_harness import check_jobs_are_bodies, check_library_names
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
    check_library_names(mc.BUOYANCY_MUTANTS, "libspc_buoyancy_mutant2.so")


def test_every_body_is_run_by_the_control():
    check_jobs_are_bodies(lbr)
