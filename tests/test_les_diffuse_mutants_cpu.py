"""The K15 table of tools/mutation_control.py (--diffuse) without a GPU: every edit still applies to the tree, every guard
names a body of tests/les_diffuse_ref.py, and the mutant libraries' names collide with no other table's."""
from tests import les_diffuse_ref as ldr
from tests.les_harness import check_jobs_are_bodies, check_library_names, check_mutant_table
from tools import mutation_control as mc


def test_diffuse_mutants_apply_to_the_tree_and_name_their_guards():
    check_mutant_table(mc.DIFFUSE_MUTANTS, (mc.DIFFUSE,), ldr)


def test_library_names_do_not_collide():
    check_library_names(mc.DIFFUSE_MUTANTS, "libspc_diffuse_mutant2.so")


def test_every_body_is_run_by_the_control():
    check_jobs_are_bodies(ldr)
