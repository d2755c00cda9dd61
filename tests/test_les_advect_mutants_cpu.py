"""The K16 table of tools/mutation_control.py (--advect) without a GPU: every edit still applies to the tree, every guard
names a body of tests/les_advect_ref.py, and the mutant libraries' names collide with no other table's."""
from tests import les_advect_ref as lar
from tests.les_harness import check_jobs_are_bodies, check_library_names, check_mutant_table
from tools import mutation_control as mc


def test_advect_mutants_apply_to_the_tree_and_name_their_guards():
    check_mutant_table(mc.ADVECT_MUTANTS, (mc.ADVECT,), lar)


def test_library_names_do_not_collide():
    check_library_names(mc.ADVECT_MUTANTS, "libspc_advect_mutant2.so")
    assert mc.lib_of(2, mc.ADVANCE_MUTANTS).endswith("libspc_advance_mutant2.so")


def test_every_body_is_run_by_the_control():
    check_jobs_are_bodies(lar)
