"""The K19 table of tools/mutation_control.py (--qtlocal) without a GPU: every edit still applies to the tree, every guard
names a body of tests/les_qt_local_ref.py, and the mutant libraries' names collide with no other table's, K18's included."""
from tests import les_qt_local_ref as qlr
from tests.les_harness import check_jobs_are_bodies, check_library_names, check_mutant_table
from tools import mutation_control as mc


def test_qtlocal_mutants_apply_to_the_tree_and_name_their_guards():
    check_mutant_table(mc.QTLOCAL_MUTANTS, (mc.QTLOCAL,), qlr)


def test_library_names_do_not_collide():
    check_library_names(mc.QTLOCAL_MUTANTS, "libspc_qtlocal_mutant2.so")
    assert mc.lib_of(2, mc.QTLOCAL_MUTANTS) != mc.lib_of(2, mc.RADIATE_MUTANTS)


def test_every_body_is_run_by_the_control():
    check_jobs_are_bodies(qlr)
