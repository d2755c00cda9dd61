"""The K23 table of tools/mutation_control.py (--transport2) without a GPU: every edit still applies to the tree, every guard
names a body of tests/les_transport2_ref.py, and the mutant libraries' names collide with no other table's."""
from tests import les_transport2_ref as lt2
from tests.les_harness import check_jobs_are_bodies, check_library_names, check_mutant_table
from tools import mutation_control as mc


def test_transport2_mutants_apply_to_the_tree_and_name_their_guards():
    check_mutant_table(mc.TRANSPORT2_MUTANTS, (mc.TRANSPORT2,), lt2)


def test_library_names_do_not_collide():
    check_library_names(mc.TRANSPORT2_MUTANTS, "libspc_transport2_mutant2.so")
    assert mc.lib_of(2, mc.TRANSPORT_MUTANTS).endswith("libspc_transport_mutant2.so")


def test_every_body_is_run_by_the_control():
    check_jobs_are_bodies(lt2)
