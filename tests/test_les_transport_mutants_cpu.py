"""The K22 table of tools/mutation_control.py (--transport) without a GPU: every edit still applies to the tree, every guard
names a body of tests/les_transport_ref.py, and the mutant libraries' names collide with no other table's."""
from tests import les_transport_ref as ltr
from tests.les_harness import check_jobs_are_bodies, check_library_names, check_mutant_table
from tools import mutation_control as mc


def test_transport_mutants_apply_to_the_tree_and_name_their_guards():
    table = mc.TRANSPORT_MUTANTS
    check_mutant_table(table, (mc.TRANSPORT, mc.VADVECT), ltr)
    assert sum(all(e[0] == mc.TRANSPORT for e in edits) for _, _, edits in table.values()) == 7      # (mutant 5: K17's chain, which K22 runs)


def test_library_names_do_not_collide():
    check_library_names(mc.TRANSPORT_MUTANTS, "libspc_transport_mutant2.so")


def test_every_body_is_run_by_the_control():
    check_jobs_are_bodies(ltr)
