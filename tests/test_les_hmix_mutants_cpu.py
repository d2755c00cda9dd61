"""The K26 table of tools/mutation_control.py (--hmix) without a GPU: every edit applies to the kernel text exactly as often as it
states and changes it, every guard names a body of tests/les_hmix_ref.py, and the mutant libraries' names collide with no other
table's."""
from tests import les_hmix_ref as lhr
from tests.les_harness import check_jobs_are_bodies, check_library_names, check_mutant_table
from tools import mutation_control as mc


def test_hmix_mutants_apply_to_the_tree_and_name_their_guards():
    check_mutant_table(mc.HMIX_MUTANTS, (mc.HMIX,), lhr)


def test_edits_change_values_only():
    """no edit touches a loop, a barrier, a launch or the indices of a workgroup"""
    for n, (_, _, edits) in mc.HMIX_MUTANTS.items():
        for edit in edits:
            for word in ("for (", "__syncthreads", "hipLaunchKernelGGL", "blockIdx", "threadIdx"):
                assert word not in edit[1] and word not in edit[2], (n, word)


def test_library_names_do_not_collide():
    check_library_names(mc.HMIX_MUTANTS, "libspc_hmix_mutant2.so")
    rows = [t for t in mc.ALL_TABLES if t.table is mc.HMIX_MUTANTS]
    assert rows == [mc.ALL_TABLES[-1]] == list(mc.HMIX_TABLES)
    assert (rows[0].flag, rows[0].kernel, rows[0].module, rows[0].gpu_test) == ("hmix", "K26", "les_hmix_ref", "test_les_hmix_gpu")
    assert mc.LATER_TABLES[-1].kernel == "K25"
    tags = [mc._tag(t.table) for t in mc.ALL_TABLES]
    assert len(set(tags)) == len(tags) and len({t.flag for t in mc.ALL_TABLES}) == len(mc.ALL_TABLES)


def test_every_body_is_run_by_the_control():
    check_jobs_are_bodies(lhr)
    assert sorted({guard.__name__.split(".", 1)[1] for _, guard, _ in mc.HMIX_MUTANTS.values()}) == ["lines", "parity", "viscosity"]
