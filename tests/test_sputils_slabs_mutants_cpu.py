"""The K7 table of tools/mutation_control.py (--sputils) without a GPU: every edit applies to the kernel text exactly as often as it
states and changes it, every guard names a body of tests/sputils_slabs.py, and the mutant libraries' names collide with no other
table's."""
from tests import sputils_slabs as ss
from tests.les_harness import check_jobs_are_bodies, check_library_names, check_mutant_table
from tools import mutation_control as mc


def test_sputils_mutants_apply_to_the_tree_and_name_their_guards():
    assert len(mc.SPUTILS_MUTANTS) >= 10
    check_mutant_table(mc.SPUTILS_MUTANTS, (mc.SU, mc.SU_HOST), ss, count=len(mc.SPUTILS_MUTANTS))


def test_edits_leave_extents_barriers_and_launches_alone():
    """no edit touches a slab's extent (nrow, cnt), a barrier, a launch or the indices of a workgroup: the mutants stay inside
    what the shipped kernels touch (the table says why, per mutant)"""
    for n, (_, _, edits) in mc.SPUTILS_MUTANTS.items():
        for edit in edits:
            for word in ("__syncthreads", "hipLaunchKernelGGL", "blockIdx", "const int nrow", "const int cnt", "spc_smem"):
                assert word not in edit[1] and word not in edit[2], (n, word)


def test_library_names_do_not_collide():
    check_library_names(mc.SPUTILS_MUTANTS, "libspc_sputils_mutant2.so")
    rows = [t for t in mc.ALL_TABLES if t.table is mc.SPUTILS_MUTANTS]
    assert rows == list(mc.SPUTILS_TABLES) and (rows[0].flag, rows[0].kernel, rows[0].module, rows[0].gpu_test) == ("sputils", "K7", "sputils_slabs", "test_sputils_slabs_gpu")
    tags = [mc._tag(t.table) for t in mc.ALL_TABLES]
    assert len(set(tags)) == len(tags) and len({t.flag for t in mc.ALL_TABLES}) == len(mc.ALL_TABLES)
    import importlib
    for e in mc.SPUTILS_TABLES:                                  # what tests/test_les_mix_mutants_cpu.py asks of the rows of LATER_TABLES
        module = importlib.import_module("tests." + e.module)
        importlib.import_module("tests." + e.gpu_test)
        for n, (what, guard, edits) in e.table.items():
            mod, name = guard.__name__.split(".", 1)
            assert mod == e.module and name in module.BODIES and callable(getattr(module, "check_" + name)), (e.flag, n)


def test_every_body_is_run_by_the_control():
    check_jobs_are_bodies(ss)
    guards = {guard.__name__.split(".", 1)[1] for _, guard, _ in mc.SPUTILS_MUTANTS.values()}
    assert guards == set(ss.BODIES) - {"plain_stores"}           # (plain stores: the same kernels with another store instruction)
