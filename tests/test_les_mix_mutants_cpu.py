"""The K24 table of tools/mutation_control.py (--mix) without a GPU: every edit applies to the kernel text exactly as often as it
states and changes it, every guard names a body of tests/les_mix_ref.py, and the mutant libraries' names collide with no other
table's."""
import importlib

from tests import les_mix_ref as lxr
from tests.les_harness import check_jobs_are_bodies, check_library_names, check_mutant_table
from tools import mutation_control as mc


def test_mix_mutants_apply_to_the_tree_and_name_their_guards():
    check_mutant_table(mc.MIX_MUTANTS, (mc.MIX,), lxr)


def test_edits_change_values_only():
    """no edit touches a loop, a barrier, a launch or the indices of a workgroup"""
    for n, (_, _, edits) in mc.MIX_MUTANTS.items():
        for _, old, new in edits:
            for word in ("for (", "__syncthreads", "hipLaunchKernelGGL", "blockIdx", "threadIdx"):
                assert word not in old and word not in new, (n, word)


def test_library_names_do_not_collide():
    check_library_names(mc.MIX_MUTANTS, "libspc_mix_mutant2.so")
    rows = [t for t in mc.ALL_TABLES if t.table is mc.MIX_MUTANTS]
    assert len(rows) == 1 and (rows[0].flag, rows[0].kernel, rows[0].module, rows[0].gpu_test) == ("mix", "K24", "les_mix_ref", "test_les_mix_gpu")
    tags = [mc._tag(t.table) for t in mc.ALL_TABLES]
    assert len(set(tags)) == len(tags) and len({t.flag for t in mc.ALL_TABLES}) == len(mc.ALL_TABLES)
    # what check_library_names and tests/test_les_harness_cpu.py ask of the rows of TABLES, of every row of ALL_TABLES
    tables = [t.table for t in mc.ALL_TABLES] + [t.equivalent for t in mc.ALL_TABLES if t.equivalent]
    libs = [mc.lib_of(n, t) for t in tables for n in t]
    assert len(set(libs)) == len(libs)
    for e in mc.LATER_TABLES:
        module = importlib.import_module("tests." + e.module)
        importlib.import_module("tests." + e.gpu_test)
        for n, (what, guard, edits) in e.table.items():
            mod, name = guard.__name__.split(".", 1)
            assert mod == e.module and name in module.BODIES and callable(getattr(module, "check_" + name)), (e.flag, n)


def test_every_body_is_run_by_the_control():
    check_jobs_are_bodies(lxr)
