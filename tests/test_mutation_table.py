"""The mutation control's table (tools/mutation_control.py) against the current kernel sources, on the CPU: the shipped
sources carry no mutant switch, every mutant is present and guarded by a property of tests/semantic_props.py (K10's by a
body of tests/slab_edges.py), and every
edit still finds its line -- a kernel edit that drops or moves a mutant's line fails here, not as a SURVIVED mutant on the
GPU box."""
import os
import re

import pytest

from tests import semantic_props as sp
from tools import mutation_control as mc


def test_no_mutant_switch_in_the_shipped_sources(repo_root):
    hits = []
    for d in (mc.CSRC, os.path.join(repo_root, "include")):
        for name in sorted(os.listdir(d)):
            with open(os.path.join(d, name)) as f:
                hits += ["%s:%d" % (name, i + 1) for i, line in enumerate(f) if re.search(r"\bSPC_MUT", line)]
    assert not hits, hits


def test_every_mutant_is_guarded_by_a_property():
    assert sorted(mc.MUTANTS) == list(range(1, 36))
    names = {p.__name__[5:] for p in sp.PROPERTIES}
    from tests import slab_edges
    for n, (what, guard, edits) in mc.MUTANTS.items():
        assert what and edits, n
        if n < 28:
            assert guard in names, (n, guard)
        else:                                        # K10: a body of tests/slab_edges.py, run on the engines of the mutant library
            assert callable(guard) and all(e[0] == mc.SLAB for e in edits), n
            assert hasattr(slab_edges, "check_" + guard.__name__.split(".", 1)[1]), (n, guard.__name__)


@pytest.mark.parametrize("n", sorted(mc.MUTANTS))
def test_mutant_edits_apply_to_the_tree(n):
    files = mc.patched(n)        # raises when an edit's old text does not occur the expected number of times
    for name, text in files.items():
        with open(os.path.join(mc.CSRC, name)) as f:
            assert text != f.read(), (n, name)
