"""K9 (sp_coupler_amd/csrc/spc_lesstate.hpp) against the unchanged host spcpl.set_les_state, run on recording LES after
re-seeding: the helpers and the bodies of the GPU tests, each taking an engine (tests/test_les_state_gpu.py hands them
Engine("cuda:0"); tools/mutation_control.py hands them the engines of its mutant libraries).  Every body asks for equal bits
and an equal numpy.random.get_state() tuple.

Numbering used below (the kernel's): word 0 is key[0] of the start state, the launch draws the words pos ... pos + 8 cells - 1,
generation g holds the words 624 g ... 624 g + 623, and with L generations per substream, substream s twists the
generations s L + 1 ... s L + L (substream 0 also emits what is left of generation 0).  From an even pos an element's first
word is even; from an odd pos it is odd, and the word 624 g is the second half of a double that began in generation g - 1."""
import contextlib

import numpy

from sp_coupler_amd import _abi, spcpl
from tests.les_harness import run_bodies

MT_N = 624


class RecLES:
    """an LES that records what the coupler sets"""

    def __init__(self, shape):
        self.shape = shape
        self.calls = []

    def get_itot(self):
        return self.shape[0]

    def get_jtot(self):
        return self.shape[1]

    def get_ktot(self):
        return self.shape[2]

    def set_field(self, name, values):
        self.calls.append((name, numpy.array(values)))

    def set_surface_pressure(self, ps):
        self.calls.append(("PS", float(ps)))


def _odd_start(seed=42):
    """a state with a cached Gaussian and an odd pos"""
    numpy.random.seed(seed)
    numpy.random.normal()                         # draws a pair: has_gauss = 1
    numpy.random.randint(0, 2 ** 32, size=3, dtype=numpy.uint32)
    s = numpy.random.get_state()
    assert s[3] == 1 and s[2] % 2 == 1
    return s


def _profiles(shapes, seed=3):
    rng = numpy.random.default_rng(seed)
    return [[rng.normal(m, 1.0, s[2]) for s in shapes] for m in (5.0, -3.0, 300.0, 0.01)]


def _same_state(a, b):
    assert a[0] == b[0] and numpy.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] and a[4] == b[4]


def _same_calls(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [c[0] for c in g.calls] == [c[0] for c in w.calls]
        for (_, x), (_, y) in zip(g.calls, w.calls):
            assert numpy.array_equal(x, y)


def _run_both(shapes, start, ps=None, **kw):
    u, v, thl, qt = _profiles(shapes)
    want = [RecLES(s) for s in shapes]
    numpy.random.set_state(start)
    for l, les in enumerate(want):
        spcpl.set_les_state(les, u[l], v[l], thl[l], qt[l], None if ps is None else ps[l])
    s_want = numpy.random.get_state()
    got = [RecLES(s) for s in shapes]
    numpy.random.set_state(start)
    spcpl.set_les_state_batched(got, u, v, thl, qt, ps=ps, **kw)
    _same_calls(got, want)
    _same_state(numpy.random.get_state(), s_want)


@contextlib.contextmanager
def installed(eng):
    """``eng`` as the engine of spcpl for the duration of a body; the engine and NumPy's global state are put back after"""
    saved, prev = numpy.random.get_state(), spcpl._engine
    spcpl.set_engine(eng)
    try:
        yield
    finally:
        spcpl.set_engine(prev)
        numpy.random.set_state(saved)


# ---- the bodies tests/test_les_state_gpu.py had before this module ------------------------------------------------------------
def check_mixed_shapes(eng):
    with installed(eng):
        shapes = [(7, 5, 19), (64, 64, 160), (1, 1, 3), (3, 4, 19), (8, 8, 160)]
        _run_both(shapes, _odd_start(), ps=[101325.0, 0.0, 99000.5, 98000.0, 100000.0])


FORCED_GENS = (1, 3, 7)


def check_forced_short_substreams(eng, gens=FORCED_GENS):
    """many substream boundaries, doubles whose two words straddle them, the prefix from an odd pos"""
    with installed(eng):
        for g in gens:
            shapes = [(7, 5, 19), (5, 3, 11), (16, 16, 40), (7, 5, 19)]
            _run_both(shapes, _odd_start(7), gens_per_substream=g)


def check_twist_boundary(eng):
    with installed(eng):
        numpy.random.seed(1)
        _run_both([(4, 4, 40), (2, 2, 30)], numpy.random.get_state())          # pos 624: the first word needs a twist
        numpy.random.seed(1)
        numpy.random.random_sample(100)
        _run_both([(1, 2, 3)], numpy.random.get_state())                       # 48 words from pos 200: no twist at all
        numpy.random.seed(1)
        numpy.random.random_sample(4)
        _run_both([(1, 1, 1), (1, 1, 2), (1, 1, 74)], numpy.random.get_state())  # 616 words from pos 8: ends at pos 624


def check_engine_level(eng):
    """Engine.les_state on one shape: [n x itot x jtot x ktot] fields and the state NumPy (and the host jump) reach"""
    with installed(eng):
        shapes = [(16, 16, 32)] * 3
        u, v, thl, qt = (numpy.stack(p) for p in _profiles(shapes))
        s = _odd_start(5)
        fields, (key, pos) = eng.les_state(shapes, u, v, thl, qt, s, gens_per_substream=5)
        numpy.random.set_state(s)
        for l in range(3):
            for name, amp, prof in zip(("U", "V", "THL", "QT"), (0.5, 0.5, 0.1, 2.5e-5), (u, v, thl, qt)):
                want = amp * numpy.random.uniform(-1., 1., shapes[l]) + prof[l]
                assert numpy.array_equal(fields[name][l].cpu().numpy(), want), (l, name)
        s1 = numpy.random.get_state()
        assert pos == s1[2] and numpy.array_equal(key, s1[1])
        k2, p2 = _abi.mt19937_jump(s[1], s[2], 8 * 3 * 16 * 16 * 32)
        assert p2 == pos and numpy.array_equal(k2, key)


# ---- seek_boundaries: an LES that begins on the first element a substream emits ----------------------------------------------
def start_at(pos_mod8, seed):
    """a state whose pos is ``pos_mod8`` modulo 8 (0: an even start; 1: an odd start with a cached Gaussian, as _odd_start)"""
    s = _odd_start(seed)
    numpy.random.set_state(s)
    numpy.random.randint(0, 2 ** 32, size=(pos_mod8 - s[2]) % 8, dtype=numpy.uint32)
    s = numpy.random.get_state()
    assert s[2] % 8 == pos_mod8 and s[3] == 1 and 0 < s[2] < MT_N
    return s


def _filler(cells):
    """LES shapes holding ``cells`` cells in all, with ktot > 1 where that divides"""
    out = []
    while cells:
        kt = next(k for k in (19, 11, 7, 5, 3, 2, 1) if k <= cells)
        j = min(cells // kt, 23)
        out.append((1, j, kt))
        cells -= j * kt
    return out


def first_word(pos, s, L):
    """the first word of the first element substream s >= 1 emits: the first word of generation s L + 1 that starts a double"""
    return MT_N * (s * L + 1) + (pos & 1)


def seek_shapes(pos, L, at=((2, (1, 1, 1)), (5, (4, 3, 7)), (7, (1, 1, 1)), (9, (1, 1, 1)))):
    """(shapes, indices of the aligned LES): before every (s, shape) of ``at`` as many filler cells as put that LES's first
    word on first_word(pos, s, L); the last aligned LES is the last LES of the list"""
    shapes, aligned, words = [], [], pos
    for s, shape in at:
        gap = first_word(pos, s, L) - words
        assert gap >= 0 and gap % 8 == 0, (pos, s, L, gap)
        shapes += _filler(gap // 8)
        aligned.append(len(shapes))
        shapes.append(shape)
        words = first_word(pos, s, L) + 8 * shape[0] * shape[1] * shape[2]
    return shapes, aligned


def seek_cases():
    """(L, start state, shapes, aligned) for L = 1, 2 from an even and from an odd pos, the alignment asserted from the offsets"""
    cases = []
    for L in (1, 2):
        for mod8, seed in ((0, 51), (1, 52)):
            start = start_at(mod8, seed)
            pos = start[2]
            shapes, aligned = seek_shapes(pos, L)
            off = pos + 8 * numpy.concatenate([[0], numpy.cumsum([i * j * k for i, j, k in shapes])])
            for l in aligned:
                g, j = divmod(int(off[l]), MT_N)
                assert j == (pos & 1) and g >= 1 and (g - 1) % L == 0 and (g - 1) // L >= 1, (L, pos, l, g, j)
            assert aligned[-1] == len(shapes) - 1 and shapes[aligned[0]] == (1, 1, 1) and shapes[-1] == (1, 1, 1)
            T = (int(off[-1]) - 1) // MT_N
            assert (T + L - 1) // L >= 10                      # the launch has the substreams the aligned LES sit on
            cases.append((L, start, shapes, aligned))
    return cases


def check_seek_boundaries(eng):
    """item 6: an LES (of one cell, of several, the last of the list) begins exactly on the first element a substream emits,
    from an even pos (the generation's first word) and from an odd pos (its second word: the first belongs to a double that
    straddles the generations)"""
    with installed(eng):
        for L, start, shapes, aligned in seek_cases():
            _run_both(shapes, start, gens_per_substream=L)


# ---- odd_substream_counts: K = 3, 5, 7 substreams ------------------------------------------------------------------------------
ODD_L = 4


def odd_count_cases():
    """(T, K, L, start state, shapes): T = K L and T = K L - 1 generations for K = 3, 5, 7, the launch ending at pos 624
    exactly (q = 624 (T + 1)); one LES, and three LES of which the last ends there; and one list from an odd pos"""
    cases = []
    for K in (3, 5, 7):
        for T in (K * ODD_L, K * ODD_L - 1):
            start = start_at(0, 60 + K)
            cells, rem = divmod(MT_N * (T + 1) - start[2], 8)
            assert rem == 0
            kt = next(k for k in (19, 17, 13, 11, 7, 5, 3, 2, 1) if cells % k == 0)
            for shapes in ([(1, cells // kt, kt)], [(2, 3, 5), (1, 1, 1)] + [(1, cells - 31, 1)]):
                q = start[2] + 8 * sum(i * j * k for i, j, k in shapes)
                assert q == MT_N * (T + 1) and (q - 1) // MT_N == T and (T + ODD_L - 1) // ODD_L == K
                cases.append((T, K, ODD_L, start, shapes))
        start = _odd_start(70 + K)
        shapes = [(3, 5, 7), (1, (MT_N * K * ODD_L - 900) // 8, 1), (2, 2, 3)]
        T = (start[2] + 8 * sum(i * j * k for i, j, k in shapes) - 1) // MT_N
        assert (T + ODD_L - 1) // ODD_L == K
        cases.append((T, K, ODD_L, start, shapes))
    return cases


def check_odd_substream_counts(eng):
    """item 6: substream counts that are no power of two (the jump rounds leave the starts K ... 2^rounds - 1 alone), a last
    substream of L and of L - 1 generations, one LES, a launch that ends on the last word of a generation (pos 624)"""
    with installed(eng):
        for T, K, L, start, shapes in odd_count_cases():
            _run_both(shapes, start, gens_per_substream=L)


OLD_BODIES = ("mixed_shapes", "forced_short_substreams", "twist_boundary", "engine_level")
NEW_BODIES = ("seek_boundaries", "odd_substream_counts")


BODIES = OLD_BODIES + NEW_BODIES


def jobs(eng, names=BODIES):
    return [(name, lambda name=name: globals()["check_" + name](eng)) for name in names]


def check_everything(eng, names=BODIES):
    """the bodies ``names`` on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the names of
    the bodies that failed (AssertionError) in the order they ran."""
    return run_bodies(names, jobs(eng, names))
