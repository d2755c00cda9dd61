"""K9's host side without a device: NumPy's MT19937 restated in plain Python, and the library's jump-ahead
(spc_mt19937_jump) against NumPy after drawing n words, from several start positions, and composed."""
import numpy
import pytest

from sp_coupler_amd import _abi, models

N, M = 624, 397
DEAD = numpy.array([0x80000000] + [0xffffffff] * (N - 1), dtype=numpy.uint32)     # the 31 low bits of key[0] are dead


class PyMT19937:
    """NumPy's legacy generator (randomkit), word by word"""

    def __init__(self, key, pos):
        self.key, self.pos = [int(k) for k in key], int(pos)

    def _twist(self):
        k = self.key
        for i in range(N):
            y = (k[i] & 0x80000000) | (k[(i + 1) % N] & 0x7fffffff)
            k[i] = k[(i + M) % N] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
        self.pos = 0

    def next32(self):
        if self.pos >= N:
            self._twist()
        y = self.key[self.pos]
        self.pos += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9d2c5680
        y ^= (y << 15) & 0xefc60000
        return y ^ (y >> 18)

    def uniform(self, low, high, n):
        out = []
        for _ in range(n):
            a, b = self.next32() >> 5, self.next32() >> 6
            out.append(low + (high - low) * ((a * 67108864.0 + b) / 9007199254740992.0))
        return numpy.array(out)


def _state(seed, pos=None):
    rs = numpy.random.RandomState(seed)
    s = rs.get_state()
    if pos is not None:
        rs.set_state((s[0], s[1], pos, 0, 0.0))
    return rs


def _draw_words(rs, n):
    """advance a legacy RandomState by exactly n 32-bit words (random_sample: two per double; randint over the full uint32
    range: one per value)"""
    if n // 2:
        rs.random_sample(n // 2)
    if n % 2:
        rs.randint(0, 2 ** 32, size=1, dtype=numpy.uint32)


def test_restatement_matches_numpy_uniform():
    """the formula of the issue: two words a, b per element, ((a >> 5) * 2^26 + (b >> 6)) / 2^53, from an odd pos"""
    for pos in (0, 623, 624, 301):
        rs = _state(11, pos)
        s = rs.get_state()
        py = PyMT19937(s[1], s[2])
        want = rs.uniform(-1., 1., (3, 5, 71))
        got = py.uniform(-1., 1., 3 * 5 * 71).reshape(3, 5, 71)
        assert numpy.array_equal(got, want)
        s1 = rs.get_state()
        assert py.pos == s1[2] and numpy.array_equal(numpy.array(py.key, dtype=numpy.uint32), s1[1])


def test_draw_words_advances_by_words():
    for n in (1, 2, 7, 1250):
        rs = _state(3, 17)
        s = rs.get_state()
        py = PyMT19937(s[1], s[2])
        for _ in range(n):
            py.next32()
        _draw_words(rs, n)
        s1 = rs.get_state()
        assert py.pos == s1[2] and numpy.array_equal(numpy.array(py.key, dtype=numpy.uint32), s1[1])


def _next_outputs(key, pos, n=2 * N):
    rs = numpy.random.RandomState()
    rs.set_state(("MT19937", numpy.asarray(key, dtype=numpy.uint32), int(pos), 0, 0.0))
    return rs.randint(0, 2 ** 32, size=n, dtype=numpy.uint32)


@pytest.mark.parametrize("start", [624, 0, 377])
@pytest.mark.parametrize("n", [0, 1, 623, 624, 625, 2 * 19937 + 3, 10 ** 7 + 1])
def test_host_jump_equals_numpy(start, n):
    rs = _state(2024, start)
    s0 = rs.get_state()
    key, pos = _abi.mt19937_jump(s0[1], s0[2], n)
    _draw_words(rs, n)
    s1 = rs.get_state()
    assert pos == s1[2]
    assert numpy.array_equal(key & DEAD, s1[1] & DEAD)
    assert numpy.array_equal(_next_outputs(key, pos), _next_outputs(s1[1], s1[2]))
    assert numpy.array_equal(key, s1[1])            # the last generation is twisted for real: every bit is NumPy's


@pytest.mark.parametrize("a,b", [(5, 619), (624 * 3, 1), (2 ** 40 + 12345, 2 ** 39 + 7), (2 ** 40 - 1, 2 ** 40 + 1)])
def test_jumps_compose(a, b):
    s = _state(99, 211).get_state()
    k1, p1 = _abi.mt19937_jump(*_abi.mt19937_jump(s[1], s[2], a), b)
    k2, p2 = _abi.mt19937_jump(s[1], s[2], a + b)
    assert p1 == p2
    assert numpy.array_equal(k1 & DEAD, k2 & DEAD)
    assert numpy.array_equal(_next_outputs(k1, p1), _next_outputs(k2, p2))


@pytest.mark.parametrize("T", [1, 2, 33, 34, 1000])
def test_jump_vs_numpy_by_generations(T):
    """n words that need exactly T twists: none of them jumped over (1), one (2), the jump polynomial of degree below and
    above the 33 generations of the stream the correlation reads (33, 34), a long jump (1000).  The jump this asks for is
    J = 624 (T - 1) words, always even: an odd J, the multiplication by x after the last squaring, cannot be reached through
    mt19937_jump and is checked on the polynomial itself in the two test_odd_jump_polynomials_* below"""
    for start, extra in ((0, 1), (311, 624)):
        rs = _state(4242, start)
        s0 = rs.get_state()
        n = N * T + extra - start
        assert (start + n - 1) // N == T
        key, pos = _abi.mt19937_jump(s0[1], s0[2], n)
        _draw_words(rs, n)
        s1 = rs.get_state()
        assert pos == s1[2] and numpy.array_equal(key, s1[1])


def test_jump_vs_numpy_from_both_branches_of_the_polynomial_cache():
    """x^J from the cached x^(J/2) (one squaring) and from nothing (square-and-multiply over the bits of J): J = 624 (T - 1)
    for T = 1001 after T = 501, and for T = 1203 before T = 602"""
    for T in (501, 1001, 1203, 602):
        rs = _state(77, 5)
        s0 = rs.get_state()
        n = N * T + 3 - 5
        key, pos = _abi.mt19937_jump(s0[1], s0[2], n)
        _draw_words(rs, n)
        s1 = rs.get_state()
        assert pos == s1[2] == 3 and numpy.array_equal(key, s1[1]), T


def _poly_int(J):
    return int.from_bytes(_abi.mt19937_jump_poly(J).tobytes(), "little")


def test_odd_jump_polynomials_multiply_by_x():
    """odd J: the multiplication by x after the last squaring, from a cached x^(J div 2) and from nothing.  x^J mod phi must
    be x * (x^(J-1) mod phi) reduced once by phi, here in Python integers"""
    phi = _poly_int(19937) | 1 << 19937
    for J, warm in ((624 * 1000 + 1, True), (624 * 1234 + 1, False), (2 ** 41 + 12345, True), (2 ** 41 + 54321, False)):
        assert J % 2 == 1
        if warm:
            _abi.mt19937_jump_poly(J // 2)                       # x^J then comes from the cache: one squaring, one mulx
        got = _poly_int(J)
        want = _poly_int(J - 1) << 1
        if want >> 19937:
            want ^= phi
        assert got == want and got >> 19937 == 0, J


def test_odd_jump_polynomials_compose_to_a_jump_numpy_confirms():
    """mt19937_jump only ever asks for J = 624 (T - 1), which is even, so the multiplication by x after the LAST squaring
    cannot be reached through it (the ones after earlier squarings are: every set bit of J but the lowest); and the test
    above takes its reference from the same routine at J - 1.  Here two odd powers are multiplied in Python integers:
    x^J1 * x^J2 mod phi must be x^(624 * 1000), the polynomial of the jump over 1000 generations, which is then applied to a
    state and compared with NumPy drawing the words"""
    phi = _poly_int(19937) | 1 << 19937
    for J1 in (624 * 1000 - 1, 311 * 1000 + 1, 12345):
        J2 = 624 * 1000 - J1
        assert J1 % 2 == 1 and J2 % 2 == 1
        a, b, prod = _poly_int(J1), _poly_int(J2), 0
        while b:
            low = b & -b
            prod ^= a << (low.bit_length() - 1)
            b ^= low
        for i in range(prod.bit_length() - 1, 19936, -1):
            if prod >> i & 1:
                prod ^= phi << (i - 19937)
        assert prod == _poly_int(624 * 1000), J1
    rs = _state(31, 100)
    s0 = rs.get_state()
    n = N * 1001 + 1 - 100                                       # T = 1001: the jump applies x^(624 * 1000)
    key, pos = _abi.mt19937_jump(s0[1], s0[2], n)
    _draw_words(rs, n)
    s1 = rs.get_state()
    assert pos == s1[2] == 1 and numpy.array_equal(key, s1[1])


def _bits(poly):
    return numpy.unpackbits(poly.view(numpy.uint8), bitorder="little")


def test_characteristic_polynomial_rederived():
    """phi (derived by the library with Berlekamp-Massey) re-checked here from its definition: x^J mod phi is x^J for
    J < 19937, x^19937 mod phi = phi - x^19937, and every bit sequence of the generator obeys the recurrence phi encodes"""
    for J in (0, 1, 63, 64, 19936):
        bits = _bits(_abi.mt19937_jump_poly(J))
        assert bits.sum() == 1 and bits[J] == 1
    low = _bits(_abi.mt19937_jump_poly(19937))[:19937].astype(numpy.int64)        # phi without its leading term
    assert low[0] == 1 and 100 < low.sum() < 19900
    rs = _state(5, 624)
    words = rs.randint(0, 2 ** 32, size=19937 + 64, dtype=numpy.uint32)
    # untempered words are a linear image of the tempered ones; every output bit is a linear recurring sequence with phi
    for bit in (0, 13, 31):
        s = ((words >> bit) & 1).astype(numpy.int64)
        for i in range(0, 64, 7):
            assert (s[i + 19937] + low @ s[i:i + 19937]) % 2 == 0


def test_jump_rejects_bad_arguments():
    s = _state(1).get_state()
    with pytest.raises(ValueError):
        _abi.mt19937_jump(s[1], 625, 1)
    with pytest.raises(ValueError):
        _abi.mt19937_jump(s[1], 0, -1)
    with pytest.raises(ValueError):
        _abi.mt19937_jump(s[1][:10], 0, 1)


@pytest.mark.parametrize("start", [624, 0, 5])
@pytest.mark.parametrize("n", [1, 2, 623, 1250, 2 * 19937 + 3])
def test_host_jump_against_the_restatement(start, n):
    """the plain-Python generator as the oracle: the jumped state continues where n single steps of it arrive"""
    s = _state(77, start).get_state()
    py = PyMT19937(s[1], s[2])
    for _ in range(n):
        py.next32()
    key, pos = _abi.mt19937_jump(s[1], s[2], n)
    assert pos == py.pos and numpy.array_equal(key, numpy.array(py.key, dtype=numpy.uint32))
    jumped = PyMT19937(key, pos)
    assert [jumped.next32() for _ in range(700)] == [py.next32() for _ in range(700)]


def test_ensemble_field_rows_keep_one_shape():
    ens = models.SyntheticLESEnsemble([1, 2, 3], numpy.linspace(10, 1000, 8), numpy.linspace(0, 1010, 9),
                                      {"QL": numpy.zeros((3, 8))})
    ens[0].set_field("U", numpy.ones((2, 2, 8)))
    ens[2].set_field("U", numpy.full((2, 2, 8), 3.0))
    assert ens.fields3d["U"].shape == (3, 2, 2, 8) and ens.fields3d["U"][2, 0, 0, 0] == 3.0
    with pytest.raises(ValueError):
        ens[1].set_field("U", numpy.ones((2, 2, 9)))
    assert ens.fields3d["U"][0, 0, 0, 0] == 1.0 and ens.fields3d["U"][2, 0, 0, 0] == 3.0
