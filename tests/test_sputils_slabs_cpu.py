"""K7's launch choice without a GPU: spc_sputils_describe_launch (include/spc.h; host only, no pointer dereferenced) against
su_rows' rule restated here and against heights worked out by hand, the cut that keeps a slab's 32-bit byte offsets below 2^32,
the refusal of ONE-row launches those offsets cannot address, SuWalk's reciprocal restated and checked exhaustively, and the
bodies of tests/sputils_slabs.py on the oracle-backed engine (which tests the bodies' own expectations, not a kernel)."""
import pytest
import torch

from sp_coupler_amd import _abi
from tests import sputils_slabs as ss

THREADS, TARGET = 256, 1100


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def su_rows(n_rows, n_out, per_row, fixed, es, cus, max_pitch, cap=16 * 1024, fit_rounds=True):
    """the rule of su_rows (spc_sputils_host.hpp) in its own words: about TARGET outputs per workgroup, at most 64 rows, at least
    four workgroups per compute unit, the slab within the LDS budget; then, among the heights within two rows of that, the one
    whose last round of 256 outputs idles least (by more than 2 %); then the 32-bit byte offsets.  Returns (rb, staged)"""
    rb = min(64, max(1, -(-TARGET // n_out)))
    most = n_rows // (4 * cus)
    rb = max(1, min(rb, most))
    fits = lambda c: (per_row * c + fixed) * es <= cap                              # noqa: E731
    while rb > 1 and not fits(rb):
        rb -= 1
    if fit_rounds:
        def waste(c):
            rounds = -(-c * n_out // THREADS)
            return (rounds * THREADS - c * n_out) / (rounds * THREADS)
        best = rb
        for c in range(max(rb - 2, 1), min(rb + 2, 64) + 1):
            if (c > most and c > 1) or (not fits(c) and c > rb):
                break
            if waste(c) < waste(best) - 0.02:
                best = c
        rb = best
    while rb > 1 and rb * max_pitch * 8 >= 2 ** 32:
        rb -= 1
    return rb, (per_row * rb + fixed) * es <= 64 * 1024


def interp_text(lib, es, n, n_x, n_xp, shared_xp=False, pitch=None):
    a = _abi.InterpArgs(n, n_x, n_xp, n_x, 0 if shared_xp else n_xp, pitch or n_xp, n_x, 1, 1, 1, 1)    # dummy pointers
    return ss.parse(_abi.sputils_describe_launch(lib, _abi.SPC_SU_INTERP, es, a))


def search_text(lib, es, n, n_a, n_v, shared_a=False):
    a = _abi.SearchsortedArgs(n, n_a, n_v, 0 if shared_a else n_a, n_v, n_v, 1, 1, 1, 1, 0)
    return ss.parse(_abi.sputils_describe_launch(lib, _abi.SPC_SU_SEARCHSORTED, es, a))


def coarse_text(lib, es, n, nG, nL, shared=False, mode=0, rho=True):
    a = _abi.InterpCArgs(n, nG, nL, nG + 1, 0 if shared else nL, nL - 1, nG, 1, 1, 1, 1 if rho else None, 1, mode, 0)
    return ss.parse(_abi.sputils_describe_launch(lib, _abi.SPC_SU_INTERP_C, es, a))


@pytest.mark.parametrize("cus", [32, 64, 128, 256])
def test_one_row_per_workgroup_below_four_workgroups_per_cu(lib, monkeypatch, cus):
    """the cap n_rows / (4 cus): below 2 x 4 x cus rows every operator runs one row per workgroup -- on 256 compute units every
    launch of fewer than 2 048 rows, which is every oracle comparison of tests/test_sputils_gpu.py at 37 to 300 rows"""
    monkeypatch.setenv("SPC_CUS", str(cus))
    for es in (8, 4):
        for n in (1, 37, min(300, 8 * cus - 1), 4 * cus, 8 * cus - 1):
            texts = [interp_text(lib, es, n, 160, 91), search_text(lib, es, n, 91, 160), coarse_text(lib, es, n, 91, 160)]
            assert [d.rb for d in texts] == [1, 1, 1] and all(d.grid == n and d.cus == cus for d in texts), (n, texts)
        texts = [interp_text(lib, es, 8 * cus, 160, 91), search_text(lib, es, 8 * cus, 91, 160), coarse_text(lib, es, 8 * cus, 91, 160)]
        assert [d.rb for d in texts] == [2, 2, 2] and all(d.grid == 4 * cus for d in texts), texts


def test_heights_worked_out_by_hand(lib, monkeypatch):
    """256 compute units, 348 528 rows (up to 340 rows per slab allowed).  interp, 91 samples per row: a row is 91 + su_pad(64) = 221 elements of LDS.
    160 queries: ceil(1100 / 160) = 7 rows = 4.4 rounds; 8 rows = exactly 5 rounds: fit_rounds takes 8.  8 queries: 64 rows asked,
    16 384 / (221 x 8 B) = 9.27: 9 rows (float: 18); xp shared: (16 384 / 8 - 130) / 91 = 21.08: 21 rows (float: (4 096 - 130) / 91
    = 43).  1 100 queries: one row asked = 4.3 rounds paid as 5 (14 % idle), two rows 8.6 as 9 (4.5 %), three 12.9 as 13 (0.8 %):
    fit_rounds takes 3; 550: two rows asked, four = 8.6 rounds as 9 (three: 7.9 %, not 2 % better than ... four: 4.5 %): 4.  A table
    of 4 entries, 5 queries: 64.  searchsorted with a shared table of 91: no LDS per row, 7 keys: 64.  interp_c 91 <- 160 levels, shared zh: a
    row is 2 x 159 + 183 = 501 elements, 258 fixed: (32 768 / 8 - 258) / 501 = 7.66: 7 rows, ceil(1100 / 91) = 13 asked (no
    fit_rounds); zh per row: 759 elements: 5 rows; float: 13 (the first choice) and 10."""
    monkeypatch.setenv("SPC_CUS", "256")
    n = 348528
    assert [interp_text(lib, es, n, 160, 91).rb for es in (8, 4)] == [8, 8]
    assert [interp_text(lib, es, n, 8, 91).rb for es in (8, 4)] == [9, 18]
    assert [interp_text(lib, es, n, 8, 91, shared_xp=True).rb for es in (8, 4)] == [21, 43]
    assert [interp_text(lib, 8, n, k, 91).rb for k in (1100, 1101, 550, 5000)] == [3, 3, 4, 1]
    assert interp_text(lib, 8, n, 5, 4).rb == 64 and search_text(lib, 8, n, 91, 7, shared_a=True).rb == 64
    assert [coarse_text(lib, es, n, 91, 160, shared=s).rb for es in (8, 4) for s in (True, False)] == [7, 5, 13, 10]
    assert interp_text(lib, 8, n, 160, 91) == ss.Desc("k_interp<f64,sl=7,wt=0>", 8, -(-n // 8), 8 * 221 * 8, 256)
    n = 35718                                                # (46 MB of interp results: write-through stores)
    assert interp_text(lib, 8, n, 160, 91) == ss.Desc("k_interp<f64,sl=7,wt=1>", 8, -(-n // 8), 8 * 221 * 8, 256)
    assert coarse_text(lib, 8, n, 91, 160, shared=True).name == "k_interp_c<f64,pd=1,sl=8,w=1,wt=1>"
    assert coarse_text(lib, 8, n, 91, 160, mode=1).name == "k_interp_c<f64,pd=1,sl=8,w=0,wt=1>"          # interp_rho ignores rho
    assert coarse_text(lib, 8, n, 91, 160, mode=2, rho=False).name == "k_interp_c<f64,pd=1,sl=8,w=0,wt=1>"
    assert coarse_text(lib, 4, n, 91, 160).name == "k_interp_c<f32,pd=-1,sl=0,w=1,wt=1>"
    assert coarse_text(lib, 8, 40, 31, 2000).name == "k_interp_c<f64,pd=-1,sl=0,w=1,wt=1>"              # staged, explicit stack
    assert interp_text(lib, 8, 3, 50, 9000).name == "k_interp<f64,sl=-1,wt=1>" and interp_text(lib, 8, 3, 50, 9000).lds == 0
    # more than 64 MiB written: plain stores
    assert interp_text(lib, 8, 52429, 160, 91).name.endswith("wt=0>") and interp_text(lib, 8, 52428, 160, 91).name.endswith("wt=1>")
    assert search_text(lib, 4, 52429, 91, 160).name == "k_searchsorted<f32,sl=0,wt=0>"                   # int64 indices
    assert _abi.sputils_describe_launch(lib, _abi.SPC_SU_RMS, 8, None, 33, 300, 300) == "k_rms<f64,pd=2,wt=1> rb=32 grid=2 lds=0 cus=256"
    assert _abi.sputils_describe_launch(lib, _abi.SPC_SU_EXNER, 4, None, 0, 1000, 0) == "k_exner<f32,wt=1> rb=0 grid=2 lds=0 cus=256"
    assert _abi.sputils_describe_launch(lib, _abi.SPC_SU_RMS, 8, None, 0, 300, 300).startswith("none ")
    with pytest.raises(_abi.SpcInvalidArgument):
        _abi.sputils_describe_launch(lib, 5, 8, None)
    with pytest.raises(_abi.SpcInvalidArgument):
        _abi.sputils_describe_launch(lib, _abi.SPC_SU_INTERP, 2, _abi.InterpArgs(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1))
    with pytest.raises(_abi.SpcInvalidArgument, match="pitch is smaller"):
        interp_text(lib, 8, 5, 160, 91, pitch=90)


@pytest.mark.parametrize("cus", [32, 64, 128, 256])
def test_the_description_follows_the_rule_of_su_rows(lib, monkeypatch, cus):
    """rows x outputs x table lengths x sharing x element size against the restatement above: rb, grid and LDS bytes"""
    monkeypatch.setenv("SPC_CUS", str(cus))
    for es in (8, 4):
        for n in (300, 8 * cus, 13 * 4 * cus + 5, 35718, 348528):
            for n_out in (1, 7, 91, 137, 160, 256, 300, 512, 1100, 5000):
                for n_tab in (1, 4, 91, 160, 512, 1100):
                    for shared in (False, True):
                        pad = ss.su_pad(n_tab)
                        per_row, fixed = n_tab + (0 if shared else pad), pad if shared else 0
                        rb, staged = su_rows(n, n_out, per_row, fixed, es, cus, max(n_out, n_tab))
                        d = interp_text(lib, es, n, n_out, n_tab, shared_xp=shared)
                        assert (d.rb, d.grid, d.lds) == (rb, -(-n // rb), (per_row * rb + fixed) * es if staged else 0), (n, n_out, n_tab, shared, d)
                        per_row, fixed = (0 if shared else pad), pad if shared else 0
                        rb, staged = su_rows(n, n_out, per_row, fixed, es, cus, max(n_out, n_tab))
                        d = search_text(lib, es, n, n_tab, n_out, shared_a=shared)
                        assert (d.rb, d.grid, d.lds) == (rb, -(-n // rb), (per_row * rb + fixed) * es), (n, n_out, n_tab, shared, d)
                        if n_tab >= 2 and n_out <= 512:
                            pad = ss.su_pad(n_tab - 1)
                            per_row, fixed = 2 * (n_tab - 1) + 2 * n_out + 1 + (0 if shared else pad), pad if shared else 0
                            rb, staged = su_rows(n, n_out, per_row, fixed, es, cus, max(n_out + 1, n_tab), cap=32 * 1024, fit_rounds=False)
                            d = coarse_text(lib, es, n, n_out, n_tab, shared=shared)
                            assert (d.rb, d.grid, d.lds) == (rb, -(-n // rb), (per_row * rb + fixed) * es if staged else 0), (n, n_out, n_tab, shared, d)


def test_the_cut_at_2_pow_32_bytes_of_slab(lib, monkeypatch):
    """the kernels address a slab with 32-bit BYTE offsets r * pitch + i: su_rows cuts the height so that rb * pitch * 8 stays
    below 2^32 whatever chose it.  Rows 2^23 elements apart, a table of 4 entries and 5 queries (64 rows asked; 256 rows with one
    compute unit counted allow them): 64 x 2^23 x 8 = 2^32, so 63; half that pitch keeps 64.  (The device test of the refusals,
    tests/test_sputils_gpu.py, has 4 rows: its height is 1 before the cut is looked at.  A device check of the cut would need a
    buffer of 4 GiB.)"""
    monkeypatch.setenv("SPC_CUS", "1")
    for es in (8, 4):
        d = interp_text(lib, es, 256, 5, 4, pitch=2 ** 23)
        assert d.rb == 63 and d.rb * 2 ** 23 * 8 < 2 ** 32 and d.grid == 5, d
        assert interp_text(lib, es, 256, 5, 4, pitch=2 ** 22).rb == 64
        assert interp_text(lib, es, 256, 5, 4, pitch=2 ** 24 - 1).rb == 32 and 33 * (2 ** 24 - 1) * 8 >= 2 ** 32
        a = _abi.SearchsortedArgs(256, 91, 7, 0, 7, 2 ** 23, 1, 1, 1, 0, 0)                       # the pitch of the int64 indices
        assert ss.parse(_abi.sputils_describe_launch(lib, _abi.SPC_SU_SEARCHSORTED, es, a)).rb == 63
        a = _abi.InterpCArgs(256, 4, 92, 5, 0, 2 ** 23, 4, 1, 1, 1, 1, 1, 0, 0)                  # q and rho
        full = coarse_text(lib, es, 256, 4, 92, shared=True).rb
        cut = ss.parse(_abi.sputils_describe_launch(lib, _abi.SPC_SU_INTERP_C, es, a)).rb
        assert full <= 63 and cut == full                                                        # (the LDS leaves fewer rows anyway)
    d = interp_text(lib, 8, 64, 5, 4, pitch=2 ** 23)                                             # 64 rows: 16 per slab, the cut is idle
    assert d.rb == 16


def _refused(lib, op, es, args, text):
    with pytest.raises(_abi.SpcError) as e:
        _abi.sputils_describe_launch(lib, op, es, args)
    assert e.value.code == _abi.SPC_ERR_UNSUPPORTED and text in str(e.value), str(e.value)


def test_one_row_launches_beyond_the_32_bit_byte_offsets_are_refused(lib):
    """su_at addresses element i of a row as base + (unsigned)(i * sizeof(T)); a ONE-row launch is exempt from the 2^24 pitch rule
    (its pitch is never multiplied), so one row of 2^29 doubles -- 2^30 floats; 2^29 keys of either type, the indices are int64 --
    wrapped the offset and computed the wrong elements without a fault.  Refused now, in the description (dummy pointers, nothing
    is dereferenced) and by the launchers themselves, which run the same choose_* and refuse in FRONT of their pointer checks:
    they are called with NULL pointers here, so a refusal that regressed would end as "required pointer is NULL", never as a launch.  One element fewer passes this check; two
    rows of that length were and are refused by the pitch rule."""
    stream = None
    for es, limit, text in ((8, 2 ** 29, "2^29"), (4, 2 ** 30, "2^30")):
        big = _abi.InterpArgs(1, limit, 3, limit, 3, 3, limit, 1, 1, 1, 1)
        _refused(lib, _abi.SPC_SU_INTERP, es, big, text)
        fn = lib.spc_interp_f64 if es == 8 else lib.spc_interp_f32
        null = _abi.InterpArgs(1, limit, 3, limit, 3, 3, limit, None, None, None, None)
        assert fn(null, stream) == _abi.SPC_ERR_UNSUPPORTED and text in lib.spc_last_error().decode()      # refused before any launch
        ok = _abi.InterpArgs(1, limit - 1, 3, limit - 1, 3, 3, limit - 1, 1, 1, 1, 1)
        d = ss.parse(_abi.sputils_describe_launch(lib, _abi.SPC_SU_INTERP, es, ok))
        assert d.rb == 1 and d.grid == 1 and d.name.endswith("wt=0>")
        null = _abi.InterpArgs(1, limit - 1, 3, limit - 1, 3, 3, limit - 1, None, None, None, None)
        assert fn(null, stream) == _abi.SPC_ERR_INVALID_ARGUMENT and "NULL" in lib.spc_last_error().decode()   # one fewer: the next check
        _refused(lib, _abi.SPC_SU_INTERP, es, _abi.InterpArgs(2, limit, 3, limit, 3, 3, limit, 1, 1, 1, 1), "2^24")
        # a long TABLE is read through 64-bit pointers (rows beyond the LDS): served
        assert ss.parse(_abi.sputils_describe_launch(lib, _abi.SPC_SU_INTERP, es, _abi.InterpArgs(1, 5, limit, 5, limit, limit, 5, 1, 1, 1, 1))).name.endswith("sl=-1,wt=1>")
        keys = 2 ** 29
        big = _abi.SearchsortedArgs(1, 3, keys, 3, keys, keys, 1, 1, 1, 1, 0)
        _refused(lib, _abi.SPC_SU_SEARCHSORTED, es, big, "2^29")
        fn = lib.spc_searchsorted_f64 if es == 8 else lib.spc_searchsorted_f32
        null = _abi.SearchsortedArgs(1, 3, keys, 3, keys, keys, None, None, None, 1, 0)
        assert fn(null, stream) == _abi.SPC_ERR_UNSUPPORTED and "2^29" in lib.spc_last_error().decode()
        ok = _abi.SearchsortedArgs(1, 3, keys - 1, 3, keys - 1, keys - 1, 1, 1, 1, 1, 0)
        assert ss.parse(_abi.sputils_describe_launch(lib, _abi.SPC_SU_SEARCHSORTED, es, ok)).rb == 1
        _refused(lib, _abi.SPC_SU_SEARCHSORTED, es, _abi.SearchsortedArgs(2, 3, keys, 3, keys, keys, 1, 1, 1, 1, 0), "2^24")
        # the same gap in interp_c: the coarse bounds Zh[0 .. nG] and the results of one row
        big = _abi.InterpCArgs(1, limit - 1, 3, limit, 3, 2, limit - 1, 1, 1, 1, 1, 1, 0, 0)
        _refused(lib, _abi.SPC_SU_INTERP_C, es, big, text)
        fn = lib.spc_interp_c_f64 if es == 8 else lib.spc_interp_c_f32
        null = _abi.InterpCArgs(1, limit - 1, 3, limit, 3, 2, limit - 1, None, None, None, None, None, 0, 0)
        assert fn(null, stream) == _abi.SPC_ERR_UNSUPPORTED and text in lib.spc_last_error().decode()
        ok = _abi.InterpCArgs(1, limit - 2, 3, limit - 1, 3, 2, limit - 2, 1, 1, 1, 1, 1, 0, 0)
        assert ss.parse(_abi.sputils_describe_launch(lib, _abi.SPC_SU_INTERP_C, es, ok)).rb == 1


def test_suwalk_divides_by_a_reciprocal_that_is_exact_below_256():
    """SuWalk (spc_sputils.hpp) takes tid / n for tid < 256 as (tid * ceil(2^16 / n)) >> 16 where n < 256: exact for every pair --
    the bound is 255 n < 2^16, the error of the rounded-up reciprocal times the largest tid stays below one step -- while the
    rounded-DOWN reciprocal is wrong at 955 pairs, first at n = 3, tid = 3.  And the step (dr, di) = divmod(256, n) with one carry
    walks every output e = tid + 256 k of a slab to (e // n, e % n)."""
    up = [(n, t) for n in range(1, 256) for t in range(256) if (t * -(-65536 // n)) >> 16 != t // n]
    down = [(n, t) for n in range(1, 256) for t in range(256) if (t * (65536 // n)) >> 16 != t // n]
    assert up == [] and len(down) == 955 and down[0] == (3, 3)
    assert all(255 * n < 2 ** 16 for n in range(1, 256)) and 255 * 258 >= 2 ** 16
    for n in list(range(1, 41)) + [127, 128, 129, 254, 255, 256, 257, 300, 511, 512, 513, 1100]:
        dr, di = divmod(THREADS, n)
        for tid in (0, 1, n - 1, n, 255):
            if not 0 <= tid < 256:
                continue
            r, i = (tid // n, tid % n) if n < 256 else ((1, tid - n) if tid >= n else (0, tid))
            for k in range(12):
                assert (r, i) == divmod(tid + THREADS * k, n), (n, tid, k)
                i, r = i + di, r + dr
                if i >= n:
                    i, r = i - n, r + 1


@pytest.mark.parametrize("dtype", ss.DTYPES, ids=["f64", "f32"])
def test_the_bodies_hold_on_the_oracle_engine_and_reach_every_name_they_claim(dtype):
    """every body on an engine that IS the oracle: its cases are well-formed, its slab heights are what it asserts (the description
    is the library's own), the poison it looks at is where it put it; and the names check_coverage expects are those the bodies'
    shapes get from the description (the launches themselves: tests/test_sputils_slabs_gpu.py)"""
    with ss.fresh_coverage():
        eng = ss.SlabOracleEngine(dtype)
        assert ss.check_everything(eng) == []
        ss.check_coverage(eng)
    assert [name for name, _ in ss.jobs(None)] == list(ss.BODIES) and all(hasattr(ss, "check_" + b) for b in ss.BODIES)


def test_a_body_that_got_one_row_per_workgroup_fails():
    """with the card's own count of compute units the few rows of a body get one row per workgroup: the body must not pass"""
    eng = ss.SlabOracleEngine(torch.float64)
    import numpy
    with ss.counted_cus(256), pytest.raises(AssertionError, match="slab height"):
        ss.OPS["interp"](eng, numpy.random.default_rng(1), 40, 160, 91)
