"""Proves tests/regex_craft.py on the CPU: the host matchers equal its golden,
every pattern has the table form its group claims, the crafted files decode
to the intended values, and the golden is not vacuous (both flags occur for
every file, pattern and polarity; every start residue and batch rank occurs
in the packed pages).  The GPU test (test_gpu_regex_bytes.py) then only has to
compare page flags."""
import numpy as np
import pytest

import regex_craft as R
from oracle import oracle as O
from pqgpu import capi
from util import to_oracle_chunk


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_host_matchers_equal_golden(pattern):
    """Glushkov NFA and the DFA image, both against Python's re, on every
    corpus value (-8: the DFA is over its size cap)."""
    over = capi.regex_dfa_info(pattern)["rc"] == -8
    assert over == (pattern in R.OVER_CAP)
    for v in set(R.corpus()):
        exp = int(R.match(pattern, v))
        assert capi.regex_match_host(pattern, v) == exp, (pattern, v)
        assert capi.regex_match_host_dfa(pattern, v) == (-8 if over else exp), (pattern, v)


def test_dollar_is_end_of_string():
    """`$` is \\Z: no match before a final newline (Python's re differs; the
    known answer is the contract, regex.hpp)."""
    for fn in (capi.regex_match_host, capi.regex_match_host_dfa):
        assert [fn("x$", b"x\n"), fn("x$", b"x")] == [0, 1]
    cf = R.kat_dollar()
    assert R.golden_flags(cf, "x$", False) == [1, 0] and R.golden_flags(cf, "x$", True) == [0, 1]
    assert not any(v.endswith(b"\n") for v in R.corpus())


def test_corpus_counts():
    c = R.corpus()
    assert c == R.corpus.__wrapped__()  # deterministic
    for p in R.NONTRIVIAL:
        m = sum(R.match(p, v) for v in c)
        assert m >= 8 and len(c) - m >= 8, (p, m)
    seen = set(b"".join(c))
    for b in b"09AZ_-. \t\n\r\x0b\x0c\x00\x01\x7f":
        assert b in seen
    assert {0xC2, 0xC3, 0xDF, 0xE0, 0xE2, 0xE6, 0xF0} <= seen  # 2-, 3- and 4-byte lead bytes
    assert {len(v.decode()) for v in c} >= set(R.RANDOM_LENGTHS)


FORMS = ([(p, True, False) for p in R.FULL_UNANCHORED] + [(p, True, True) for p in R.FULL_ANCHORED] +
         [(p, False, None) for p in R.CLASS_TABLE])


@pytest.mark.parametrize("pattern,full,anchored", FORMS)
def test_table_form(pattern, full, anchored):
    """The table form k_regex_plain gets: byte-indexed ("full"), its kSink
    variant (full and anchored) or the class table."""
    d = capi.regex_dfa_info(pattern)
    assert d["rc"] == 0 and d["full"] == full, d
    assert d["nclasses"] == 256 if full else d["nclasses"] < 256
    if anchored is not None:
        assert d["anchored"] == anchored, d


def test_table_form_boundaries():
    """build_dfa switches to the class table by size: the last full and the
    first class-form pattern of two families (62 | 63 states anchored,
    61 | 64 unanchored).  A change of the size rule fails here: re-pick them."""
    got = {p: capi.regex_dfa_info(p) for p in ("^[a-z]{59}x", "^[a-z]{60}x", ".{19}x", ".{20}x")}
    assert [(d["nstates"], d["full"]) for d in got.values()] == [(62, True), (63, False), (61, True), (64, False)], got
    assert got["^[a-z]{59}x"]["bytes"] == 32304 and got[".{19}x"]["bytes"] == 31792
    for p in R.TRIVIAL:
        assert capi.regex_dfa_info(p)["rc"] == 0


def all_files():
    yield R.s1()
    yield R.kat_dollar()
    yield R.s2()
    yield R.s4()
    yield R.s4_huge()
    for p in R.PACKED_PATTERNS:
        for neg in (False, True):
            yield R.s3(p, neg)
    for small in (True, False):
        for opt in (False, True):
            yield R.s5_entries(small, opt)
            for p in R.PACKED_PATTERNS:
                for neg in (False, True):
                    yield R.s5_mixed(p, neg, small, opt)


def test_files_decode_to_intended_values():
    """The oracle reads every crafted file (rc 0) to exactly the rows the
    golden is computed from, page by page; sizes stay small."""
    n = 0
    for cf in all_files():
        rc, msg, col = O.read_all(cf.file, to_oracle_chunk(cf.chunk))
        assert rc == 0, (cf.name, msg)
        data = [pg for pg in col.pages if pg[1] == 0]
        assert [pg[4] for pg in data] == [len(p) for p in cf.pages], cf.name
        rows = [v for p in cf.pages for v in p]
        assert col.valid.tolist() == [int(v is not None) for v in rows], cf.name
        raw = col.data.tobytes()
        assert raw == b"".join(v for v in rows if v is not None), cf.name
        assert np.array_equal(np.diff(col.offsets), [len(v) if v is not None else 0 for v in rows]), cf.name
        assert len(cf.pages) <= 1200 and len(cf.file) <= 1 << 20, (cf.name, len(cf.pages), len(cf.file))
        n += 1
    assert n == 5 + 12 + 4 * 13


def both_flags(cf, patterns, negs=(False, True)):
    for p in patterns:
        for neg in negs:
            fl = R.golden_flags(cf, p, neg)
            assert 0 in fl and 1 in fl, (cf.name, p, neg)


def test_golden_not_vacuous():
    """Every file x non-trivial pattern x polarity it is scanned with has a
    reported and an unreported page."""
    for cf in (R.s1(), R.s2()):
        both_flags(cf, R.NONTRIVIAL)
    for small in (True, False):
        for opt in (False, True):
            both_flags(R.s5_entries(small, opt), R.NONTRIVIAL)
    for cf in (R.s4(), R.s4_huge()):
        both_flags(cf, R.LONG_PATTERNS)
        if cf is R.s4_huge():  # the 70,000-byte pages themselves split
            for p in R.LONG_PATTERNS:
                big = [f for f, pg in zip(R.golden_flags(cf, p, False), cf.pages) if len(pg[0]) == R.HUGE]
                assert 0 in big and 1 in big, p
    for p in R.PACKED_PATTERNS:
        for neg in (False, True):
            both_flags(R.s3(p, neg), [p], [neg])
            for small in (True, False):
                for opt in (False, True):
                    both_flags(R.s5_mixed(p, neg, small, opt), [p], [neg])
    # all-NULL pages are reported whatever the pattern and polarity
    s2 = R.s2()
    null_pages = [i for i, p in enumerate(s2.pages) if all(v is None for v in p)]
    assert len(null_pages) > 50
    for neg in (False, True):
        fl = R.golden_flags(s2, "x*", neg)
        assert all(fl[i] == 1 for i in null_pages)


@pytest.mark.parametrize("neg", [False, True])
@pytest.mark.parametrize("pattern", R.PACKED_PATTERNS)
def test_packed_pages_cover_ranks_and_residues(pattern, neg):
    """S3: exactly the pages with a deciding value are unreported; the
    deciding values sit at ranks 0, 63, 64, 255, 256, 257 and 599, start at
    every payload offset mod 16, and are each of a lane's four interleaved
    strings under both window sizes the GPU test uses."""
    cf = R.s3(pattern, neg)
    assert all(len(p) == R.PAGE_VALUES for p in cf.pages)
    assert R.golden_flags(cf, pattern, neg) == [int(d is None) for d in cf.deciding]
    assert sum(d is None for d in cf.deciding) >= 3
    for pg, d in zip(cf.pages, cf.deciding):
        if d is not None:  # the recorded offset is where the deciding value's bytes start
            assert d[1] == sum(4 + len(v) for v in pg[:d[0]]) + 4
            assert R.match(pattern, pg[d[0]]) != neg
    ranks = [d[0] for d in cf.deciding if d is not None]
    assert ranks[:7] == R.DECIDING_RANKS
    residues = {d[1] % 16 for d in cf.deciding if d is not None}
    if any(len(v) % 4 for v in R.fillers_for(pattern, neg)):
        assert residues == set(range(16))
    else:  # ("^$" notlike: every filler is empty, a value starts at a multiple of 4)
        assert (pattern, neg) == ("^$", True) and residues == {0, 4, 8, 12}
    for win in (8192, 1024):
        assert R.batch_ranks(cf, win) == {0, 1, 2, 3}
    # some deciding value is decided past its first 16-byte block
    assert any(len(pg[d[0]]) > 16 for pg, d in zip(cf.pages, cf.deciding) if d is not None) or (pattern, neg) == ("^$", False)


def test_dictionary_sizes():
    """The small dictionary takes the armed one-pass filter (payload below
    kArmDictBytes), the whole corpus does not, and both stay one 16-bit pipe
    dictionary."""
    small = sum(4 + len(v) for v in R.dict_entries(True))
    whole = sum(4 + len(v) for v in R.dict_entries(False))
    assert 8192 < small < R.ARM_DICT_BYTES < whole <= 65536 - 64
    assert len(R.dict_entries(True)) > 256
