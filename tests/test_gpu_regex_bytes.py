"""GPU parity of the regex page kernels on crafted bytes, lengths and start
alignments (tests/regex_craft.py; its golden and files are proven on the CPU
by test_regex_craft.py).

The generator's values never hold a digit, an upper-case letter, a control,
a NUL or a byte >= 0x80, are at most 44 bytes long, and hide a per-string
error among hundreds of values per page.  Here every value is its own page
(S1, S2, S4, the per-entry pages of S5) or the one value of its page that
decides the flag (S3, the mixed pages of S5), so a wrong table column, class,
block edge or start alignment flips a flag.

Kernels by shape (ctx.timing counts, test_kernels_by_shape):
S1-S4 REQUIRED/OPTIONAL PLAIN: k_regex_plain ("window"), k_regex_lanes
("codes", "lanes"; the 70,000-byte pages of S4 under every DFA setting),
k_regex_pages ("nfa", and "x.{10}$" always).  S5 dictionary: k_regex_dict
always, then k_pipe_match ("window", "codes"), k_regex_lanes or k_regex_pages;
the armed writer through decode_regex_async on the small dictionary.
"""
import numpy as np
import pytest

import regex_craft as R
from oracle import oracle as O
from pqgpu import capi
from util import to_desc, to_oracle_chunk

pytestmark = pytest.mark.gpu

POLARITY = pytest.mark.parametrize("neg", [False, True], ids=["like", "notlike"])
COUNTERS = ("regex_plain", "regex_lanes", "regex_pages", "regex_codes", "regex_dict")   # ctx.timing names


def check(dc, cf, pattern, neg, what=""):
    exp = np.array(R.golden_flags(cf, pattern, neg), dtype=np.uint8)
    got = dc.regex_pages(pattern, neg)
    if not np.array_equal(got, exp):
        bad = np.nonzero(got != exp)[0][:6] if len(got) == len(exp) else []
        pytest.fail(f"{cf.name} {what}: pattern {pattern!r} {'notlike' if neg else 'like'}: {len(got)} flags, "
                    f"expected {len(exp)}; first differing pages (expected flag {[int(exp[b]) for b in bad]}): "
                    f"{R.describe(cf, bad)}")


def scan_all(ctx, cf, patterns, neg, wins=(8192,), twice=False):
    dc = ctx.upload(cf.file, [to_desc(cf.chunk)])
    try:
        for win in wins:
            ctx.set_option("regex_win", win)
            for p in patterns:
                check(dc, cf, p, neg, f"regex_win {win}")
                if twice:  # REQUIRED PLAIN chunks: this one reads the string index the first filed
                    check(dc, cf, p, neg, f"regex_win {win}, second scan")
    finally:
        ctx.set_option("regex_win", 8192)
        dc.free()


@POLARITY
def test_s1_one_value_per_page(ctx, kernel, neg):
    """REQUIRED PLAIN, every corpus value its own page: the flags are the
    per-value results, for every pattern."""
    scan_all(ctx, R.s1(), R.PATTERNS, neg, wins=(8192, 1024), twice=True)


@POLARITY
def test_dollar_before_final_newline(ctx, kernel, neg):
    """x$ on "x\\n" and "x": [no match, match] by the contract ($ is \\Z)."""
    scan_all(ctx, R.kat_dollar(), ["x$"], neg, wins=(8192, 1024), twice=True)


@POLARITY
def test_s2_optional_nulls(ctx, kernel, neg):
    """OPTIONAL: [NULL, v, NULL] pages, RLE and bit-packed def levels, and
    all-NULL pages (reported under both polarities)."""
    scan_all(ctx, R.s2(), R.PATTERNS, neg)


@POLARITY
@pytest.mark.parametrize("pattern", R.PACKED_PATTERNS)
def test_s3_packed_pages(ctx, kernel, pattern, neg):
    """600 values per page, one of them deciding: at ranks 0, 63, 64, 255, 256,
    257, 599 (the windowed kernel takes 256 strings per batch, four per
    lane), at every start offset mod 16, and control pages without one."""
    scan_all(ctx, R.s3(pattern, neg), [pattern], neg, wins=(8192, 1024), twice=True)


@POLARITY
def test_s4_long_values(ctx, kernel, neg):
    """1,000 to 20,000-byte values (the window grows to the page's slot), the
    deciding byte first, last and at bytes 15, 16, 17 of a late block."""
    scan_all(ctx, R.s4(), R.LONG_PATTERNS, neg, twice=True)


@POLARITY
def test_s4_huge_values(ctx, kernel, neg):
    """70,000-byte pages: past the windowed kernel's 16-bit offsets, the chunk
    takes k_regex_lanes under the default options."""
    scan_all(ctx, R.s4_huge(), R.LONG_PATTERNS, neg)


@POLARITY
@pytest.mark.parametrize("optional", [False, True], ids=["req", "opt"])
@pytest.mark.parametrize("small", [True, False], ids=["small", "all"])
def test_s5_dictionary_entries(ctx, kernel, small, optional, neg):
    """The corpus as dictionary entries (k_regex_dict), a data page per entry
    (an RLE run of its index): the page's flag is the entry's result."""
    scan_all(ctx, R.s5_entries(small, optional), R.PATTERNS, neg)


@POLARITY
@pytest.mark.parametrize("optional", [False, True], ids=["req", "opt"])
@pytest.mark.parametrize("small", [True, False], ids=["small", "all"])
def test_s5_dictionary_mixed_pages(ctx, kernel, small, optional, neg):
    """Bit-packed index pages: fillers and one deciding index."""
    for p in R.PACKED_PATTERNS:
        scan_all(ctx, R.s5_mixed(p, neg, small, optional), [p], neg)


def oracle_dump(cf):
    rc, msg, col = O.read_all(cf.file, to_oracle_chunk(cf.chunk))
    assert rc == 0, msg
    return O.dump_column(col)


@POLARITY
@pytest.mark.parametrize("shape", ["s5_small_req", "s5_small_opt", "s5_all_req", "s1"])
def test_decode_and_filter_in_one_call(ctx, shape, neg):
    """decode_regex_async: the armed writer on the small dictionary (payload
    below kArmDictBytes: k_regex_dict, then k_pipe_write tests the match bits,
    no k_pipe_match), decode then scan on the whole one and on S1; flags equal
    the golden and the column equals the oracle's, twice over."""
    small = shape.startswith("s5_small")
    cf = R.s1() if shape == "s1" else R.s5_entries(small, shape.endswith("opt"))
    ref = oracle_dump(cf)
    dc = ctx.upload(cf.file, [to_desc(cf.chunk)])
    try:
        ctx.timing(True)
        ctx.timing_reset()
        dc.decode_regex_async("x", neg)
        dc.regex_pages_result()
        dc.decode_check()
        ctx.timing(False)
        ran = {k: ctx.timing_get(k)[1] for k in COUNTERS + ("pipe_write",)}
        if shape == "s1":
            assert (ran["regex_plain"], ran["regex_dict"], ran["regex_codes"]) == (1, 0, 0), ran
        else:  # (armed, the small dictionary: no separate pass over the codes)
            assert (ran["regex_dict"], ran["pipe_write"], ran["regex_codes"]) == (1, 1, int(not small)), ran
        for p in R.PATTERNS:
            exp = np.array(R.golden_flags(cf, p, neg), dtype=np.uint8)
            for rep in range(2 if p in R.PACKED_PATTERNS else 1):
                dc.decode_regex_async(p, neg)
                got = dc.regex_pages_result()
                dc.decode_check()
                if not np.array_equal(got, exp):
                    bad = np.nonzero(got != exp)[0][:6]
                    pytest.fail(f"{cf.name}: pattern {p!r} neg {neg} pass {rep}: {R.describe(cf, bad)}")
            if p in R.PACKED_PATTERNS:
                assert capi.canonical_dump(dc.to_host()) == ref, (cf.name, p)
    finally:
        ctx.timing(False)
        dc.free()


def counts(ctx, cf, pattern):
    """Launch counts of one scan of `cf`, flags checked."""
    dc = ctx.upload(cf.file, [to_desc(cf.chunk)])
    try:
        ctx.timing(True)
        ctx.timing_reset()
        check(dc, cf, pattern, False)
        return {k: ctx.timing_get(k)[1] for k in COUNTERS}
    finally:
        ctx.timing(False)
        dc.free()


def test_kernels_by_shape(ctx, kernel):
    """Which kernel a shape takes under each setting of the `kernel` fixture:
    each of the five is launched somewhere in this file."""
    def only(c, *names):
        return all((c[k] == 1) == (k in names) and c[k] <= 1 for k in COUNTERS)

    plain = {"window": "regex_plain", "codes": "regex_lanes", "lanes": "regex_lanes", "nfa": "regex_pages"}[kernel]
    for cf, p in ((R.s1(), "[0-9]"), (R.s2(), "[0-9]"), (R.s3("^[a-z]{20}x", False), "^[a-z]{20}x"), (R.s4(), "x$")):
        c = counts(ctx, cf, p)
        assert only(c, plain), (kernel, cf.name, c)
    # pages past the 16-bit window offsets: never the windowed kernel
    c = counts(ctx, R.s4_huge(), "x$")
    assert only(c, "regex_pages" if kernel == "nfa" else "regex_lanes"), (kernel, c)
    # a DFA over its size cap: the NFA kernel under every setting
    c = counts(ctx, R.s1(), R.OVER_CAP[0])
    assert only(c, "regex_pages"), (kernel, c)
    second = {"window": "regex_codes", "codes": "regex_codes", "lanes": "regex_lanes", "nfa": "regex_pages"}[kernel]
    for cf in (R.s5_entries(True, False), R.s5_entries(False, True), R.s5_mixed(r"\x00", False, False, False)):
        c = counts(ctx, cf, r"\x00")
        assert only(c, "regex_dict", second), (kernel, cf.name, c)
