"""Crafted strings for the regex page kernels (test helper, not collected).

The generator's values are lowercase words of 1-44 bytes; this corpus holds
what they never do: digits, upper case, controls, NUL, 2/3/4-byte UTF-8,
lengths 0-257 around every 16-byte block edge, and per-pattern near misses.
Everything is deterministic (random.Random with a fixed seed).

Golden: `re.compile(p, re.ASCII).search(value.decode())` per value; a page is
reported (flag 1) iff no non-null value satisfies (match != neg).  The values
of a crafted file are known by construction (`Crafted.pages`), so no decoder
takes part in the golden.

No corpus value ends in "\\n": Python's `$` also matches before a final
newline, this project's `$` is `\\Z` (regex.hpp).  That divergence has its own
known-answer file (`kat_dollar`), whose expectation is the contract, not `re`.
"""
from __future__ import annotations

import random
import re
from dataclasses import dataclass
from functools import lru_cache

import pqbuild as B

BYTE_ARRAY = 6
SEED = 20250117

# ── patterns, by the table form the CPU test asserts ───────────────────────
FULL_UNANCHORED = ["[0-9]", "[^a-z ]", r"\d+\s", r"\w\W", r"\S\s\S", ".", "a.c", "[^x]y", r"\x00", r"a\x00b",
                   "[A-Z][a-z]+", "é", "é.$", r"\n", r"\t|\v|\f|\r", "x", "x$", r"\s$", ".{19}x"]
FULL_ANCHORED = ["^x", "^.$", "^.{3}$", r"^\w+$", "^[^q]+$", "^.{16}$", "^[a-z]{20}x", "^[a-z]{59}x"]
CLASS_TABLE = [".{20}x", "^[a-z]{60}x", "x[a-z]{6}$", "x.{5}$"]
OVER_CAP = ["x.{10}$"]
TRIVIAL = ["x*", "^$", "$"]
NONTRIVIAL = FULL_UNANCHORED + FULL_ANCHORED + CLASS_TABLE + OVER_CAP
PATTERNS = NONTRIVIAL + TRIVIAL
# S3 / the mixed dictionary pages: one pattern per group plus \x00 ("^$" is
# the one trivial pattern both polarities of which some value fails)
PACKED_PATTERNS = ["[A-Z][a-z]+", "^[a-z]{20}x", ".{20}x", "x.{10}$", "^$", r"\x00"]
# S4
LONG_PATTERNS = ["x$", "^x", "x", r"\x00", "^[a-z]{20}x", ".{20}x"]

ALPHABET = list("abcxyzq \t\n\r\x0b\x0c\x00\x01\x7fAZ09_-.") + ["é", "ß", "€", "日", "😀", "\u0080", "\u07ff", "\u0800"]
RANDOM_LENGTHS = list(range(71)) + [127, 128, 129, 255, 256, 257]
RUN_LENGTHS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def _hand() -> list[str]:
    """Positives and near misses per pattern; an anchored pattern's near miss
    is one byte wrong at or after byte 16."""
    a, v = "a", []
    # ^[a-z]{20}x, ^[a-z]{59}x, ^[a-z]{60}x: the x, and the byte before it
    for n in (20, 59, 60):
        v += [a * n + "x", a * n + "x" + "tail Z9", "q" * n + "x\x00", "abcxyzq" * 9 + "x",
              ("abcxyzq" * 9)[:n] + "x" + "é", "z" * n + "xx", a * (n - 1) + "bx" + " x", a * 16 + "z" * (n - 16) + "x",
              a * (n - 1) + "A" + "x", a * (n - 1) + "\x00" + "x", a * n + "X", a * n + "y" + "x", a * 16 + "0" + a * (n - 17) + "x",
              a * 17 + " " + a * (n - 18) + "x", a * (n - 1) + "é" + "x", a * n + "\nx", a * 15 + "_" + a * (n - 16) + "x",
              a * (n - 1) + "x"]
    # .{19}x / .{20}x: code points, not bytes; a newline breaks the run
    for n in (19, 20):
        v += ["é" * n + "x", "日" * n + "x", "😀" * n + "x", a * n + "x", "\x00" * n + "x", "q" * 40 + "x",
              "\n" + "b" * n + "x" + "\nzz", "Z9_-." * 4 + "x",
              a * (n - 1) + "x", "é" * (n - 1) + "x", a * (n - 1) + "\n" + "x", (a * (n - 1) + "\n") * 3 + "x",
              "日" * (n - 1) + "\n" + "x", a * 10 + "\n" + a * (n - 1) + "x", "x" + a * 30, "😀" * (n - 1) + "x" + a * 20]
    # ^.{16}$: 16 code points of 16, 17 and 40 bytes; 15 and 17 code points
    v += [a * 16, a * 15 + "é", "abcxyzq AZ09_-.\x00", "日" * 8 + a * 8, "\x00" * 16, "😀" * 4 + "€" * 8 + a * 4,
          "\t\r\x0b\x0c" * 4, "é" * 16, "😀" * 16,
          a * 15, a * 17, "\n" + a * 15, "é" * 15, "é" * 17, a * 8 + "\n" + a * 7, "日" * 15, "😀" * 17, a * 16 + "\x00"]
    # ^.$ / ^.{3}$
    v += ["é", "日", "😀", "\x00", "\x7f", "Z", "\u0080", "\u07ff", "\u0800", "é日😀", "\x00\x00\x00", "a\tb", "€€€", "_-.", "😀😀😀",
          "a\nb", "\n\n\nq", "éé", "日日日日", "\x00\x00", "a\na", "😀😀", "ab\nc", "\nab"]
    # x[a-z]{6}$, x.{5}$, x.{10}$: counted from the end
    for n, cls in ((6, "lower"), (5, "dot"), (10, "dot")):
        tails = ["abcxyz"[:n].ljust(n, "q"), "z" * n, "q" * n, ("yx" * n)[:n]]
        if cls == "dot":
            tails += [("é日😀\x00 \t_9" * 2)[:n], "😀" * n, "\x00" * n, ("A\r" * n)[:n]]
        else:
            tails += [("xyzabc" * 2)[:n], ("bcq" * n)[:n], "x" * n, ("cab" * n)[:n]]
        for t in tails:
            v += ["x" + t, a * 20 + "x" + t, "é\nx" + t]
        for t in tails[:4]:   # one short, one long, one wrong inside the tail (at or after byte 16)
            v += ["x" + t[:-1], "x" + t + "a", a * 20 + "x" + t[:2] + ("\n" if cls == "dot" else "A") + t[3:]]
    # é, é.$, a\x00b, a.c, [^x]y, \d+\s, \w\W, \S\s\S, [A-Z][a-z]+, \s$, x$
    v += ["é", "éa", "aaéz", "a" * 15 + "éq", "a" * 16 + "é日", "é😀", "\x00é\x00", "éé", "ééé", "\né", "Ã", "©a", "é\nq", "aé", "a" * 15 + "é",
          "a\x00b", "a" * 15 + "\x00b", "aa\x00bb", "\x00a\x00b\x00", "a\x00\x00b", "a\x01b", "a b", "a\x00B", "A\x00b", "ab\x00",
          "a\x00b" * 3, "éa\x00b", "a" * 16 + "\x00b", "a\x00ba\x00b", "\na\x00b\nq", "", "",   # ("": with the six random ones, 8 values "." fails)
          "a\x00c", "aéc", "a日c", "a😀c", "abc", "a" * 15 + "bc", "a\nc", "ac", "a\n\nc", "aéé", "a😀",
          "ay", "xay", "\x00y", "éy", "\ny", "xy", "y", "xxy", "yx", "xyxy",
          "9 ", "09\t", "a0\n.", "x99\r9", "5\x0b5", "0\x0c", "9a ", "9", "9_ ", "9\x00 ", "9é ",
          "a ", "_\x00", "Z-", "9é", "a\x7f", "0.", "aZ09_", "é ", "  ", "\x00\x00", "_", "az_",
          "a b", "\x00\tA", "é\n日", ".\r.", "\x01\x0c\x7f", "a  b", " a ", "ab", "\t\t\t", " \n ",
          "Za", "aaZaa", "AZq", "日Zz!", "0Ab", "ZA", "Z", "Zé", "aZ", "Z\x00a", "zZ",
          "a ", "a\t", "a\r", "a\x0b", "a\x0c", "é ", "a" * 15 + " ", "a" * 16 + "\t", "a \x00", " a", "a\x01", "a\x1c", "a\u0080",
          "x", "ax", "a" * 15 + "x", "a" * 16 + "x", "a" * 17 + "x", "éx", "\x00x", "x\nx", "xa", "x\x00", "x ", "x\nq", "X", "xé"]
    # \n and the other space controls inside a value
    v += ["a\nb", "\nq", "a" * 15 + "\nb", "a" * 16 + "\nb", "\n\nq", "é\nq", "\x00\n\x00", "q\n\n\nq",
          "a\tb", "a\rb", "a\x0bb", "a\x0cb", "a" * 16 + "\x0c", "\r", "\x0b" * 17, "é\t"]
    # ^\w+$ / ^[^q]+$: wrong at or after byte 16
    v += ["aZ09_" * 4, "_" * 16, "a" * 33, "Z" * 17, "0" * 64, "az_AZ09" * 3, "q" * 16, "x" * 48,
          "a" * 16 + "-", "a" * 16 + "é", "a" * 17 + " ", "a" * 20 + "\x00", "a" * 31 + ".", "a" * 16 + "\na", "a" * 47 + "\x7f", "_" * 16 + "日",
          "a" * 16 + "q", "é" * 9 + "q", "\x00" * 17 + "q", "a" * 31 + "q" + "a", "A" * 63 + "q", " " * 16 + "q ", "日" * 6 + "q", "-" * 32 + "q"]
    return v


@lru_cache(maxsize=None)
def corpus() -> tuple[bytes, ...]:
    rng = random.Random(SEED)
    vals: list[str] = []
    for n in RANDOM_LENGTHS:
        for _ in range(6):
            s = [rng.choice(ALPHABET) for _ in range(n)]
            while s and s[-1] == "\n":
                s[-1] = rng.choice(ALPHABET)
            vals.append("".join(s))
    for fill in ("a", "\x00"):
        for n in RUN_LENGTHS:
            vals += [fill * (n - 1) + "x", "x" + fill * (n - 1), fill * n]
    vals += _hand()
    assert not any(s.endswith("\n") for s in vals)
    return tuple(s.encode("utf-8") for s in vals)


@lru_cache(maxsize=None)
def _rx(pattern: str):
    return re.compile(pattern, re.ASCII)


@lru_cache(maxsize=None)
def match(pattern: str, value: bytes) -> bool:
    return _rx(pattern).search(value.decode("utf-8")) is not None


# ── crafted files ──────────────────────────────────────────────────────────
@dataclass
class Crafted:
    name: str
    file: bytes
    chunk: dict
    pages: list      # per data page: its rows, bytes or None (NULL)
    deciding: list | None = None   # S3: per page (rank, payload offset of the value's first byte) or None
    kat: dict | None = None        # known answers {(pattern, neg): flags}, not derived from re

    @property
    def num_rows(self) -> int:
        return sum(len(p) for p in self.pages)


def golden_flags(cf: Crafted, pattern: str, neg: bool) -> list[int]:
    if cf.kat is not None:
        return list(cf.kat[(pattern, neg)])
    return [0 if any(v is not None and match(pattern, v) != neg for v in rows) else 1 for rows in cf.pages]


def _plain_page(vals) -> bytes:
    pay = B.plain_ba(vals)
    return B.data_header(len(pay), len(vals), 0) + pay


def _required_plain(name: str, pages: list, **kw) -> Crafted:
    f, ch = B.build_file([_plain_page(p) for p in pages], BYTE_ARRAY, False, sum(len(p) for p in pages))
    return Crafted(name, f, ch, [list(p) for p in pages], **kw)


@lru_cache(maxsize=None)
def s1() -> Crafted:
    """REQUIRED PLAIN, every corpus value its own page."""
    return _required_plain("s1", [[v] for v in corpus()])


@lru_cache(maxsize=None)
def kat_dollar() -> Crafted:
    """`$` is \\Z: "x\\n" does not match x$ (Python's re would say it does)."""
    return _required_plain("kat_dollar", [[b"x\n"], [b"x"]], kat={("x$", False): [1, 0], ("x$", True): [0, 1]})


@lru_cache(maxsize=None)
def s2() -> Crafted:
    """OPTIONAL PLAIN: pages of [NULL, v, NULL], def levels RLE and bit-packed
    in turn; every 9th page is all NULL (reported under both polarities)."""
    blobs, pages = [], []
    for i, v in enumerate(corpus()):
        if i % 9 == 4:
            pay = B.levels_section(B.rle(3, 0, 1) if i % 2 else B.bitpack([0, 0, 0], 1))
            blobs.append(B.data_header(len(pay), 3, 0) + pay)
            pages.append([None, None, None])
        lv = B.rle(1, 0, 1) + B.rle(1, 1, 1) + B.rle(1, 0, 1) if i % 2 == 0 else B.bitpack([0, 1, 0], 1)
        pay = B.levels_section(lv) + B.plain_ba([v])
        blobs.append(B.data_header(len(pay), 3, 0) + pay)
        pages.append([None, v, None])
    f, ch = B.build_file(blobs, BYTE_ARRAY, True, 3 * len(pages))
    return Crafted("s2", f, ch, pages)


# S3 ------------------------------------------------------------------------
PAGE_VALUES = 600
DECIDING_RANKS = [0, 63, 64, 255, 256, 257, 599]   # 256 = k_regex_plain's batch (4 strings x 64 lanes)
ALIGN_RANK0 = 130                                  # the 16 alignment pages: ranks 130..145 (third string of a lane)
BATCH = 256


def fillers_for(pattern: str, neg: bool, cap: int = 48, least: int = 16) -> list[bytes]:
    """Corpus values that do not satisfy the predicate, the short ones."""
    ok = sorted({v for v in corpus() if match(pattern, v) == neg}, key=lambda v: (len(v), v))
    short = [v for v in ok if len(v) <= cap]
    return short if len(short) >= least else ok[:least]


def deciders_for(pattern: str, neg: bool) -> list[bytes]:
    """Corpus values that satisfy it: short and long, in a fixed order."""
    ok = sorted({v for v in corpus() if match(pattern, v) != neg}, key=lambda v: (len(v), v))
    step = max(1, len(ok) // 24)
    return ok[::step]


def _lead_for_residue(rng, fillers, count: int, residue: int):
    """`count` leading fillers after which the next value's first byte sits at
    payload offset = residue (mod 16), or None when their lengths cannot."""
    free = min(count, 15)
    lead = [rng.choice(fillers) for _ in range(count - free)]
    base = sum(4 + len(v) for v in lead) + 4
    by_res = {}
    for v in fillers:
        by_res.setdefault((4 + len(v)) % 16, v)
    reach = [{base % 16: []}]
    for _ in range(free):
        nxt = {}
        for r, path in reach[-1].items():
            for d, v in by_res.items():
                nxt.setdefault((r + d) % 16, path + [v])
        reach.append(nxt)
    tail = reach[free].get(residue)
    return None if tail is None else lead + tail


@lru_cache(maxsize=None)
def s3(pattern: str, neg: bool) -> Crafted:
    """REQUIRED PLAIN pages of 600 values: fillers that do not satisfy the
    predicate plus one deciding value at a chosen rank / start residue, and
    control pages without one."""
    rng = random.Random(f"{SEED} s3 {pattern} {neg}")
    fil, dec = fillers_for(pattern, neg), deciders_for(pattern, neg)
    pages, deciding = [], []

    def page(lead, d):
        rest = [rng.choice(fil) for _ in range(PAGE_VALUES - len(lead) - 1)]
        pages.append(lead + [d] + rest)
        deciding.append((len(lead), sum(4 + len(v) for v in lead) + 4))

    for i, r in enumerate(DECIDING_RANKS):
        page([rng.choice(fil) for _ in range(r)], dec[(3 * i) % len(dec)])
        if i % 3 == 1:
            pages.append([rng.choice(fil) for _ in range(PAGE_VALUES)])
            deciding.append(None)
    for k in range(16):
        lead = _lead_for_residue(rng, fil, ALIGN_RANK0 + k, k)
        if lead is None:   # (filler lengths that cannot reach k: the page still has its deciding value)
            lead = [rng.choice(fil) for _ in range(ALIGN_RANK0 + k)]
        page(lead, dec[(5 * k + 1) % len(dec)])
    pages.append([rng.choice(fil) for _ in range(PAGE_VALUES)])
    deciding.append(None)
    return _required_plain(f"s3[{pattern!r},{'notlike' if neg else 'like'}]", pages, deciding=deciding)


def plain_windows(cf: Crafted, regex_win: int) -> list[tuple[int, int]]:
    """(first page, pages) of the windowed kernel's windows for a REQUIRED
    PLAIN crafted file, by plan.cpp's rule: page slots (payload rounded up to
    16, plus 16) lie back to back; a window takes consecutive pages while
    they fit max(regex_win, largest slot) bytes, 64 at the most."""
    slot = [(sum(4 + len(v) for v in p) + 15) // 16 * 16 + 16 for p in cf.pages]
    win = max(regex_win, max(slot))
    out, p = [], 0
    while p < len(slot):
        q, used = p, 0
        while q < len(slot) and q - p < 64 and used + slot[q] <= win:
            used += slot[q]
            q += 1
        out.append((p, q - p))
        p = q
    return out


def batch_ranks(cf: Crafted, regex_win: int) -> set[int]:
    """Which of a lane's four interleaved strings (k_regex_plain: string g of
    a window is string (g % 256) // 64 of lane g % 64) the deciding values are."""
    got = set()
    for p0, n in plain_windows(cf, regex_win):
        g0 = 0
        for p in range(p0, p0 + n):
            if cf.deciding[p] is not None:
                got.add(((g0 + cf.deciding[p][0]) % BATCH) // 64)
            g0 += len(cf.pages[p])
    return got


# S4 ------------------------------------------------------------------------
LONG_LENGTHS = [1000, 4000, 8100, 20000]
HUGE = 70000


def long_values(n: int) -> list[bytes]:
    """n-byte values: the deciding byte first, last, and at bytes 15, 16 and
    17 of a late 16-byte block."""
    late = (n - 40) // 16 * 16
    spots = [0, n - 1, late + 15, late + 16, late + 17]
    out = [b"a" * n]
    for ch in (b"x", b"\x00"):
        out += [b"a" * k + ch + b"a" * (n - k - 1) for k in spots]
    out += [b"a" * 20 + b"x" + b"a" * (n - 21), b"a" * 19 + b"Ax" + b"a" * (n - 21), b"a" * 19 + b"x" + b"a" * (n - 20),
            b"a" * 16 + b"\x00" + b"aaax" + b"a" * (n - 21)]
    body = (b"a" * 19 + b"\n") * (n // 20)
    out += [body[:n - 1] + b"x",                                    # <= 19 code points before every x
            body[:n - 22] + b"\n" + b"a" * 20 + b"x"]               # 20 before the last one
    assert all(len(v) == n for v in out)
    return out


@lru_cache(maxsize=None)
def s4() -> Crafted:
    return _required_plain("s4", [[v] for n in LONG_LENGTHS for v in long_values(n)])


@lru_cache(maxsize=None)
def s4_huge() -> Crafted:
    """70,000-byte values, one per page (past the windowed kernel's u16
    offsets: the chunk takes k_regex_lanes), among 1,000-byte pages."""
    big = [b"a" * (HUGE - 1) + b"x", b"a" * (HUGE - 1000 + 16) + b"\x00" + b"a" * (1000 - 17),
           b"a" * 20 + b"x" + b"a" * (HUGE - 21), b"a" * HUGE, b"x" + b"a" * (HUGE - 1)]
    small = long_values(1000)
    pages = [[v] for v in small[:8]] + [[v] for v in big] + [[v] for v in small[8:]]
    return _required_plain("s4_huge", pages)


# S5 ------------------------------------------------------------------------
ARM_DICT_BYTES = 32768   # kernels.hpp kArmDictBytes


@lru_cache(maxsize=None)
def dict_entries(small: bool) -> tuple[bytes, ...]:
    """The corpus as dictionary entries; small: its short values, a payload
    below the armed one-pass filter's limit."""
    if not small:
        return corpus()
    out = tuple(v for v in corpus() if len(v) <= 72)   # (every pattern still has matching entries)
    assert sum(4 + len(v) for v in out) < ARM_DICT_BYTES
    return out


def _dict_page(entries) -> bytes:
    pay = B.plain_ba(entries)
    return B.dict_header(len(pay), len(entries)) + pay


def _index_page(stream: bytes, bw: int, defs):
    """A dictionary-encoded data page: defs None (REQUIRED) or the def
    levels.  Returns (payload, rows or None)."""
    pay = bytes([bw]) + stream
    n = None
    if defs is not None:
        n = len(defs)
        run = all(d == defs[0] for d in defs)
        pay = B.levels_section(B.rle(n, defs[0], 1) if run else B.bitpack(defs, 1)) + pay
    return pay, n


def _dict_file(name: str, entries, pages_idx: list, optional: bool, packed: bool) -> Crafted:
    """pages_idx: per page its indices (one per non-null row).  RLE runs when
    every index of a page is the same and not `packed`, else bit-packed."""
    bw = max(1, (len(entries) - 1).bit_length())
    blobs, pages = [_dict_page(entries)], []
    for i, idx in enumerate(pages_idx):
        if optional:
            # a NULL before every third value, and one at the end of odd pages
            defs = []
            for k in range(len(idx)):
                if k % 3 == 1:
                    defs.append(0)
                defs.append(1)
            if i % 2:
                defs.append(0)
            if i % 5 == 0:
                defs = [1] * len(idx)   # an RLE def run
        else:
            defs = None
        stream = B.bitpack(idx, bw) if packed or len(set(idx)) > 1 else B.rle(len(idx), idx[0], bw)
        pay, n = _index_page(stream, bw, defs)
        nvals = len(idx) if n is None else n
        blobs.append(B.data_header(len(pay), nvals, 8) + pay)
        it = iter(idx)
        pages.append([entries[next(it)] for _ in idx] if defs is None else [entries[next(it)] if d else None for d in defs])
    f, ch = B.build_file(blobs, BYTE_ARRAY, optional, sum(len(p) for p in pages), dict_at_start=True)
    return Crafted(name, f, ch, pages)


@lru_cache(maxsize=None)
def s5_entries(small: bool, optional: bool) -> Crafted:
    """Per entry one data page of 8 values, an RLE run of its index: the
    page's flag is that entry's result."""
    ent = dict_entries(small)
    return _dict_file(f"s5_entries[{'small' if small else 'all'},{'opt' if optional else 'req'}]", ent,
                      [[k] * 8 for k in range(len(ent))], optional, False)


@lru_cache(maxsize=None)
def s5_mixed(pattern: str, neg: bool, small: bool, optional: bool) -> Crafted:
    """Bit-packed pages of 24 indices: fillers that do not satisfy the
    predicate and one deciding index, at every position of the first group,
    both edges of the others; control pages without one."""
    rng = random.Random(f"{SEED} s5 {pattern} {neg} {small} {optional}")
    ent = dict_entries(small)
    fil = [k for k, v in enumerate(ent) if match(pattern, v) == neg]
    dec = [k for k, v in enumerate(ent) if match(pattern, v) != neg]
    assert fil and dec, (pattern, neg, small)
    pages = []
    for i, at in enumerate([0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 23]):
        idx = [rng.choice(fil) for _ in range(24)]
        idx[at] = dec[(7 * i) % len(dec)]
        pages.append(idx)
        if i % 4 == 2:
            pages.append([rng.choice(fil) for _ in range(24)])
    return _dict_file(f"s5_mixed[{pattern!r},{'notlike' if neg else 'like'},{'small' if small else 'all'},"
                      f"{'opt' if optional else 'req'}]", ent, pages, optional, True)


def describe(cf: Crafted, pages) -> str:
    return "; ".join(f"page {int(p)}: {[v if v is None or len(v) <= 80 else v[:40] + b'...' + v[-40:] for v in cf.pages[int(p)]][:6]!r}"
                     for p in pages)
