"""GPU: compressed streams through the codec pass (csrc/kernels/codec.hip,
k_codec), bit for bit against the bytes that were compressed.  The streams are
the corpora of the host parser tests and the hand-built cases of
tests/codec_craft.py, which tests/test_codec_craft.py proves on the CPU (an
independent decoder and the host builds agree on every one, and each case that
aims at an edge of the kernel hits it).  They reach what only the GPU runs: the
staged input windows and the header bytes held in registers, the parser and
executor waves and their queue, the output ring's wrap, flushes and last
masked store, ZSTD's literal storage in the slot's tail and its far matches
read back from the slot, the CRC-32 fold, and the switch between the small and
the full layout at 8192 bytes.

A payload rides in a REQUIRED PLAIN column (pqbuild.carrier): the decoded
column is the payload itself (INT32) or its bits (BOOLEAN).  Small cases are
pages of one chunk and one upload."""
import functools
import gzip
import struct
import zlib

import numpy as np
import pytest

import codec_craft as K
import pqbuild as B
from codec_craft import GZIP, LZ4, LZ4_RAW, SNAPPY, ZSTD, Case
from pqgpu import capi
from util import to_desc

pa = pytest.importorskip("pyarrow")
for _c in ("snappy", "lz4_raw", "zstd"):
    if not pa.Codec.is_available(_c):
        pytest.skip(f"pyarrow without {_c}", allow_module_level=True)

pytestmark = pytest.mark.gpu
ERR_DECOMPRESS = -9
ERR_STATUS = (-9, -2, -8)


# ── pages, chunks, comparison ──────────────────────────────────────────────
def chunk_file(cases, codec: int, lead: bytes = b""):
    """One chunk with a V1 page per case: (file, chunk descriptor, INT32?)."""
    int32 = all(c.n % 4 == 0 for c in cases)
    pages, total = [], 0
    for c in cases:
        ptype, nvals = B.carrier(c.n) if int32 else (capi.BOOLEAN, 8 * c.n)
        pages.append(B.data_header(len(c.z), nvals, usize=c.n) + c.z)
        total += nvals
    f, ch = B.build_file(pages, capi.INT32 if int32 else capi.BOOLEAN, False, total, codec=codec, lead=lead)
    d = to_desc(ch)
    d.ext_flags = capi.EXT_CODECS | capi.EXT_PAGE_V2
    return f, d, int32


def decode(ctx, f, d):
    dc = ctx.upload(f, [d])
    try:
        dc.decode()
        return dc.to_host()
    finally:
        dc.free()


def check(ctx, cases, codec: int, lead: bytes = b""):
    """Every case's page decodes to its bytes."""
    assert cases and all(c.raw is not None and c.codec == codec for c in cases)
    f, d, int32 = chunk_file(cases, codec, lead)
    h = decode(ctx, f, d)
    assert h.validity.all()
    got = h.data.tobytes()
    at = 0
    for c in cases:
        exp = c.raw if int32 else np.unpackbits(np.frombuffer(c.raw, np.uint8), bitorder="little").tobytes()
        part = got[at:at + len(exp)]
        if part != exp:
            a, b = np.frombuffer(part, np.uint8), np.frombuffer(exp, np.uint8)
            k = len(b) if len(a) != len(b) else int(np.nonzero(a != b)[0][0]) // (1 if int32 else 8)
            raise AssertionError(f"{c}: first wrong byte {k} of {c.n}")
        at += len(exp)
    assert at == len(got)
    return len(cases)


def refused(ctx, case: Case, codes=(ERR_DECOMPRESS,)):
    """The page ends in an error of the codec pass, never in data."""
    f, d, _ = chunk_file([case], case.codec)
    with pytest.raises(capi.PqError) as ei:
        decode(ctx, f, d)
    assert ei.value.code in codes, (case, ei.value)


def hadoop(raw: bytes, block: int) -> bytes:
    c = pa.Codec("lz4_raw")
    out = b""
    for i in range(0, max(len(raw), 1), block):
        z = c.compress(raw[i:i + block], asbytes=True)
        out += struct.pack(">II", len(raw[i:i + block]), len(z)) + z
    return out


def zstream(d: bytes, level: int, strategy: int, wbits: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(d) + c.flush()


# ── a. corpus parity ───────────────────────────────────────────────────────
@functools.lru_cache(maxsize=None)
def corpus() -> tuple[bytes, ...]:
    """The inputs of the three host parser tests without their 1.5 MB and
    2.4 MB items, each once, zero-padded to a multiple of 4 bytes."""
    import test_gzip_host
    import test_lz_host
    import test_zstd_host
    seen, out = set(), []
    for mod in (test_lz_host, test_gzip_host, test_zstd_host):
        for d in mod.inputs():
            if len(d) in (1_500_000, 2_400_000):
                continue
            d += b"\0" * (-len(d) % 4)
            if d not in seen:
                seen.add(d)
                out.append(d)
    assert len(out) >= 12
    return tuple(out)


def halves(d: bytes, f) -> bytes:
    return f(d[:len(d) // 2]) + f(d[len(d) // 2:])


def _zstd(level):
    return lambda d: pa.Codec("zstd", compression_level=level).compress(d, asbytes=True)


WRITERS = {
    "snappy": (SNAPPY, lambda d: pa.Codec("snappy").compress(d, asbytes=True)),
    "lz4_raw": (LZ4_RAW, lambda d: pa.Codec("lz4_raw").compress(d, asbytes=True)),
    "hadoop-4k": (LZ4, lambda d: hadoop(d, 4096)),
    "hadoop-64k": (LZ4, lambda d: hadoop(d, 65536)),
    "gzip-2-members": (GZIP, lambda d: halves(d, lambda x: gzip.compress(x, mtime=0))),
    "zstd-2-frames": (ZSTD, lambda d: halves(d, _zstd(3))),
}
for _lv in (0, 1, 6, 9):
    WRITERS[f"gzip-l{_lv}"] = (GZIP, lambda d, lv=_lv: zstream(d, lv, zlib.Z_DEFAULT_STRATEGY, 31))
    WRITERS[f"zlib-l{_lv}"] = (GZIP, lambda d, lv=_lv: zstream(d, lv, zlib.Z_DEFAULT_STRATEGY, 15))
for _nm, _st in (("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE), ("filtered", zlib.Z_FILTERED)):
    WRITERS[f"gzip-{_nm}"] = (GZIP, lambda d, st=_st: zstream(d, 6, st, 31))
    WRITERS[f"zlib-{_nm}"] = (GZIP, lambda d, st=_st: zstream(d, 6, st, 15))
for _lv in (-5, 1, 3, 9, 19):
    WRITERS[f"zstd-l{_lv}"] = (ZSTD, _zstd(_lv))


@pytest.mark.parametrize("writer", sorted(WRITERS))
def test_corpus_parity(ctx, writer):
    codec, f = WRITERS[writer]
    check(ctx, [Case(f"{writer}[{i}]", codec, f(d), d) for i, d in enumerate(corpus())], codec)


def test_crafted_zstd_frames(ctx):
    """Raw and RLE blocks, skippable frames, the checksum flag, single-segment
    and window-descriptor frames, several frames in a page (both layouts)."""
    check(ctx, K.zstd_frame_cases(), ZSTD)


def test_crafted_hadoop_blocks(ctx):
    check(ctx, K.hadoop_cases(), LZ4)


# ── b. output-side sizes ───────────────────────────────────────────────────
SIZES = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 32767, 32768, 32769, 65535, 65536, 65537)
SIZE_WRITERS = {"snappy": WRITERS["snappy"], "lz4_raw": WRITERS["lz4_raw"], "lz4": WRITERS["hadoop-4k"],
                "gzip": (GZIP, lambda d: gzip.compress(d, mtime=0)), "zstd": WRITERS["zstd-l3"]}


@pytest.mark.parametrize("writer", sorted(SIZE_WRITERS))
def test_output_sizes(ctx, writer):
    """Every output length around the flush size, the layout switch and each
    ring size, and every residue of the last 16-byte store: a compressible and
    an incompressible page of each, back to back, the shortest last but one."""
    codec, f = SIZE_WRITERS[writer]
    t, r = K.text(70000, seed=51), K.rnd(70000, seed=53)
    cases = [Case(f"{writer}-{kind}{n}", codec, f(src[:n]), src[:n])
             for n in SIZES for kind, src in (("text", t), ("random", r))]
    shortest = cases.pop(0)
    cases.insert(len(cases) - 1, shortest)
    assert cases[-2].n == 1 and len(cases) == 2 * len(SIZES)
    check(ctx, cases, codec)


# ── c. input-side alignment and window edges ───────────────────────────────
@pytest.mark.parametrize("writer", sorted(SIZE_WRITERS))
def test_payload_alignment(ctx, writer):
    """A payload that starts at every address mod 16, in both layouts (the
    staged window starts at the payload address rounded down to 16)."""
    codec, f = SIZE_WRITERS[writer]
    t = K.text(16000, seed=55)
    small, full = Case("small", codec, f(t[:3000]), t[:3000]), Case("full", codec, f(t[3000:15000]), t[3000:15000])
    seen = {"small": set(), "full": set()}
    for order in ((small, full), (full, small)):
        for lead in range(16):
            fb, d, _ = chunk_file(order, codec, lead=b"\xa5" * lead)
            rc, _, table = capi.build_page_table(fb, d)
            assert rc == 0 and len(table) == 2
            seen[order[0].name].add(table[0].payload_offset % 16)
            seen[order[1].name].add(table[1].payload_offset % 16)
            check(ctx, list(order), codec, lead=b"\xa5" * lead)
    assert seen["small"] == set(range(16)) and seen["full"] == set(range(16))


@pytest.mark.parametrize("small", [True, False], ids=["small", "full"])
@pytest.mark.parametrize("codec", [SNAPPY, LZ4_RAW], ids=["snappy", "lz4"])
def test_headers_at_window_edges(ctx, codec, small):
    """5-byte SNAPPY headers and LZ4 tokens with long runs of 0xFF length
    bytes that start at every stream offset from W - 24 to W + 8 for the
    window sizes 1024, 2048 and 8192."""
    check(ctx, K.window_cases(codec, small), codec)


# ── d. queue shapes ────────────────────────────────────────────────────────
@pytest.mark.parametrize("codec", [SNAPPY, LZ4_RAW], ids=["snappy", "lz4"])
def test_queue_shapes(ctx, codec):
    """Exact command counts around the 64-command group and the 256-command
    queue, literal-only streams, a long slow command behind a full queue, fast
    and slow commands in turn (overlapping copies of every distance under 64)."""
    check(ctx, K.queue_cases(codec), codec)


# ── e. far copies per ring ─────────────────────────────────────────────────
@pytest.mark.parametrize("codec", [SNAPPY, LZ4_RAW], ids=["snappy", "lz4"])
def test_far_copies_64k_ring(ctx, codec):
    cases = K.far_lz_cases(codec)
    if codec == LZ4_RAW:
        cases.append(K.lz4_far_case()[0])
    check(ctx, cases, codec)


def test_snappy_copy_past_ring_is_refused(ctx):
    """A copy from 70,000 back: valid SNAPPY that the 64 KiB ring cannot serve."""
    refused(ctx, K.snappy_past_ring())


def test_deflate_far_match_across_wrap(ctx):
    check(ctx, [K.deflate_far_case()], GZIP)


def test_zstd_far_matches(ctx):
    """One match at a chosen distance on both sides of the slot read-back
    threshold (ring - 2 KiB: 6144 and 30720), levels 1, 3 and 19."""
    cases = [c for c, _ in K.zstd_far_cases()]
    assert len(cases) == 30
    check(ctx, cases, ZSTD)


def test_zstd_far_match_into_former_literal_tail(ctx):
    check(ctx, [K.zstd_tail_case()], ZSTD)


# ── f. GZIP CRC ────────────────────────────────────────────────────────────
def test_gzip_crc_lengths(ctx):
    """Members of 1..130 bytes and around the fold threshold (64512), a stored
    member of 200,000, later members that start mid-ring, header fields."""
    assert check(ctx, K.gzip_crc_cases(), GZIP) == len(K.GZ_LENGTHS) + 4


@pytest.mark.parametrize("k", range(4))
def test_gzip_crc_bit_flip_is_refused(ctx, k):
    refused(ctx, K.gzip_crc_twins()[k])


# ── g. V2 prologue ─────────────────────────────────────────────────────────
def v2_chunk(codec: int, z: bytes, values: bytes):
    """An OPTIONAL INT32 DATA_PAGE_V2 page: every fifth row null, the values'
    bytes compressed as z.  (file, descriptor, validity)."""
    nv = len(values) // 4
    valid = []
    while sum(valid) < nv:
        valid.append(int(len(valid) % 5 != 0))
    levels = B.bitpack(valid, 1)
    page = B.data_header_v2(len(levels) + len(z), len(valid), len(levels) + len(values), def_len=len(levels),
                            num_nulls=len(valid) - nv, is_compressed=True) + levels + z
    f, ch = B.build_file([page], capi.INT32, True, len(valid), codec=codec)
    d = to_desc(ch)
    d.ext_flags = capi.EXT_CODECS | capi.EXT_PAGE_V2
    return f, d, np.array(valid, np.uint8)


@pytest.mark.parametrize("codec", [SNAPPY, LZ4_RAW, ZSTD], ids=["snappy", "lz4", "zstd"])
def test_v2_page_with_def_levels(ctx, codec):
    """The values start behind the level section: a copy may reach the first
    value byte and no farther."""
    if codec == ZSTD:
        raw = K.text(6000, seed=57)
        good, over = Case("zstd-v2", ZSTD, pa.Codec("zstd").compress(raw, asbytes=True), raw), None
    else:
        good, over = K.reach_cases(codec)
    f, d, valid = v2_chunk(codec, good.z, good.raw)
    h = decode(ctx, f, d)
    assert np.array_equal(h.validity, valid)
    got = np.frombuffer(h.data.tobytes(), "<i4")[valid == 1]
    assert np.array_equal(got, np.frombuffer(good.raw, "<i4"))
    if over is not None:
        f, d, _ = v2_chunk(codec, over.z, b"\0" * over.n)
        with pytest.raises(capi.PqError) as ei:
            decode(ctx, f, d)
        assert ei.value.code == ERR_DECOMPRESS


# ── h. status, not data ────────────────────────────────────────────────────
DAMAGED = K.damaged_cases() + [K.reach_cases(SNAPPY)[1], K.reach_cases(LZ4_RAW)[1]]


@pytest.mark.parametrize("case", DAMAGED, ids=[c.name for c in DAMAGED])
def test_damaged_stream_ends_in_status(ctx, case):
    refused(ctx, case, ERR_STATUS)
