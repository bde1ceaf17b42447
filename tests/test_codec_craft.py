"""CPU: every hand-built stream of tests/codec_craft.py is checked against an
independent decoder (pyarrow's snappy / lz4_raw / zstd, Python's zlib) and
against the host builds of the codec pass's parsers (liblz_check.so,
libzstd_check.so, libgzip_check.so) before tests/test_gpu_codec_streams.py
trusts it as GPU input: valid streams decode to the model's bytes, invalid
ones are refused by both.  The inputs that aim at an edge of k_codec (a far
match at a chosen distance, a header at a window edge, an exact command
count) are proved here to hit it."""
import ctypes as C
import os
import subprocess
import zlib

import pytest

import codec_craft as K
from codec_craft import GZIP, LZ4, LZ4_RAW, SNAPPY, ZSTD

pa = pytest.importorskip("pyarrow")
for _c in ("snappy", "lz4_raw", "zstd"):
    if not pa.Codec.is_available(_c):
        pytest.skip(f"pyarrow without {_c}", allow_module_level=True)

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "duckdb-parquet-parser_amd")
OK, CORRUPT, SIZE = 0, 1, 2


@pytest.fixture(scope="module")
def host():
    libs = {}
    for name in ("lz", "zstd", "gzip"):
        subprocess.run(["make", "-C", PKG, f"pqgpu/lib{name}_check.so"], check=True, stdout=subprocess.DEVNULL)
        libs[name] = C.CDLL(os.path.join(PKG, "pqgpu", f"lib{name}_check.so"))
    return libs


def host_decode(host, case: K.Case):
    """(status, bytes) of the repo's host build of the parser the GPU runs."""
    n = case.n
    out = (C.c_uint8 * (n + 16))()
    ol = C.c_uint32(0)
    if case.codec in (SNAPPY, LZ4, LZ4_RAW):
        rc = host["lz"].lz_decompress(case.codec, case.z, len(case.z), out, n, case.ring, C.byref(ol))
    elif case.codec == ZSTD:
        rc = host["zstd"].zs_decompress(case.z, len(case.z), out, n, C.byref(ol))
    else:
        rc = host["gzip"].gz_decompress(case.z, len(case.z), out, n, C.byref(ol))
    return rc, bytes(out[:ol.value])


def other_decode(case: K.Case) -> bytes:
    """An independent decoder's output (raises when it refuses the stream)."""
    z, n = case.z, case.n
    if case.codec == SNAPPY:
        got = pa.Codec("snappy").decompress(z, decompressed_size=n, asbytes=True)
    elif case.codec == LZ4_RAW:
        got = pa.Codec("lz4_raw").decompress(z, decompressed_size=n, asbytes=True)
    elif case.codec == ZSTD:
        got = pa.Codec("zstd").decompress(z, decompressed_size=n, asbytes=True)
    elif case.codec == LZ4:
        got, p = b"", 0
        while p < len(z):
            if len(z) - p < 8:
                raise ValueError("cut Hadoop block header")
            raw, packed = int.from_bytes(z[p:p + 4], "big"), int.from_bytes(z[p + 4:p + 8], "big")
            if packed > len(z) - p - 8:
                raise ValueError("cut Hadoop block")
            got += pa.Codec("lz4_raw").decompress(z[p + 8:p + 8 + packed], decompressed_size=raw, asbytes=True)
            p += 8 + packed
    else:
        got = b""
        while z:  # members (or one zlib stream), header CRCs and trailers checked
            d = zlib.decompressobj(47)
            got += d.decompress(z)
            if not d.eof:
                raise ValueError("cut DEFLATE stream")
            z = d.unused_data
    if len(got) != n:
        raise ValueError(f"{len(got)} bytes for a page of {n}")
    return got


def prove(host, cases):
    for c in cases:
        if c.raw is not None:
            assert other_decode(c) == c.raw, c
            assert host_decode(host, c) == (OK, c.raw), c
            continue
        rc, got = host_decode(host, c)
        assert rc in (CORRUPT, SIZE, 3) and len(got) <= c.n, (c, rc)
        if c.elsewhere_ok:
            other_decode(c)  # (does not raise)
        else:
            with pytest.raises(Exception):
                other_decode(c)


# ── the writers ────────────────────────────────────────────────────────────
def test_model_overlap_and_history():
    assert K.model([("lit", b"abc"), ("copy", 3, 7), ("copy", 1, 3), ("copy", 10, 2)]) == b"abcabcabcaaaaab"
    assert K.model([("copy", 2, 5)], history=b"xy") == b"xyxyx"


def test_snappy_header_forms(host):
    """Every copy offset size and literal length field size, picked per
    command and as the writer's default."""
    r = K.rnd(70000, seed=1)
    cases = []
    for nb in (0, 1, 2, 3, 4):
        for ob in (1, 2, 4):
            cmds = [("lit", r[:50], nb), ("copy", 33, 9, ob), ("lit", r[50:60], nb), ("copy", 60, 11, ob)]
            z = K.snappy(cmds)
            assert len(z) == 1 + 2 * (1 + nb) + 60 + 2 * (1 + ob)
            cases.append(K.Case(f"snappy-nb{nb}-ob{ob}", SNAPPY, z, K.model(cmds)))
    cmds = [("lit", r[:66000]), ("copy", 65535, 64), ("copy", 66000, 64), ("copy", 1, 500)]
    for off in (None, 4):
        for litlen in (None, 3, 4):
            cases.append(K.Case("snappy-defaults", SNAPPY, K.snappy(cmds, off=off, litlen=litlen), K.model(cmds)))
    prove(host, cases[:-6])
    # (the 66,000 distance is past the GPU's ring: pyarrow takes it, the host build refuses)
    for c in cases[-6:]:
        assert other_decode(c) == c.raw
        assert host_decode(host, c)[0] == CORRUPT
    assert K.queue_commands(cmds, SNAPPY) == 3 + 8  # 500 = 7 * 64 + 52


def test_lz4_length_extensions(host):
    """Literal and match lengths around each 255-byte extension step."""
    r = K.rnd(3000, seed=2)
    cases = []
    for n in (14, 15, 16, 269, 270, 271, 524, 525, 526, 2000):
        cmds = K.pad4([("lit", r[:n]), ("copy", min(n, 7), n + 4)])
        z = K.lz4_block(cmds)
        ext = 0 if n < 15 else 1 + (n - 15) // 255
        assert len(z) == (1 + ext + n + 2 + ext) + 1 + len(cmds[-1][1])
        cases.append(K.Case(f"lz4-len{n}", LZ4_RAW, z, K.model(cmds)))
    prove(host, cases + K.hadoop_cases())


def test_zstd_frames(host):
    assert K.xxh64(b"") == 0xEF46DB3751D8E999 and K.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert K.xxh64(b"abc" * 40) == K.xxh64(memoryview(b"abc" * 40).tobytes())
    cases = K.zstd_frame_cases()
    assert {c.n < 8192 for c in cases} == {True, False}
    prove(host, cases)
    # a frame whose checksum is wrong: refused by zstd (the codec pass skips the field)
    bad = bytearray(K.zstd_frame([("raw", b"checked bytes")], checksum=True))
    bad[-1] ^= 1
    with pytest.raises(Exception):
        pa.Codec("zstd").decompress(bytes(bad), decompressed_size=13, asbytes=True)
    # cut frames and a bad magic
    f = K.zstd_frame([("raw", K.rnd(100)), ("rle", 3, 100)])
    prove(host, [K.Case("zstd-cut", ZSTD, f[:-2], None, n=200), K.Case("zstd-magic", ZSTD, b"\x29" + f[1:], None, n=200),
                 K.Case("zstd-short-page", ZSTD, f, None, n=196)])


def test_deflate_fixed_and_gzip_fields(host):
    r = K.rnd(40000, seed=4)
    cmds = [("lit", r[:32768]), ("copy", 32768, 258), ("copy", 1, 3), ("copy", 32768, 3), ("copy", 259, 258),
            ("lit", bytes(range(256)))]
    raw = K.model(cmds)
    d = K.Deflate().fixed(cmds, final=True).done()
    assert zlib.decompress(d, -15) == raw
    cases = [K.Case("gzip-fixed", GZIP, K.gzip_member(d, raw), raw),
             K.Case("zlib-fixed", GZIP, K.zlib_stream(d, raw), raw)]
    for kw in (dict(extra=b"some extra"), dict(name=b"file.bin"), dict(comment=b"note"), dict(hcrc=True),
               dict(extra=b"\0" * 300, name=b"n", comment=b"c" * 700, hcrc=True)):
        cases.append(K.Case("gzip-" + "+".join(kw), GZIP, K.gzip_member(d, raw, **kw), raw))
    cases.append(K.deflate_far_case())
    prove(host, cases)
    with pytest.raises(Exception):  # zlib checks FHCRC: the writer's is right, a flipped one is not
        h = bytearray(K.gzip_member(d, raw, name=b"x", hcrc=True))
        h[12] ^= 1
        zlib.decompress(bytes(h), 31)


# ── the GPU suite's inputs ─────────────────────────────────────────────────
@pytest.mark.parametrize("codec", [SNAPPY, LZ4_RAW])
@pytest.mark.parametrize("small", [True, False])
def test_window_sweep_streams(host, codec, small):
    """(c) A 5-byte SNAPPY header, or an LZ4 token with its run of 0xFF
    length bytes, starts at every stream offset from W - 24 to W + 8."""
    cases = K.window_cases(codec, small)
    want = {w + k for w in (K.WINDOWS_SMALL if small else K.WINDOWS_FULL) for k in K.SWEEP}
    if codec == LZ4_RAW and small:
        want = {a for a in want if a < 4096}
    for c in cases:
        at = int(c.name.split("@")[1])
        assert (c.n < 8192) == small
        if codec == SNAPPY:
            tag = c.z[at]
            assert tag == (63 << 2) if "lit5" in c.name else tag & 3 == 3, c
        else:
            assert c.z[at] == 0xFF and c.z[at + 1] == 0xFF
    assert {int(c.name.split("@")[1]) for c in cases} == want
    prove(host, cases)


@pytest.mark.parametrize("codec", [SNAPPY, LZ4_RAW])
def test_queue_shape_streams(host, codec):
    """(d) Exact command counts (counted_cmds asserts them), both layouts."""
    cases = K.queue_cases(codec)
    for n in K.QUEUE_COUNTS:
        assert K.queue_commands(K.counted_cmds(n, codec), codec) == n
        assert K.queue_commands(K.counted_cmds(n, codec, 9000), codec) == n
    assert sum(c.n < 8192 for c in cases) >= 8 and sum(c.n >= 8192 for c in cases) >= 9
    prove(host, cases)


@pytest.mark.parametrize("codec", [SNAPPY, LZ4_RAW])
def test_far_copy_streams(host, codec):
    """(e) Crafted distances at the ring's limit; (g) the first reachable byte."""
    prove(host, K.far_lz_cases(codec) + list(K.reach_cases(codec)))
    if codec == SNAPPY:
        prove(host, [K.snappy_past_ring()])


def test_far_matches_are_found(host, capsys):
    """(e) The compressor found the one match of R + filler + R: it saved all
    of R but a few bytes of sequence coding.  snappy and zlib do not find
    these matches (their far cases are the crafted ones)."""
    saved = {}
    for case, rlen in K.zstd_far_cases():
        saved[case.name] = len(case.raw) - len(case.z)
        assert saved[case.name] >= rlen - 64, (case, saved[case.name])
    # LZ4 spends a length byte per 255 literal bytes (257 for the 65,535 in
    # front of the match), so the size alone cannot meet that bound: the
    # block is parsed instead, and holds the match itself
    case, rlen = K.lz4_far_case()
    saved[case.name] = len(case.raw) - len(case.z)
    seqs = K.lz4_parse(case.z)
    assert [(d, m >= rlen - 64) for _, d, m in seqs if d] == [(65535, True)], seqs
    assert saved[case.name] >= rlen - 64 - (len(case.raw) + 254) // 255
    with capsys.disabled():
        small = [v for k, v in saved.items() if k.startswith("zstd") and int(k.split("far")[1].split("-")[0]) < 8192]
        full = [v for k, v in saved.items() if k.startswith("zstd") and int(k.split("far")[1].split("-")[0]) > 8192]
        print(f"\nsaved: zstd small {min(small)}-{max(small)} of 600, zstd full {min(full)}-{max(full)} of 4000, "
              f"lz4_raw 65535 {saved['lz4-pyarrow-far65535']} of 4000")
    prove(host, [c for c, _ in K.zstd_far_cases()] + [K.lz4_far_case()[0]])
    for codec, z in (("snappy", pa.Codec("snappy").compress(K.far_input(65535, 4000), asbytes=True)),
                     ("zlib", zlib.compress(K.far_input(32768, 4000), 9))):
        assert len(z) > len(K.far_input(32768, 4000)) - 1000, codec


def test_zstd_literal_tail_shape(host):
    """(e) Several blocks, the first with Huffman-coded literals, and the far
    match found (against the same input with a random end)."""
    case = K.zstd_tail_case()
    blocks = K.zstd_blocks(case.z)
    assert len(blocks) >= 2 and blocks[0][0] == 2 and blocks[0][2] == 2, blocks
    raw, plain = K.zstd_tail_input()
    zp = pa.Codec("zstd", compression_level=3).compress(plain, asbytes=True)
    assert len(zp) - len(case.z) >= 4000 - 64
    prove(host, [case])


def test_gzip_crc_streams(host):
    """(f) and the CRC twins."""
    cases = K.gzip_crc_cases()
    assert [c.n for c in cases[:len(K.GZ_LENGTHS)]] == list(K.GZ_LENGTHS)
    stored = next(c for c in cases if c.name == "gzip-stored-200000")
    assert (stored.z[10] >> 1) & 3 == 0  # a stored block opens the member
    prove(host, cases + K.gzip_crc_twins())


def test_damaged_streams(host):
    """(h)"""
    prove(host, K.damaged_cases())
