"""Hand-built compressed streams for the codec pass (test input only, pure
Python): SNAPPY and LZ4 from an explicit command list, ZSTD frames of the
shapes that need no entropy coder, fixed-Huffman and stored DEFLATE blocks,
GZIP members with every optional header field; and the named case lists the
CPU suite proves (tests/test_codec_craft.py) before the GPU suite decodes them
(tests/test_gpu_codec_streams.py).

A command list is [("lit", bytes) | ("copy", dist, n)].  model() executes it
in plain Python and gives the bytes every decoder must produce.  A command may
carry one more field that picks its header form: ("lit", bytes, nb) with nb
the bytes of SNAPPY's literal length field (0: in the tag), ("copy", dist, n,
ob) with ob the bytes of SNAPPY's copy offset (1, 2 or 4)."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SNAPPY, GZIP, LZ4, ZSTD, LZ4_RAW = 1, 2, 5, 6, 7  # parquet.thrift CompressionCodec


# ── the model ──────────────────────────────────────────────────────────────
def model(cmds, history: bytes = b"") -> bytes:
    """The bytes the commands produce (after `history`, which is not returned)."""
    out = bytearray(history)
    for c in cmds:
        if c[0] == "lit":
            out += c[1]
            continue
        d, n = c[1], c[2]
        assert 1 <= d <= len(out), (d, len(out))
        if d >= n:
            out += out[len(out) - d:len(out) - d + n]
        else:  # overlapping: the last d bytes repeat
            pat = bytes(out[len(out) - d:])
            out += (pat * (n // d + 1))[:n]
    return bytes(out[len(history):])


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


# ── SNAPPY (format_description.txt) ────────────────────────────────────────
def snappy_lit(b: bytes, nb: int | None = None) -> bytes:
    n = len(b)
    assert n >= 1
    if nb is None:
        nb = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
    if nb == 0:
        assert n <= 60
        return bytes([(n - 1) << 2]) + b
    assert n - 1 < 1 << (8 * nb)
    return bytes([(59 + nb) << 2]) + (n - 1).to_bytes(nb, "little") + b


def snappy_copy(d: int, n: int, ob: int | None = None) -> bytes:
    """One copy element (n <= 64; 4..11 and d < 2048 for a 1-byte offset)."""
    if ob is None:
        ob = 1 if 4 <= n <= 11 and d < 2048 else (2 if d < 65536 else 4)
    if ob == 1:
        assert 4 <= n <= 11 and d < 2048
        return bytes([1 | ((n - 4) << 2) | ((d >> 8) << 5), d & 0xFF])
    assert 1 <= n <= 64
    if ob == 2:
        assert d < 65536
        return bytes([2 | ((n - 1) << 2)]) + struct.pack("<H", d)
    return bytes([3 | ((n - 1) << 2)]) + struct.pack("<I", d)


def snappy_elements(cmds, off: int | None = None, litlen: int | None = None) -> list[bytes]:
    """The elements of the stream, one per command; a copy longer than 64
    bytes (the format's limit) becomes several.  off / litlen: the default
    offset / literal length field sizes of commands that name none."""
    out = []
    for c in cmds:
        if c[0] == "lit":
            out.append(snappy_lit(c[1], c[2] if len(c) > 2 else litlen))
            continue
        d, n = c[1], c[2]
        ob = c[3] if len(c) > 3 else off
        while n > 64:
            # (keep the rest >= 4 so a 1-byte-offset form stays possible)
            k = 64 if n - 64 >= 4 or n == 64 else 60
            out.append(snappy_copy(d, k, ob if ob != 1 else 2))
            n -= k
        out.append(snappy_copy(d, n, ob))
    return out


def snappy(cmds, off: int | None = None, litlen: int | None = None, ulen: int | None = None) -> bytes:
    body = b"".join(snappy_elements(cmds, off, litlen))
    return varint(len(model(cmds)) if ulen is None else ulen) + body


# ── LZ4 (lz4_Block_format.md) ──────────────────────────────────────────────
def _lz4_len(n: int) -> bytes:
    """Extension bytes of a length whose token nibble is 15 (n >= 15)."""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def lz4_sequence(lit: bytes, d: int | None, n: int = 0) -> bytes:
    """One sequence: literals, then (d not None) a match of n >= 4 from d."""
    ll = len(lit)
    ml = n - 4 if d is not None else 0
    assert d is None or (n >= 4 and 1 <= d <= 65535)
    tok = (min(ll, 15) << 4) | min(ml, 15)
    out = bytes([tok]) + (_lz4_len(ll) if ll >= 15 else b"") + lit
    if d is not None:
        out += struct.pack("<H", d) + (_lz4_len(ml) if ml >= 15 else b"")
    return out


def lz4_sequences(cmds) -> list[bytes]:
    """Adjacent literals join into one sequence; the block ends on a
    literal-only sequence (empty when the commands end on a copy)."""
    out, lit = [], b""
    for c in cmds:
        if c[0] == "lit":
            lit += c[1]
        else:
            out.append(lz4_sequence(lit, c[1], c[2]))
            lit = b""
    out.append(lz4_sequence(lit, None))
    return out


def lz4_block(cmds) -> bytes:
    return b"".join(lz4_sequences(cmds))


def lz4_parse(z: bytes) -> list[tuple[int, int, int]]:
    """(literal bytes, distance, match bytes) of a block's sequences (0, 0 in
    the last, which has no match)."""
    out, p = [], 0
    while True:
        tok = z[p]
        p += 1
        n = tok >> 4
        if n == 15:
            while z[p] == 255:
                n += 255
                p += 1
            n += z[p]
            p += 1
        p += n
        if p == len(z):
            out.append((n, 0, 0))
            return out
        d = z[p] | (z[p + 1] << 8)
        p += 2
        m = tok & 15
        if m == 15:
            while z[p] == 255:
                m += 255
                p += 1
            m += z[p]
            p += 1
        out.append((n, d, m + 4))


def lz4_hadoop(blocks) -> bytes:
    """Hadoop's framing over several blocks, each with its own command list
    (a block's copies stay inside the block): [u32 BE raw][u32 BE packed][block]."""
    out = b""
    for cmds in blocks:
        z = lz4_block(cmds)
        out += struct.pack(">II", len(model(cmds)), len(z)) + z
    return out


def queue_commands(cmds, codec: int) -> int:
    """Commands the parser queues for the stream the writer emits: SNAPPY one
    per element; LZ4 one per non-empty literal run and one per match."""
    if codec == SNAPPY:
        return len(snappy_elements(cmds))
    n, lit = 0, False
    for c in cmds:
        if c[0] == "lit":
            lit = lit or len(c[1]) > 0
        else:
            n += 1 + lit
            lit = False
    return n + lit


# ── ZSTD frames without an entropy coder (RFC 8878) ────────────────────────
_M64 = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = (11400714785074694791, 14029467366897019727, 1609587929392839161,
                           9650029242287828579, 2870177450012600261)


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M64


def _round(acc, v):
    return (_rotl((acc + v * _P2) & _M64, 31) * _P1) & _M64


def _merge(h, v):
    return (((h ^ _round(0, v)) * _P1) + _P4) & _M64


def xxh64(b: bytes, seed: int = 0) -> int:
    """XXH64 (the frame's content checksum is its low 32 bits)."""
    n, p = len(b), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M64, (seed + _P2) & _M64, seed, (seed - _P1) & _M64]
        words = struct.unpack_from("<%dQ" % (n // 32 * 4), b)
        for k in range(0, len(words), 4):
            v[0] = _round(v[0], words[k])
            v[1] = _round(v[1], words[k + 1])
            v[2] = _round(v[2], words[k + 2])
            v[3] = _round(v[3], words[k + 3])
        p = n // 32 * 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M64
        for x in v:
            h = _merge(h, x)
    else:
        h = (seed + _P5) & _M64
    h = (h + n) & _M64
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", b, p)[0]), 27) * _P1 + _P4) & _M64
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", b, p)[0] * _P1 & _M64), 23) * _P2 + _P3) & _M64
        p += 4
    while p < n:
        h = (_rotl(h ^ (b[p] * _P5 & _M64), 11) * _P1) & _M64
        p += 1
    h = ((h ^ (h >> 33)) * _P2) & _M64
    h = ((h ^ (h >> 29)) * _P3) & _M64
    return h ^ (h >> 32)


ZSTD_BLOCK_MAX = 1 << 17


def zstd_frame(blocks, single: bool = True, checksum: bool = False, window_log: int = 20) -> bytes:
    """blocks: [("raw", bytes) | ("rle", byte value, count)], each at most 128
    KiB.  single: a single-segment frame (the content size, no window
    descriptor); otherwise a window descriptor of 2^window_log and no content
    size."""
    content = b"".join(b[1] if b[0] == "raw" else bytes([b[1]]) * b[2] for b in blocks)
    n = len(content)
    out = bytearray(b"\x28\xb5\x2f\xfd")
    ck = 4 if checksum else 0
    if single:
        if n < 256:
            out += bytes([0x20 | ck, n])
        elif n < 65536 + 256:
            out += bytes([0x60 | ck]) + struct.pack("<H", n - 256)
        else:
            out += bytes([0xA0 | ck]) + struct.pack("<I", n)
    else:
        assert 10 <= window_log <= 30 and all((b[2] if b[0] == "rle" else len(b[1])) <= 1 << window_log for b in blocks)
        out += bytes([ck, (window_log - 10) << 3])
    assert blocks
    for k, b in enumerate(blocks):
        last = int(k == len(blocks) - 1)
        if b[0] == "raw":
            assert len(b[1]) <= ZSTD_BLOCK_MAX
            out += (last | (0 << 1) | (len(b[1]) << 3)).to_bytes(3, "little") + b[1]
        else:
            assert 1 <= b[2] <= ZSTD_BLOCK_MAX
            out += (last | (1 << 1) | (b[2] << 3)).to_bytes(3, "little") + bytes([b[1]])
    if checksum:
        out += struct.pack("<I", xxh64(content) & 0xFFFFFFFF)
    return bytes(out)


def zstd_content(blocks) -> bytes:
    return b"".join(b[1] if b[0] == "raw" else bytes([b[1]]) * b[2] for b in blocks)


def zstd_skippable(data: bytes, nibble: int = 0) -> bytes:
    return struct.pack("<II", 0x184D2A50 | nibble, len(data)) + data


# ── DEFLATE: stored and fixed-Huffman blocks (RFC 1951) ────────────────────
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
             227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
              4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _rev(v: int, n: int) -> int:
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def _fixed_litlen(sym: int) -> tuple[int, int]:
    """(code reversed for an LSB-first writer, bits) of RFC 1951 3.2.6."""
    if sym < 144:
        return _rev(0x30 + sym, 8), 8
    if sym < 256:
        return _rev(0x190 + sym - 144, 9), 9
    if sym < 280:
        return _rev(sym - 256, 7), 7
    return _rev(0xC0 + sym - 280, 8), 8


_FIXED = [_fixed_litlen(s) for s in range(288)]
_FDIST = [_rev(s, 5) for s in range(30)]


class Deflate:
    """A raw DEFLATE stream, block by block.  The last block added with
    final=True ends the stream."""

    def __init__(self):
        self.acc = 0
        self.n = 0
        self.out = bytearray()

    def _put(self, v: int, nb: int):
        self.acc |= v << self.n
        self.n += nb
        if self.n >= 64:
            k = self.n // 8
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def _align(self):
        k = (self.n + 7) // 8
        self.out += self.acc.to_bytes(k, "little") if k else b""
        self.acc = self.n = 0

    def stored(self, data: bytes, final: bool = False):
        assert len(data) <= 65535
        self._put(int(final), 1)
        self._put(0, 2)
        self._align()
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data
        return self

    def fixed(self, cmds, final: bool = False):
        """Literal and match symbols of the fixed code; a copy is one match
        (3 <= n <= 258, 1 <= dist <= 32768)."""
        self._put(int(final), 1)
        self._put(1, 2)
        for c in cmds:
            if c[0] == "lit":
                for b in c[1]:
                    self._put(*_FIXED[b])
                continue
            d, n = c[1], c[2]
            assert 3 <= n <= 258 and 1 <= d <= 32768
            ls = max(k for k in range(29) if _LEN_BASE[k] <= n) if n < 258 else 28
            self._put(*_FIXED[257 + ls])
            if _LEN_EXTRA[ls]:
                self._put(n - _LEN_BASE[ls], _LEN_EXTRA[ls])
            ds = max(k for k in range(30) if _DIST_BASE[k] <= d)
            self._put(_FDIST[ds], 5)
            if _DIST_EXTRA[ds]:
                self._put(d - _DIST_BASE[ds], _DIST_EXTRA[ds])
        self._put(*_FIXED[256])
        return self

    def done(self) -> bytes:
        self._align()
        return bytes(self.out)


def gzip_member(raw_deflate: bytes, data: bytes, crc: int | None = None, extra: bytes | None = None,
                name: bytes | None = None, comment: bytes | None = None, hcrc: bool = False) -> bytes:
    """An RFC 1952 member around a raw DEFLATE stream, with any of FEXTRA,
    FNAME, FCOMMENT and FHCRC.  crc: the trailer's CRC-32 when it is to differ
    from the data's."""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | \
          (2 if hcrc else 0)
    h = bytes([0x1F, 0x8B, 8, flg]) + b"\0\0\0\0\0\xff"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    c = zlib.crc32(data) if crc is None else crc
    return h + raw_deflate + struct.pack("<II", c & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def zlib_stream(raw_deflate: bytes, data: bytes) -> bytes:
    return b"\x78\x01" + raw_deflate + struct.pack(">I", zlib.adler32(data))


def raw_deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


# ── test data ──────────────────────────────────────────────────────────────
def rnd(n: int, seed: int = 3) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text(n: int, seed: int = 3) -> bytes:
    """Compressible bytes (words; Huffman-coded literals and short matches)."""
    rng = np.random.default_rng(seed)
    words = [b"carefully ", b"quickly ", b"special ", b"requests ", b"the ", b"final ", b"deposits ", b"of ", b"x"]
    out = b"".join(words[i] for i in rng.integers(0, len(words), n // 4 + 8))
    return out[:n]


# ── named cases (proved on the CPU, then decoded on the GPU) ───────────────
class Case:
    """One page payload.  raw: the bytes it must decode to; None: it must be
    refused.  ring: the history the layout that takes it has (the host
    build's argument).  elsewhere_ok: a stream other decoders accept and the
    codec pass refuses by design (a distance past its ring)."""

    def __init__(self, name: str, codec: int, z: bytes, raw: bytes | None, n: int | None = None,
                 elsewhere_ok: bool = False, zlib_framed: bool = False):
        self.name, self.codec, self.z, self.raw = name, codec, z, raw
        self.n = len(raw) if n is None else n  # the page's uncompressed size
        self.elsewhere_ok = elsewhere_ok
        self.zlib_framed = zlib_framed

    @property
    def ring(self) -> int:
        return 8192 if self.n < 8192 else 65536

    def __repr__(self):
        return f"Case({self.name}, codec {self.codec}, {len(self.z)} -> {self.n})"


def lz_case(name: str, codec: int, cmds, **kw) -> Case:
    """The command list as one SNAPPY stream or one LZ4 block."""
    raw = model(cmds)
    z = snappy(cmds, **kw) if codec == SNAPPY else lz4_block(cmds)
    return Case(name, codec, z, raw)


def pad4(cmds, fill: bytes = b"0123456789abcdef") -> list:
    """The commands plus a last literal of 12..15 bytes that makes the output
    a multiple of 4 bytes (an INT32 page) and ends an LZ4 block as the format
    asks (the last match ends 12 or more bytes before the end)."""
    n = len(model(cmds))
    return list(cmds) + [("lit", fill[:12 + (-(n + 12)) % 4])]


# (c) multi-byte headers at the edges of the staged input windows
WINDOWS_FULL, WINDOWS_SMALL = (1024, 2048, 8192), (1024, 2048, 8192)
SWEEP = range(-24, 9)  # header offsets relative to the window size


def sweep_snappy(kind: str, at: int, small: bool) -> Case:
    """A 5-byte header (kind "lit5": a literal tag with a 4-byte length;
    "copy5": a copy with a 4-byte offset) that starts at stream offset `at`,
    behind filler commands; then a few commands more, which a parse that lost
    its place would misread.  Every header byte that can be other than zero
    in a page this size is: a literal of 0x0101 + 1 bytes (0x010101 + 1 in the
    full layout), a distance of 0x0125 (0x2525): a byte read as zero, as the
    bytes behind the staged window are, shows.  small: under 8192 bytes of
    output (a filler past 4 KiB is then 1-byte copies with 4-byte offsets: 5
    stream bytes per output byte)."""
    r = rnd(80000, seed=at)
    for pre in (2, 3):  # the length preamble's size depends on the total
        room = at - pre
        if small and at > 4096:
            k = (room - 9) // 5       # 5-byte copies after a first literal
            first = room - 5 * k - 1  # a literal with an in-tag length: 1 + first bytes
            assert 4 <= first <= 60
            cmds = [("lit", r[:first], 0)] + [("copy", 1 + j % first, 1, 4) for j in range(k)]
        elif small:
            cmds = [("lit", r[:room - 3], 2)]  # tag + 2 length bytes + the bytes
        else:  # (160 copies of 64 bytes: the history the far distance needs)
            cmds = [("lit", r[:room - 3 - 3 * 160], 2)] + [("copy", 60, 64, 2)] * 160
        assert sum(map(len, snappy_elements(cmds))) == room
        if kind == "lit5":
            cmds.append(("lit", r[10000:10000 + (0x0101 if small else 0x010101) + 1], 4))
        else:
            cmds.append(("copy", 0x0125 if small else 0x2525, 20, 4))
        cmds += [("lit", b"sync"), ("copy", 9, 30, 2), ("lit", r[9100:9130]), ("copy", 50, 11, 1)]
        cmds = pad4(cmds)
        raw = model(cmds)
        if len(varint(len(raw))) == pre:
            assert (len(raw) < 8192) == small
            z = snappy(cmds)
            assert all(z[at + 1:at + (3 if small or kind == "copy5" else 4)]) and z[at + 4] == 0
            return Case(f"snappy-{kind}@{at}", SNAPPY, z, raw)
    raise AssertionError("no preamble size fits")


def sweep_lz4(at: int, small: bool) -> Case:
    """A sequence whose token starts at block offset `at` and is followed by
    20 literal-length 0xFF bytes and later by 20 match-length 0xFF bytes (10
    and 10 where the page is to stay under 8192 bytes: 20 and 20 alone make
    10,234), behind one filler sequence."""
    r = rnd(16384, seed=at + 7)
    n = next(k for k in range(at) if len(lz4_sequence(r[:k], 5, 4)) == at)
    ff = 10 if small else 20
    cmds = [("lit", r[:n]), ("copy", 5, 4),
            ("lit", r[n:n + 15 + 255 * ff + 7]), ("copy", 1000, 4 + 15 + 255 * ff + 3),
            ("lit", b"sync"), ("copy", 9, 30)]
    cmds = pad4(cmds)
    z = lz4_block(cmds)
    assert z[at] == 0xFF and z[at + 1:at + 2 + ff] == b"\xff" * ff + b"\x07"
    m = at + 2 + ff + (15 + 255 * ff + 7) + 2  # behind the literals and the offset
    assert z[m:m + ff + 1] == b"\xff" * ff + b"\x03"
    raw = model(cmds)
    assert (len(raw) < 8192) == small, len(raw)
    return Case(f"lz4-ext@{at}", LZ4_RAW, z, raw)


def window_cases(codec: int, small: bool) -> list[Case]:
    out = []
    for w in (WINDOWS_SMALL if small else WINDOWS_FULL):
        for k in SWEEP:
            if codec == SNAPPY:
                out += [sweep_snappy("lit5", w + k, small), sweep_snappy("copy5", w + k, small)]
            elif not (small and w == 8192):  # (8 KiB of LZ4 input gives more than 8 KiB of output)
                out.append(sweep_lz4(w + k, small))
    return out


# (d) queue shapes
def counted_cmds(n: int, codec: int, first: int = 24) -> list:
    """A stream of exactly n queue commands, every one after the first
    literal (of `first` bytes) a single wave step (at most 60 bytes), literals
    and copies mixed."""
    r = rnd(70000, seed=n)
    if n == 1:
        return [("lit", r[:first + 16])]
    cmds, q, at = [("lit", r[:first])], 1, first
    tail = 1  # the last literal (LZ4 needs it; SNAPPY gets it too)
    k = 0
    while q < n - tail:
        k += 1
        if k % 3 == 0 and q + 2 <= n - tail:  # a literal and a copy
            ln = 1 + k % 50
            cmds += [("lit", r[at:at + ln]), ("copy", 1 + k % 20, 4 + k % 50)]
            at += ln
            q += 2
        else:
            cmds.append(("copy", 4 + k % 21, 4 + (7 * k) % 57))
            q += 1
    cmds.append(("lit", r[at:at + 12 + (-(len(model(cmds)) + 12)) % 4]))
    assert queue_commands(cmds, codec) == n, (queue_commands(cmds, codec), n)
    return cmds


QUEUE_COUNTS = (1, 63, 64, 65, 129, 255, 256, 257, 1000)


def short_cmds(k: int, codec: int, seed: int) -> list:
    """k one-step commands of the fewest bytes the format has: SNAPPY 1-byte
    literals and 1-byte copies; LZ4 a 1-byte literal and a 4-byte match."""
    r = rnd(k + 16, seed)
    out = []
    for j in range(k // 2):
        out += [("lit", r[j:j + 1]), ("copy", 3 + j % 5, 1 if codec == SNAPPY else 4)]
    return out


def queue_cases(codec: int) -> list[Case]:
    nm = "snappy" if codec == SNAPPY else "lz4"
    out = [lz_case(f"{nm}-{n}cmds", codec, counted_cmds(n, codec)) for n in QUEUE_COUNTS]
    # (the same counts in the full layout: a first literal of 9000 bytes)
    out += [lz_case(f"{nm}-{n}cmds-full", codec, counted_cmds(n, codec, 9000)) for n in QUEUE_COUNTS]
    r = rnd(300000, seed=11)
    if codec == SNAPPY:  # literals only, every length-field size
        lits, at = [], 0
        for j in range(200):
            ln = (1, 60, 61, 64, 65, 255, 256, 257, 700)[j % 9]
            lits.append(("lit", r[at:at + ln]))
            at += ln
        lits.append(("lit", r[at:at + 70000]))
        out.append(lz_case("snappy-literals-only", codec, pad4(lits)))
    else:
        out.append(lz_case("lz4-literal-only", codec, [("lit", r[:5000])]))
    # a full queue in front of a long slow command
    head = [("lit", r[:16])] + short_cmds(300, codec, 5)
    out.append(lz_case(f"{nm}-300+copy200000+300", codec,
                       pad4(head + [("copy", 1, 200000)] + short_cmds(300, codec, 6))))
    out.append(lz_case(f"{nm}-300+lit200000+300", codec,
                       pad4(head + [("lit", r[1000:201000])] + short_cmds(300, codec, 6))))
    # fast and slow commands in turn
    alt = [("lit", r[:200])]
    for n in (64, 65):
        alt += [("copy", n, n), ("lit", b"xy"), ("copy", n - 1, n), ("lit", b"z"), ("copy", 200, n), ("copy", 7, 5)]
    for d in range(1, 64):
        for n in ((1, 63, 64, 65, 200) if codec == SNAPPY else (4, 63, 64, 65, 200)):
            alt += [("copy", d, n), ("lit", r[d * n:d * n + 1 + d % 3])]
    out.append(lz_case(f"{nm}-fast-slow", codec, pad4(alt)))
    return out


# (e) far copies
def far_lz_cases(codec: int) -> list[Case]:
    """Distances at the 64 KiB ring's limit, and copies whose source or
    destination crosses the ring's wrap (output offset 65536), each as one
    wave step (one command of the fast path) and as a long command."""
    nm = "snappy" if codec == SNAPPY else "lz4"
    r = rnd(200000, seed=13)
    out = []
    for d in (65535, 65534, 32768):
        for n in (64, 200):
            out.append(lz_case(f"{nm}-far{d}x{n}", codec, pad4([("lit", r[:d + 90]), ("copy", d, n), ("copy", d, 13)])))
    for n in (64, 200):
        out.append(lz_case(f"{nm}-wrap-dst-x{n}", codec,
                           pad4([("lit", r[:65536 - 30]), ("copy", 100, n), ("lit", r[:40000 - n]),
                                 ("copy", 40000, n),   # the source crosses the wrap
                                 ("lit", r[:65535 - n - 30]), ("copy", 65535, n)])))
    return out


def snappy_past_ring() -> Case:
    """A valid SNAPPY stream the 64 KiB ring cannot serve: a copy from 70,000 back."""
    r = rnd(70100, seed=17)
    cmds = pad4([("lit", r), ("copy", 70000, 32, 4)])
    return Case("snappy-far70000", SNAPPY, snappy(cmds), None, n=len(model(cmds)), elsewhere_ok=True)


def deflate_far_case() -> Case:
    """DEFLATE's longest match (258) from its farthest distance (32,768),
    once with the destination and once with the source across the 64 KiB
    ring's wrap; stored blocks carry the history."""
    r = rnd(100000, seed=19)
    a, b = 65536 - 100, 98304 - 100
    cmds = [("lit", r[:a]), ("copy", 32768, 258), ("lit", r[a:a + (b - a - 258)]), ("copy", 32768, 258),
            ("copy", 32768, 3), ("lit", b"end.")]
    raw = model(cmds)
    d = Deflate().stored(r[:40000]).stored(r[40000:a]).fixed(cmds[1:2])
    d.stored(cmds[2][1]).fixed(cmds[3:], final=True)
    return Case("deflate-32768x258", GZIP, gzip_member(d.done(), raw), raw)


ZSTD_FAR_SMALL, ZSTD_FAR_FULL, ZSTD_FAR_LEVELS = (6000, 6143, 6144, 6900), (30719, 30720, 32767, 32768, 65536, 400000), (1, 3, 19)


def far_input(dist: int, rlen: int, seed: int = 3) -> bytes:
    """R + random filler + R with the second R exactly `dist` after the first."""
    g = np.random.default_rng(seed)
    R = g.integers(0, 256, rlen).astype(np.uint8).tobytes()
    return R + g.integers(0, 256, dist - rlen).astype(np.uint8).tobytes() + R


def zstd_far_cases() -> list[tuple[Case, int]]:
    """(case, len(R)): pyarrow's zstd on far_input; the only match lies at the
    chosen distance, around the slot read-back threshold of each layout."""
    import pyarrow as pa
    out = []
    for dists, rlen in ((ZSTD_FAR_SMALL, 600), (ZSTD_FAR_FULL, 4000)):
        for d in dists:
            raw = far_input(d, rlen)
            for lv in ZSTD_FAR_LEVELS:
                z = pa.Codec("zstd", compression_level=lv).compress(raw, asbytes=True)
                out.append((Case(f"zstd-far{d}-l{lv}", ZSTD, z, raw), rlen))
    return out


def lz4_far_case() -> tuple[Case, int]:
    import pyarrow as pa
    raw = far_input(65535, 4000)
    return Case("lz4-pyarrow-far65535", LZ4_RAW, pa.Codec("lz4_raw").compress(raw, asbytes=True), raw), 4000


def skewed(n: int, seed: int = 23) -> bytes:
    """Bytes of 64 values with a skewed distribution: Huffman shortens them,
    matches are rare (literal-heavy blocks)."""
    g = np.random.default_rng(seed)
    return np.minimum(g.geometric(0.08, n), 64).astype(np.uint8).tobytes()


def zstd_tail_input() -> tuple[bytes, bytes]:
    """(input, the input with its last 4000 bytes random): a first block of
    128 KiB of Huffman-coded literals, which the decoder parks in the slot's
    tail, 40,000 random bytes, then the first block's last 4000 bytes again,
    44,000 after their first place: a far match into bytes that were literal
    storage before the output overwrote them."""
    t = skewed(131072)
    mid = rnd(40000, seed=29)
    return t + mid + t[-4000:], t + mid + rnd(4000, seed=31)


def zstd_blocks(z: bytes) -> list[tuple[int, int, int]]:
    """(block type, block size, literals type) of a frame's blocks (literals
    type -1 outside compressed blocks)."""
    assert z[:4] == b"\x28\xb5\x2f\xfd"
    fhd = z[4]
    p = 5 + (0 if fhd & 0x20 else 1) + (0, 1, 2, 4)[fhd & 3]
    p += (1 if fhd & 0x20 else 0, 2, 4, 8)[fhd >> 6]
    out = []
    while True:
        bh = int.from_bytes(z[p:p + 3], "little")
        bt, bs = (bh >> 1) & 3, bh >> 3
        out.append((bt, bs, z[p + 3] & 3 if bt == 2 else -1))
        p += 3 + (1 if bt == 1 else bs)
        if bh & 1:
            return out


def zstd_tail_case(level: int = 3) -> Case:
    import pyarrow as pa
    raw, _ = zstd_tail_input()
    return Case(f"zstd-literal-tail-l{level}", ZSTD, pa.Codec("zstd", compression_level=level).compress(raw, asbytes=True), raw)


def zstd_frame_cases() -> list[Case]:
    """Frames that need no entropy coder: raw and RLE blocks, a skippable
    frame, the content-checksum flag, single-segment frames and frames with a
    window descriptor, several frames in one page."""
    r = rnd(300000, seed=37)
    out = []

    def add(name, z, raw):
        out.append(Case("zstd-" + name, ZSTD, z, raw))
    for n in (1, 255, 256, 5000, 65791, 65792, 131072):  # every content-size field width
        add(f"raw{n}", zstd_frame([("raw", r[:n])]), r[:n])
    bl = [("raw", r[:1000]), ("rle", 7, 5000), ("raw", r[1000:1003]), ("rle", 0, 1), ("rle", 255, 131072),
          ("raw", r[2000:2000 + 131072]), ("rle", 9, 70000)]
    c = zstd_content(bl)
    add("raw+rle", zstd_frame(bl), c)
    add("raw+rle-checksum", zstd_frame(bl, checksum=True), c)
    add("raw+rle-window", zstd_frame(bl, single=False, window_log=17), c)
    add("raw+rle-window-checksum", zstd_frame(bl, single=False, window_log=22, checksum=True), c)
    small = [("rle", 65, 100), ("raw", r[:700]), ("rle", 66, 3000)]
    sc = zstd_content(small)
    add("small-window", zstd_frame(small, single=False, window_log=10 + 3), sc)
    add("skippable-first", zstd_skippable(b"skip me") + zstd_frame(small), sc)
    add("skippable-between", zstd_frame(small, checksum=True) + zstd_skippable(r[:300], 7) + zstd_frame(bl, single=False),
        sc + c)
    add("three-frames", zstd_frame([("raw", r[:9000])]) + zstd_frame(small, single=False) + zstd_frame([("rle", 1, 40000)], checksum=True),
        r[:9000] + sc + b"\x01" * 40000)
    add("skippable-last", zstd_frame(small) + zstd_skippable(b""), sc)
    return out


# (f) GZIP members and their CRC-32
GZ_LENGTHS = tuple(range(1, 131)) + (4095, 4096, 64511, 64512, 64513, 65536, 200000)


def gzip_crc_cases() -> list[Case]:
    import gzip
    t = text(200000, seed=41)
    out = [Case(f"gzip-{n}", GZIP, gzip.compress(t[:n], mtime=0), t[:n]) for n in GZ_LENGTHS]
    out.append(Case("gzip-stored-200000", GZIP, gzip.compress(t, compresslevel=0, mtime=0), t))
    # later members start mid-ring (the ring position carries over, the CRC does not)
    a, b, c = t[:40000], t[50000:50000 + 70001], t[130000:130000 + 33333]
    out.append(Case("gzip-2-members", GZIP, gzip.compress(a, mtime=0) + gzip.compress(b, 1, mtime=0), a + b))
    out.append(Case("gzip-3-members", GZIP, gzip.compress(a, 9, mtime=0) + gzip.compress(b, 0, mtime=0) + gzip.compress(c, mtime=0),
                    a + b + c))
    out.append(Case("gzip-header-fields", GZIP,
                    gzip_member(raw_deflate(a), a, extra=b"extra field", name=b"name.txt", comment=b"a comment", hcrc=True) +
                    gzip_member(raw_deflate(c, 1), c, name=b"second", hcrc=True) +
                    gzip_member(raw_deflate(b, 9), b, extra=b"", comment=b""), a + c + b))
    return out


def flip_crc(z: bytes, member_end: int | None = None) -> bytes:
    """One bit of the CRC-32 of the member that ends at member_end (the last)."""
    e = len(z) if member_end is None else member_end
    b = bytearray(z)
    b[e - 8 + 1] ^= 0x04
    return bytes(b)


def gzip_crc_twins() -> list[Case]:
    """A 200,000-byte dynamic member, a stored member and the second member
    of a pair, each with one CRC bit flipped."""
    import gzip
    t = text(200000, seed=41)
    a, b = t[:40000], t[50000:50000 + 70001]
    return [Case("gzip-200000-badcrc", GZIP, flip_crc(gzip.compress(t, mtime=0)), None, n=len(t)),
            Case("gzip-stored-badcrc", GZIP, flip_crc(gzip.compress(t, compresslevel=0, mtime=0)), None, n=len(t)),
            Case("gzip-2nd-member-badcrc", GZIP, gzip.compress(a, mtime=0) + flip_crc(gzip.compress(b, 1, mtime=0)), None,
                 n=len(a) + len(b)),
            Case("gzip-1st-member-badcrc", GZIP, flip_crc(gzip.compress(a, mtime=0)) + gzip.compress(b, 1, mtime=0), None,
                 n=len(a) + len(b))]


# (h) damaged streams the host tests pin (test_lz_host.py test_lz_damaged,
# test_gzip_host.py test_gzip_damaged, test_zstd_host.py): status, not data
def damaged_cases() -> list[Case]:
    import gzip
    import random
    import pyarrow as pa
    out = []

    def bad(name, codec, z, n, elsewhere_ok=False):
        out.append(Case(name, codec, bytes(z), None, n=n, elsewhere_ok=elsewhere_ok))
    bad("snappy-copy-no-history", SNAPPY, bytes([4, (0 << 2) | 1, 1]), 4)
    bad("lz4-copy-no-history", LZ4_RAW, bytes([0x00, 1, 0]), 4)
    d = bytes(range(256)) * 40
    z = pa.Codec("lz4_raw").compress(d, asbytes=True)
    bad("lz4-page-short", LZ4_RAW, z, len(d) - 4)
    # (whole streams in a page of another size: pyarrow fills what it is given)
    bad("lz4-page-long", LZ4_RAW, z, len(d) + 4, elsewhere_ok=True)
    z = pa.Codec("snappy").compress(d, asbytes=True)
    bad("snappy-length-differs", SNAPPY, z, len(d) + 4, elsewhere_ok=True)
    for cut in (1, 2, len(z) // 2, len(z) - 1):
        bad(f"snappy-cut{cut}", SNAPPY, z[:cut], len(d))
    c = pa.Codec("lz4_raw")
    zh = b"".join(struct.pack(">II", len(d[i:i + 4096]), len(c.compress(d[i:i + 4096], asbytes=True))) +
                  c.compress(d[i:i + 4096], asbytes=True) for i in range(0, len(d), 4096))
    for cut in (3, 8, 9, len(zh) // 2):
        bad(f"hadoop-cut{cut}", LZ4, zh[:cut], len(d))
    b = bytearray(zh)
    b[3] ^= 1
    bad("hadoop-raw-size-differs", LZ4, b, len(d))
    g = b"".join(random.Random(2).choice([b"alpha ", b"beta ", b"gamma "]) for _ in range(4000))
    g = g[:len(g) // 4 * 4]
    z = gzip.compress(g, mtime=0)
    b = bytearray(z)
    b[-8] ^= 1
    bad("gzip-crc", GZIP, b, len(g))
    b = bytearray(z)
    b[-4] ^= 1
    bad("gzip-isize", GZIP, b, len(g))
    bad("gzip-page-short", GZIP, z, len(g) - 4)
    bad("gzip-page-long", GZIP, z, len(g) + 4)
    for cut in (1, 5, 10, 11, len(z) // 2, len(z) - 8, len(z) - 1):
        bad(f"gzip-cut{cut}", GZIP, z[:cut], len(g))
    bad("gzip-method9", GZIP, b"\x1f\x8b\x09" + z[3:], len(g))
    # a fixed-Huffman block: literal 'a', then a match of 3 from distance 2
    w = Deflate()
    w._put(1, 1)
    w._put(1, 2)
    w._put(*_FIXED[ord("a")])
    w._put(*_FIXED[257])
    w._put(_FDIST[1], 5)
    w._put(*_FIXED[256])
    bad("zlib-distance-before-start", GZIP, b"\x78\x01" + w.done() + b"\0\0\0\0", 4)
    bad("zstd-weights-zero-run", ZSTD, zstd_bad_weights_frame(), 100)
    return out


def _bits_le(fields) -> bytes:
    acc = n = 0
    for v, nb in fields:
        acc |= v << n
        n += nb
    return acc.to_bytes((n + 7) // 8, "little")


def zstd_bad_weights_frame() -> bytes:
    """test_zstd_host.py test_zstd_huffman_weights_zero_run_past_alphabet's
    frame: an FSE-coded Huffman weight table whose zero run passes the 12
    weight symbols the format allows."""
    hdesc = _bits_le([(0, 4), (1, 5)] + [(3, 2)] * 22 + [(0, 2)])
    huf = bytes([len(hdesc) + 3]) + hdesc + b"\x00" * 3
    regen, comp = 100, len(huf) + 8
    lit_hdr = (2 | (0 << 2) | (regen << 4) | (comp << 14)).to_bytes(3, "little")
    body = lit_hdr + huf + b"\x55" * 8 + b"\x00"
    block = (1 | (2 << 1) | (len(body) << 3)).to_bytes(3, "little") + body
    return bytes([0x28, 0xB5, 0x2F, 0xFD, 0x20, regen]) + block


def hadoop_cases() -> list[Case]:
    """Hadoop LZ4 framing over crafted blocks: several blocks in one page, an
    empty-literal last sequence excluded (every block ends as pad4 ends it)."""
    r = rnd(80000, seed=43)
    b1 = pad4([("lit", r[:3000]), ("copy", 3000, 500), ("copy", 1, 70)])
    b2 = pad4([("lit", r[3000:3010]), ("copy", 3, 66000)])
    b3 = pad4([("lit", r[4000:74000]), ("copy", 65535, 64), ("copy", 65535, 200)])
    b4 = [("lit", r[:8])]
    out = [Case("hadoop-4-blocks", LZ4, lz4_hadoop([b1, b2, b3, b4]), b"".join(model(b) for b in (b1, b2, b3, b4))),
           Case("hadoop-small-3-blocks", LZ4, lz4_hadoop([b1, b4, b1]), model(b1) + model(b4) + model(b1))]
    return out


# (g) the first byte a copy may reach (in a V2 page: the first value byte,
# behind the level sections)
def reach_cases(codec: int) -> tuple[Case, Case]:
    """(a copy whose distance equals the bytes produced so far, one whose
    distance is one more)."""
    nm = "snappy" if codec == SNAPPY else "lz4"
    r = rnd(400, seed=47)
    ok = pad4([("lit", r[:100]), ("copy", 100, 50), ("lit", r[100:107]), ("copy", 157, 157), ("copy", 314, 7)])
    good = lz_case(f"{nm}-reach-first-byte", codec, ok)
    over = [("lit", r[:100]), ("copy", 101, 50), ("lit", r[100:122])]
    n = 100 + 50 + 22
    z = varint(n) + b"".join(snappy_elements(over)) if codec == SNAPPY else lz4_block(over)
    return good, Case(f"{nm}-reach-before-first-byte", codec, z, None, n=n)
