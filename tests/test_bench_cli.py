"""bench.py's command line and its --dump-outputs writer (no GPU: the writer
is fed a host column built here)."""
import os
import sys

import numpy as np

import bench
from pqgpu import capi


def _args(argv):
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        return bench.parse()
    finally:
        sys.argv = old


def test_plain_run_is_the_default():
    a = _args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = _args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def _column(n, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(rng.integers(0, 9, n))]).astype(np.int64)
    return capi.HostColumn(capi.BYTE_ARRAY, rng.integers(0, 2, n).astype(np.uint8),
                           rng.integers(0, 256, int(off[-1])).astype(np.uint8), off)


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_sampled(tmp_path):
    """A column longer than the sample sizes: fixed sample, float dtypes, whole
    array covered by the block sums, same files from the same column."""
    n = bench.DUMP_ROWS + 12345
    h = _column(n, 1)
    bench.dump_outputs(h, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(h, str(tmp_path / "b"), 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["chars.npy", "chars_sums.npy", "offsets.npy", "offsets_sums.npy", "validity.npy",
                         "validity_sums.npy"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert len(a["validity.npy"]) == bench.DUMP_ROWS and len(a["offsets.npy"]) == bench.DUMP_ROWS + 1
    assert len(a["chars.npy"]) == bench.DUMP_CHARS
    assert a["offsets.npy"][-1] == h.offsets[-1]
    assert a["validity_sums.npy"].sum() == h.validity.sum()
    assert a["chars_sums.npy"].sum() == h.data.sum(dtype=np.int64)
    assert a["offsets_sums.npy"].sum() == h.offsets.sum()
    # one flipped char shows in the block sums, sampled or not
    h.data[-1] ^= 1
    bench.dump_outputs(h, str(tmp_path / "c"), 0, 1)
    assert not np.array_equal(_load(tmp_path / "c")["chars_sums.npy"], a["chars_sums.npy"])


def test_dump_outputs_small_whole(tmp_path):
    """A column no longer than the sample sizes is written whole; ranks of a
    multi-GPU run write their own files."""
    h = _column(1000, 2)
    bench.dump_outputs(h, str(tmp_path), 1, 2)
    a = _load(tmp_path)
    assert np.array_equal(a["validity.rank1.npy"], h.validity.astype(np.float32))
    assert np.array_equal(a["offsets.rank1.npy"], np.concatenate([h.offsets[:-1], h.offsets[-1:]]).astype(np.float64))
    assert np.array_equal(a["chars.rank1.npy"], h.data.astype(np.float32))
