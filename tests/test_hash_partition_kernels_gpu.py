"""GPU tests of the hashing and bucket-partition kernels
(``hash_partition.hip``) against the Python-int / numpy references of
``kernel_refs.py``.  Everything is integer arithmetic, so every
comparison is bit for bit.

Row hashes go through ``ops.hash_rows`` (which owns the int16 widening
and the seeded start), the bucket kernels through ``get_ext()``."""
import functools

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

import kernel_refs as kr
from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine
from fugue_amd.hip.ext import get_ext
from fugue_amd.hip.frame import DeviceColumn, StringDeviceColumn

SEED = 0x5851F42D4C957F2D
HASH_N = [0, 1, 255, 257, 70_001]
DTYPES = [np.bool_, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
PA_OF = {
    np.bool_: pa.bool_(), np.int8: pa.int8(), np.int16: pa.int16(),
    np.int32: pa.int32(), np.int64: pa.int64(), np.float32: pa.float32(),
    np.float64: pa.float64(),
}


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _column(dt, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if dt == np.bool_:
        return rng.random(n) < 0.5
    if np.dtype(dt).kind == "f":
        a = (rng.standard_normal(n) * 1e3).astype(dt)
        a[:4] = np.array([0.0, -0.0, np.inf, np.nan], dtype=dt)[: min(n, 4)]
        return a
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    a[:4] = np.array([info.min, info.max, -1, 0], dtype=dt)[: min(n, 4)]
    return a


def _fixed(a: np.ndarray, valid):
    """(device column, reference column) of a fixed-width array."""
    dc = DeviceColumn(
        _dev(a, a.dtype), None if valid is None else _dev(valid, np.bool_),
        PA_OF[a.dtype.type],
    )
    return dc, (a, valid)


def _strings(rows, valid):
    """(device column, reference column) of a list of ``bytes``; the
    bytes of null rows stay in the buffer."""
    lens = np.array([len(b) for b in rows], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = np.frombuffer(b"".join(rows), dtype=np.uint8)
    sc = StringDeviceColumn(
        _dev(offsets, np.int64), _dev(data, np.uint8),
        None if valid is None else _dev(valid, np.bool_),
    )
    return sc, (list(rows), valid)


def _check_hash(pairs, seed):
    got = _u64(dops.hash_rows([d for d, _ in pairs], seed=seed))
    np.testing.assert_array_equal(got, kr.hash_rows_ref([r for _, r in pairs], seed))
    return got


# ------------------------------------------------------------------ #
# 1. hash_rows                                                        #
# ------------------------------------------------------------------ #


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n", HASH_N)
def test_hash_rows_fixed_width(n, dt):
    """Each type alone (its cell hash is the row hash) and as a later
    column (combined into a running hash), with and without a validity
    mask and a seed."""
    a = _column(dt, n, 3)
    lead = _fixed(_column(np.int64, n, 4), None)
    mask = np.random.default_rng(5).random(n) < 0.7
    for valid in (None, mask):
        col = _fixed(a, valid)
        for seed in (None, SEED):
            _check_hash([col], seed)
            _check_hash([lead, col], seed)


def _words(rng, n: int):
    lens = rng.integers(0, 20, n)
    blob = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8).tobytes()
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [blob[offs[i] : offs[i + 1]] for i in range(n)]


@pytest.mark.parametrize("n", [1, 257, 70_001])
def test_hash_rows_four_column_mix(n):
    rng = np.random.default_rng(n)
    pairs = [
        _fixed(_column(np.int16, n, 6), rng.random(n) < 0.9),
        _strings(_words(rng, n), rng.random(n) < 0.8),
        _fixed(_column(np.float64, n, 7), None),
        _fixed(_column(np.bool_, n, 8), rng.random(n) < 0.5),
    ]
    for seed in (None, 0, SEED):
        _check_hash(pairs, seed)
    # a string column first: its cell hash starts the row hash
    _check_hash(pairs[1:], None)


def test_hash_rows_string_edges():
    rows = [
        b"", b"a", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefghABCDEFGH",
        bytes(range(256)) * 3 + bytes(232),  # 1000 bytes
        b"ab", b"ab\0", b"\0", b"", b"null-but-stored", b"abcdefgh",
    ]
    assert [len(r) for r in rows[:7]] == [0, 1, 7, 8, 9, 16, 1000]
    valid = np.ones(len(rows), dtype=bool)
    valid[[4, 11]] = False  # null rows whose byte range is not empty
    for v in (None, valid):
        for seed in (None, SEED):
            _check_hash([_strings(rows, v)], seed)
            lead = _fixed(np.arange(len(rows), dtype=np.int32), None)
            _check_hash([lead, _strings(rows, v)], seed)
    h = _check_hash([_strings(rows, valid)], None)
    assert h[7] != h[8], "a trailing NUL is part of the string"
    assert h[0] == h[10] and h[3] == h[12] and h[9] != h[0]
    assert h[4] == h[11] == np.uint64(kr.NULL_HASH)
    assert len(set(h.tolist())) == len(rows) - 3


def test_hash_rows_floats_hash_raw_bits():
    """The kernel's contract is the bit pattern: the two zeros differ,
    and so do two NaNs with different payloads."""
    bits = np.array(
        [0, 1 << 63, 0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000],
        dtype=np.uint64,
    )
    h = _check_hash([_fixed(bits.view(np.float64), None)], None)
    assert len(set(h.tolist())) == 5
    bits32 = np.array([0, 1 << 31, 0x7FC00000, 0x7FC00001], dtype=np.uint32)
    h = _check_hash([_fixed(bits32.view(np.float32), None)], None)
    assert len(set(h.tolist())) == 4


# ------------------------------------------------------------------ #
# 2. bucket_of / bucket_histogram / bucket_scatter                    #
# ------------------------------------------------------------------ #


@functools.lru_cache(maxsize=None)
def _hashes(n: int) -> np.ndarray:
    rng = np.random.default_rng(n)
    h = rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    h[:3] = np.array([0, 2**63, 2**64 - 1], dtype=np.uint64)[: min(n, 3)]
    h.setflags(write=False)
    return h


def _check_scatter(buckets: np.ndarray, num_buckets: int):
    """Histogram equals bincount; the scatter is a permutation that makes
    bucket ids non-decreasing, with run lengths equal to the histogram."""
    n = len(buckets)
    bd = _dev(buckets, np.int32)
    hist = get_ext().bucket_histogram(bd, num_buckets)
    exp = np.bincount(buckets, minlength=num_buckets)
    np.testing.assert_array_equal(hist.cpu().numpy(), exp)
    offsets = torch.zeros(num_buckets, dtype=torch.int64, device="cuda")
    torch.cumsum(hist[:-1], 0, out=offsets[1:])
    perm = get_ext().bucket_scatter(bd, offsets.clone()).cpu().numpy()
    np.testing.assert_array_equal(np.sort(perm), np.arange(n))
    along = buckets[perm]
    assert (np.diff(along) >= 0).all()
    np.testing.assert_array_equal(np.bincount(along, minlength=num_buckets), exp)


@pytest.mark.parametrize("n", [0, 1, 257, 50_003])
@pytest.mark.parametrize("num_buckets", [1, 2, 7, 8, 1000])
def test_bucket_of_histogram_scatter(num_buckets, n):
    h = _hashes(n)
    got = get_ext().bucket_of(_dev(h.view(np.int64), np.int64), num_buckets)
    assert got.dtype == torch.int32
    buckets = got.cpu().numpy()
    # the modulo is unsigned: 2^63 and 2^64 - 1 are not negative
    np.testing.assert_array_equal(buckets, kr.bucket_of_ref(h, num_buckets))
    assert n == 0 or (buckets.min() >= 0 and buckets.max() < num_buckets)
    _check_scatter(buckets, num_buckets)


@pytest.mark.parametrize("n", [257, 50_003])
def test_bucket_scatter_skewed(n):
    rng = np.random.default_rng(n)
    holes = rng.integers(0, 7, n).astype(np.int32)
    holes[holes == 3] = 4  # an empty bucket in the middle
    _check_scatter(holes, 7)
    _check_scatter(np.full(n, 999, dtype=np.int32), 1000)  # all in the last


# ------------------------------------------------------------------ #
# 3. partition_by_hash / partition_by_bucket_ids                      #
# ------------------------------------------------------------------ #


@pytest.fixture(scope="module")
def engine():
    return HipExecutionEngine()


def _payload_frame(n: int):
    rng = np.random.default_rng(n)
    s = [None if i % 11 == 0 else f"key-{i % 97}" * (i % 4) for i in range(n)]
    return pd.DataFrame(dict(s=s, i=np.arange(n), x=rng.random(n)))


@pytest.mark.parametrize("num_buckets", [1, 7, 64])
def test_partition_by_hash_keeps_rows(engine, num_buckets):
    pdf = _payload_frame(3001)
    df = engine.to_df(pdf)
    hashes = dops.hash_rows([df.col("s")])
    out, counts = dops.partition_by_hash(df, hashes, num_buckets)
    ref = kr.bucket_of_ref(_u64(hashes), num_buckets)
    np.testing.assert_array_equal(
        counts.cpu().numpy(), np.bincount(ref, minlength=num_buckets)
    )
    got = out.as_pandas()
    # bucket-contiguous, and every row still carries its own payload
    assert (np.diff(ref[got["i"].to_numpy()]) >= 0).all()
    pd.testing.assert_frame_equal(
        got.sort_values("i").reset_index(drop=True), pdf, check_dtype=False
    )
    again = kr.bucket_of_ref(_u64(dops.hash_rows([out.col("s")])), num_buckets)
    assert (np.diff(again) >= 0).all()


def test_partition_by_bucket_ids_keeps_rows(engine):
    pdf = _payload_frame(3001)
    df = engine.to_df(pdf)
    ids = np.random.default_rng(2).integers(0, 5, len(pdf))
    ids[ids == 2] = 4
    out, counts = dops.partition_by_bucket_ids(df, _dev(ids, np.int64), 5)
    np.testing.assert_array_equal(counts.cpu().numpy(), np.bincount(ids, minlength=5))
    got = out.as_pandas()
    assert (np.diff(ids[got["i"].to_numpy()]) >= 0).all()
    pd.testing.assert_frame_equal(
        got.sort_values("i").reset_index(drop=True), pdf, check_dtype=False
    )
