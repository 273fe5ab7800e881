"""CPU tests of the references in ``kernel_refs.py`` that the GPU kernel
tests compare against: the join-pair reference against the ops layer's
pandas join, the hash against the ops layer's numpy copy, and the
postfix-program reference on hand-computed rows."""
import numpy as np
import pyarrow as pa
import pytest

torch = pytest.importorskip("torch")

import kernel_refs as kr
from fugue_amd.column.expressions import col, lit
from fugue_amd.hip import expr as hexpr
from fugue_amd.hip import ops as dops
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
from fugue_amd.schema import Schema

I64_MIN, I64_MAX = kr.INT64_MIN, kr.INT64_MAX
MODES = {"inner": 0, "left": 1, "semi": 2, "anti": 3}


def _join_case(seed: int, with_h2: bool):
    rng = np.random.default_rng(seed)
    b = rng.integers(-20, 20, 300).astype(np.int64)
    p = rng.integers(-30, 30, 500).astype(np.int64)
    b[:4] = [I64_MIN, I64_MAX, 0, -1]
    p[:4] = [I64_MIN, I64_MAX, 0, -1]
    if not with_h2:
        return p, b, None, None
    return p, b, rng.integers(0, 3, 500), rng.integers(0, 3, 300)


@pytest.mark.parametrize("with_h2", [False, True])
@pytest.mark.parametrize("how", list(MODES))
def test_join_reference_matches_ops_cpu(how, with_h2):
    p, b, p2, b2 = _join_case(5, with_h2)
    t = torch.from_numpy
    ep, eb = dops._hash_join_indices_cpu(
        t(p), t(b), how,
        None if p2 is None else t(p2), None if b2 is None else t(b2),
    )
    gp, gb = kr.join_pairs_ref(p, b, MODES[how], p2, b2)
    exp = kr.sorted_pairs(ep.numpy(), eb.numpy())
    got = kr.sorted_pairs(gp, gb)
    assert len(exp) > 0
    np.testing.assert_array_equal(got, exp)
    # counts agree with the pair list
    cnt = kr.match_counts(p, b, p2, b2)
    assert int(kr.out_counts(cnt, MODES[how]).sum()) == len(exp)


def test_join_reference_empty_sides():
    e = np.empty(0, dtype=np.int64)
    p = np.array([3, 4, 3], dtype=np.int64)
    for mode in range(4):
        pi, bi = kr.join_pairs_ref(e, p, mode)
        assert len(pi) == 0 and len(bi) == 0
    assert len(kr.join_pairs_ref(p, e, 0)[0]) == 0
    assert len(kr.join_pairs_ref(p, e, 2)[0]) == 0
    for mode in (1, 3):
        pi, bi = kr.join_pairs_ref(p, e, mode)
        np.testing.assert_array_equal(pi, [0, 1, 2])
        np.testing.assert_array_equal(bi, [-1, -1, -1])


def test_mix64_matches_ops_copy_and_known_value():
    x = np.array([0, 1, -1, I64_MIN, I64_MAX, 123456789], dtype=np.int64)
    np.testing.assert_array_equal(
        kr.mix64(x), dops._np_mix64(x.view(np.uint64).copy())
    )
    # fmix64(1), by hand from the two multiply/xor-shift rounds
    v = 1
    for m in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53):
        v ^= v >> 33
        v = (v * m) & (2**64 - 1)
    v ^= v >> 33
    assert int(kr.mix64(np.array([1], dtype=np.int64))[0]) == v
    assert int(kr.mix64(np.array([0], dtype=np.int64))[0]) == 0
    s = kr.slot_of(x, 16)
    assert s.min() >= 0 and s.max() < 16


def _frame():
    c = lambda a, v=None: (torch.from_numpy(np.array(a)),
                           None if v is None else torch.tensor(v))
    cols = {
        "a": DeviceColumn(*c(np.array([1, -2, I64_MIN, 3], dtype=np.int64)), pa.int64()),
        "x": DeviceColumn(
            *c(np.array([0.5, 2.0, np.nan, 4.0]), [True, False, True, True]),
            pa.float64(),
        ),
        "h": DeviceColumn(*c(np.array([1, 0, 2, -3], dtype=np.int16)), pa.int16()),
        "b": DeviceColumn(
            *c(np.array([True, False, True, True]), [True, True, False, True]),
            pa.bool_(),
        ),
    }
    return HipDataFrame.from_columns(
        cols, Schema("a:long,x:double,h:short,b:bool"), "cpu"
    )


def _run(e, wide=False):
    df = _frame()
    b = hexpr._ProgBuilder(df)
    b.emit(e)
    tag, v, valid = kr.run_program(*kr.program_of(b), df.count(), wide=wide)
    assert tag == b.tags[-1], "static tag simulation disagrees"
    return tag, v, valid


def test_program_reference_hand_rows():
    # int arithmetic wraps, stays int, all valid
    tag, v, valid = _run(col("a") * lit(2) + col("h"))
    assert tag == kr.TAG_I and valid.all()
    assert v.tolist() == [3, -4, 2, 3]  # I64_MIN*2 wraps to 0
    tag, v, valid = _run(-col("a") - lit(0))
    assert v.tolist() == [-1, 2, I64_MIN, -3]
    # float arithmetic propagates invalid; division is always float
    tag, v, valid = _run(col("x") * col("h") + lit(1))
    assert tag == kr.TAG_F and valid.tolist() == [True, False, True, True]
    assert v[0] == 1.5 and np.isnan(v[2]) and v[3] == -11.0
    tag, v, valid = _run(col("h") / (col("h") - col("h")))
    assert tag == kr.TAG_F and valid.all()
    assert v[0] == np.inf and np.isnan(v[1]) and v[3] == -np.inf
    # comparisons on null are false for every op, != included
    for e in (col("x") != lit(7.0), col("x") < lit(7.0)):
        tag, v, valid = _run(e)
        assert tag == kr.TAG_B and valid.all()
        assert kr.filter_of(tag, v, valid).tolist()[1] is False
    # NaN: != is true, == and < are false
    assert kr.filter_of(*_run(col("x") != col("x"))).tolist() == [
        False, False, True, False]
    assert kr.filter_of(*_run(col("x") == col("x"))).tolist() == [
        True, False, False, True]
    # NOT / AND / OR treat null as false; IS NULL reads the bit
    assert kr.filter_of(*_run(~col("b"))).tolist() == [False, True, True, False]
    assert kr.filter_of(*_run(col("b") & (col("x") > lit(0)))).tolist() == [
        True, False, False, True]
    assert kr.filter_of(*_run(col("b") | col("x").is_null())).tolist() == [
        True, True, False, True]
    assert kr.filter_of(*_run(col("b").is_null())).tolist() == [
        False, False, True, False]
    assert kr.filter_of(*_run(col("x").not_null())).tolist() == [
        True, False, True, True]
    # bool under arithmetic is an int; float against int compares as float
    tag, v, valid = _run(col("b") + col("b"))
    assert tag == kr.TAG_I and v.tolist() == [2, 0, 2, 2]
    assert valid.tolist() == [True, True, False, True]
    assert kr.filter_of(*_run(col("x") > col("a"))).tolist() == [
        False, False, False, True]
    # wide mode carries more than 53 bits
    tag, v, valid = _run(col("x") / lit(3.0), wide=True)
    assert v.dtype == np.longdouble
    assert v[0] != np.longdouble(np.float64(0.5) / np.float64(3.0))


# ------------------------------------------------------------------ #
# hashing, partitioning                                               #
# ------------------------------------------------------------------ #

_HASH_DTYPES = [np.bool_, np.int8, np.int16, np.int32, np.int64,
                np.float32, np.float64]
_PA = {np.bool_: pa.bool_(), np.int8: pa.int8(), np.int16: pa.int16(),
       np.int32: pa.int32(), np.int64: pa.int64(), np.float32: pa.float32(),
       np.float64: pa.float64()}


def _hash_column(dt, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if dt == np.bool_:
        return rng.random(n) < 0.5
    if np.dtype(dt).kind == "f":
        a = (rng.standard_normal(n) * 1e3).astype(dt)
        a[:4] = [0.0, -0.0, np.inf, np.nan]
        return a
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    a[:4] = [info.min, info.max, -1, 0]
    return a


def test_int_hash_helpers_match_numpy():
    x = np.array([0, 1, -1, I64_MIN, I64_MAX, 123456789], dtype=np.int64)
    m = kr.mix64(x)
    assert [kr.mix64_int(int(v)) for v in x] == [int(v) for v in m]
    h = kr.hash_combine(m, m[::-1].copy())
    assert [int(v) for v in h] == [
        kr.hash_combine_int(int(a), int(b)) for a, b in zip(m, m[::-1])
    ]
    np.testing.assert_array_equal(h, dops._np_hash_combine(m, m[::-1].copy()))


@pytest.mark.parametrize("seed", [None, 0, 0x5851F42D4C957F2D])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dt", _HASH_DTYPES, ids=lambda d: np.dtype(d).name)
def test_hash_rows_reference_matches_ops_cpu(dt, masked, seed):
    """The ops layer's numpy twin of the kernel hash agrees with the
    reference for every fixed-width type, alone and as a later column;
    int16 (negative values included) hashes as the int32 it is widened
    to."""
    n = 64
    a = _hash_column(dt, n, 3)
    lead = _hash_column(np.int64, n, 4)
    valid = np.random.default_rng(5).random(n) < 0.7 if masked else None
    t = torch.from_numpy
    dc = DeviceColumn(t(a), None if valid is None else t(valid), _PA[dt])
    lc = DeviceColumn(t(lead), None, pa.int64())
    for cols, ref_cols in (
        ([dc], [(a, valid)]),
        ([lc, dc], [(lead, None), (a, valid)]),
    ):
        got = dops._hash_rows_cpu(cols, seed=seed).numpy().view(np.uint64)
        np.testing.assert_array_equal(got, kr.hash_rows_ref(ref_cols, seed))
    if masked:
        h = kr.hash_rows_ref([(a, valid)])
        assert (h[~valid] == np.uint64(kr.NULL_HASH)).all()


def test_hash_rows_reference_widths_by_hand():
    """What each width feeds to mix64, on a negative value."""
    m = kr.mix64_int
    one = lambda v, dt: int(kr.hash_rows_ref([(np.array([v], dtype=dt), None)])[0])
    assert one(-2, np.int8) == m(0xFE)
    assert one(-2, np.int16) == m(0xFFFFFFFE)  # widened to int32
    assert one(-2, np.int32) == m(0xFFFFFFFE)
    assert one(-2, np.int64) == m(2**64 - 2)
    assert one(True, np.bool_) == m(1)
    assert one(1.0, np.float32) == m(0x3F800000)
    assert one(-0.0, np.float64) == m(1 << 63)
    assert one(0.0, np.float64) == 0  # mix64(0)
    # seeded: the start value is combined with the first column
    s = 12345
    assert kr.seeded_start(s) == m(s + 1)
    got = int(kr.hash_rows_ref([(np.array([7], dtype=np.int64), None)], s)[0])
    assert got == kr.hash_combine_int(m(s + 1), m(7))
    # null: the canonical hash, whatever is stored
    got = kr.hash_rows_ref([(np.array([7], dtype=np.int64), np.array([False]))])
    assert int(got[0]) == kr.NULL_HASH == 0x9E3779B97F4A7C15
    assert len(kr.hash_rows_ref([(np.empty(0, dtype=np.int32), None)])) == 0


def test_hash_bytes_hand_rows():
    m, hc = kr.mix64_int, kr.hash_combine_int
    seed = 0x27D4EB2F165667C5
    assert kr.hash_bytes(b"") == m(seed)
    assert kr.hash_bytes(b"a") == m(hc(seed ^ 1, 0x61))
    # 7-byte tail: big-endian accumulation
    assert kr.hash_bytes(b"abcdefg") == m(hc(seed ^ 7, 0x61626364656667))
    # one whole block: little-endian load, no tail step
    assert kr.hash_bytes(b"abcdefgh") == m(hc(seed ^ 8, 0x6867666564636261))
    assert kr.hash_bytes(b"abcdefghi") == m(
        hc(hc(seed ^ 9, 0x6867666564636261), 0x69)
    )
    assert kr.hash_bytes(b"abcdefghABCDEFGH") == m(
        hc(hc(seed ^ 16, 0x6867666564636261), 0x4847464544434241)
    )
    # a trailing NUL changes the length and the tail
    assert kr.hash_bytes(b"ab") == m(hc(seed ^ 2, 0x6162))
    assert kr.hash_bytes(b"ab\0") == m(hc(seed ^ 3, 0x616200))
    assert kr.hash_bytes(b"ab") != kr.hash_bytes(b"ab\0")
    assert kr.hash_bytes(b"\0") != kr.hash_bytes(b"")
    # as a column: nulls keep the canonical hash, later columns combine
    col_ = [b"", b"abcdefghi", b"zz"]
    valid = np.array([True, True, False])
    h = kr.hash_rows_ref([(col_, valid)])
    assert [int(x) for x in h] == [
        kr.hash_bytes(b""), kr.hash_bytes(b"abcdefghi"), kr.NULL_HASH]
    k = np.array([1, 2, 3], dtype=np.int32)
    h2 = kr.hash_rows_ref([(k, None), (col_, valid)])
    assert int(h2[1]) == hc(m(2), kr.hash_bytes(b"abcdefghi"))
    assert int(h2[2]) == hc(m(3), kr.NULL_HASH)


def test_part_and_bucket_references():
    keys = np.array([0, 1, -1, I64_MIN, I64_MAX, 99], dtype=np.int64)
    for parts in (1, 2, 16, 4096):
        bits = parts.bit_length() - 1
        exp = [kr.mix64_int(int(k)) >> (64 - bits) if bits else 0 for k in keys]
        assert kr.part_of(keys, parts).tolist() == exp
    h = np.array([0, -(2**63), -1, 5], dtype=np.int64)  # 0, 2^63, 2^64-1, 5
    assert kr.bucket_of_ref(h, 7).tolist() == [0, 2**63 % 7, (2**64 - 1) % 7, 5]
    assert kr.bucket_of_ref(h, 1).tolist() == [0, 0, 0, 0]
    assert kr.bucket_of_ref(h, 1000).tolist() == [0, 2**63 % 1000, 615, 5]


# ------------------------------------------------------------------ #
# group-by, reductions, key preparation                               #
# ------------------------------------------------------------------ #


def test_groupby_reference_matches_ops_cpu():
    rng = np.random.default_rng(17)
    n = 600
    keys = rng.integers(-8, 8, n).astype(np.int64)
    keys[:3] = [I64_MIN, I64_MAX, I64_MIN]
    v = rng.integers(-1000, 1000, (2, n)).astype(np.float64)
    valid1 = rng.random(n) < 0.6
    valid1[:3] = True
    valid1[keys == 3] = False  # one group without a valid value
    t = torch.from_numpy
    df = HipDataFrame.from_columns(
        {
            "k": DeviceColumn(t(keys), None, pa.int64()),
            "a": DeviceColumn(t(v[0]), None, pa.float64()),
            "b": DeviceColumn(t(v[1]), t(valid1), pa.float64()),
        },
        Schema("k:long,a:double,b:double"), "cpu",
    )
    aggs = [("a", 0, "sa"), ("a", 1, "mina"), ("b", 2, "maxb"),
            ("b", 3, "cntb"), ("b", 0, "sb"), ("b", 1, "minb")]
    ok, oa, oc, meta = dops.groupby_aggregate(df, ["k"], aggs)
    assert meta is None
    order = np.argsort(ok.numpy())
    vals = np.stack([v[0], v[0], v[1], v[1], v[1], v[1]])
    valids = np.stack([np.ones(n, bool)] * 2 + [valid1] * 4)
    rk, rc, ra = kr.groupby_ref(keys, vals, valids, [op for _, op, _ in aggs])
    np.testing.assert_array_equal(ok.numpy()[order], rk)
    np.testing.assert_array_equal(oc.numpy()[order], rc)
    has_b = ra[3] > 0
    assert (~has_b).sum() == 1
    for i, (_, op, name) in enumerate(aggs):
        got = oa[name].numpy()[order]
        # pandas has NaN for MIN/MAX of no values; the tables keep the identity
        sel = has_b if op in (1, 2) else np.ones(len(rk), bool)
        np.testing.assert_array_equal(got[sel], ra[i][sel])
    assert ra[2][~has_b] == -np.inf and ra[5][~has_b] == np.inf
    assert ra[4][~has_b] == 0.0 and ra[3][~has_b] == 0.0


def test_groupby_and_reduce_reference_hand_rows():
    keys = np.array([5, -1, 5, 5, -1], dtype=np.int64)
    vals = np.array([[1e16, -0.0, 1.0, -1e16, -0.0],
                     [2.0, np.inf, -3.0, 0.0, 1.0]])
    valids = np.array([[True] * 5, [True, True, False, True, False]])
    k, c, a = kr.groupby_ref(keys, vals, valids, [0, 1])
    assert k.tolist() == [-1, 5] and c.tolist() == [2, 3]
    # exact sum (a left-to-right double sum of key 5 gives 0.0), and a
    # group of -0.0 only sums to +0.0 like a table that starts at +0.0
    assert a[0].tolist() == [0.0, 1.0] and not np.signbit(a[0][0])
    assert a[1].tolist() == [np.inf, 0.0]
    out, cnt = kr.reduce_cols_ref(vals, valids, [0, 2])
    assert out.tolist() == [1.0, np.inf] and cnt.tolist() == [5, 3]
    out, cnt = kr.reduce_cols_ref(vals, np.zeros((2, 5), bool), [1, 2])
    assert out.tolist() == [np.inf, -np.inf] and cnt.tolist() == [0, 0]
    assert kr.abs_sums(keys, vals[1][[0, 2, 2, 3, 4]]).tolist() == [4.0, 5.0]
    tk = np.array([I64_MIN, 7, I64_MIN, -2], dtype=np.int64)
    k, c, a = kr.table_groups(tk, np.array([0, 3, 0, 1]), np.arange(8.0).reshape(2, 4))
    assert k.tolist() == [-2, 7] and c.tolist() == [1, 3]
    assert a.tolist() == [[3.0, 1.0], [7.0, 5.0]]


def test_key_stats_reference_hand_rows():
    a = np.array([3, 3, 9, 3, -4, 9, 7, 3, 3, 1], dtype=np.int64)
    b = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 1], dtype=np.int16)
    vb = np.array([1, 1, 1, 0, 1, 1, 1, 1, 1, 1], dtype=bool)
    mins, maxs, d, f1, f2 = kr.key_stats_ref([a, b], [None, vb], 100)
    assert mins == [-4, 1] and maxs == [9, 1]
    # rows: (3,1)x4, (3,null), (9,1)x2, (-4,1), (7,1), (1,1)
    assert (d, f1, f2) == (6, 4, 1)
    # nsamples 4 -> stride 2, rows 0 2 4 6: 3 9 -4 7
    assert kr.key_stats_ref([a], [None], 4)[2:] == (4, 4, 0)
    # nsamples 3 -> stride 3, eff 3, rows 0 3 6: 3 3 7
    assert kr.key_stats_ref([a], [None], 3)[2:] == (2, 1, 1)
    ext = np.array([I64_MIN, I64_MAX], dtype=np.int64)
    assert kr.key_stats_ref([ext], [None], 2)[:2] == ([I64_MIN], [I64_MAX])


def test_pack_reference_and_code_width():
    assert [kr.code_width(0, h) for h in (0, 1, 2, 3, 6, 7)] == [1, 2, 2, 3, 3, 4]
    # codes 0 .. 2^60 need 61 bits; a float log2 of 2^60 + 1 says 60
    for lo, hi in [(0, 2**60 - 1), (-5, 2**53 - 5), (I64_MIN, I64_MAX), (4, 4)]:
        assert dops._code_width(lo, hi) == kr.code_width(lo, hi)
        assert (hi - lo + 1) < (1 << kr.code_width(lo, hi))
    assert kr.code_width(0, 2**60 - 1) == 61
    assert kr.pack_shifts([3, 5, 2]) == [7, 2, 0]
    a = np.array([-3, 0, 4], dtype=np.int64)
    b = np.array([10, 11, 10], dtype=np.int32)
    vb = np.array([True, False, True])
    widths = [kr.code_width(-3, 4), kr.code_width(10, 11)]
    assert widths == [4, 2]
    p = kr.pack_ref([a, b], [None, vb], [-3, 10], widths)
    assert p.tolist() == [(1 << 2) | 1, (4 << 2) | 0, (8 << 2) | 1]
    (ua, va), (ub, vb2) = kr.unpack_ref(p, [-3, 10], widths)
    assert ua.tolist() == [-3, 0, 4] and va.all()
    assert vb2.tolist() == [True, False, True] and ub[[0, 2]].tolist() == [10, 10]
    # the ops layer's torch packing agrees (CPU tensors take that path)
    t = torch.from_numpy
    cols = [DeviceColumn(t(a), None, pa.int64()),
            DeviceColumn(t(b), t(vb), pa.int32())]
    pk, meta = dops.pack_keys(cols)
    assert meta["mins"] == [-3, 10] and meta["widths"] == widths
    np.testing.assert_array_equal(pk.numpy(), p)
    # a nullable column spanning 2^60 values keeps its largest value
    big = np.array([0, 2**60 - 1], dtype=np.int64)
    pk, meta = dops.pack_keys(
        [DeviceColumn(t(big), t(np.array([True, True])), pa.int64())]
    )
    assert meta["widths"] == [61]
    back = dops.unpack_keys(pk, meta, cols[:1])[0]
    assert back.data.tolist() == big.tolist()
    assert back.valid is None or bool(back.valid.all())


def test_cpu_string_hash_ignores_nulls_elsewhere():
    """The host twin hashes a string the same whether or not the column
    also holds a null (rows of one key must meet on one rank)."""
    from fugue_amd.hip.frame import StringDeviceColumn

    def h(values):
        arr = pa.array(values, type=pa.string())
        c = StringDeviceColumn.from_arrow_strings(arr, "cpu")
        return dops._hash_rows_cpu([c]).numpy().view(np.uint64)

    a, b = h(["", "x", None, "yy"]), h(["", "x", "q", "yy"])
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3]
    assert int(a[2]) == kr.NULL_HASH and a[0] != a[2]


def test_pack_keys_float_keys_cast_only_when_exact():
    t = torch.tensor
    whole = DeviceColumn(
        t([2.0, -0.0, 0.0, -3.0], dtype=torch.float64), None, pa.float64()
    )
    pk, meta = dops.pack_keys([whole])
    assert pk.tolist() == [6, 4, 4, 1] and meta["mins"] == [-3]
    for bad in ([1.0, 1.5], [0.0, float("inf")], [float("nan")], [1e300]):
        with pytest.raises(NotImplementedError):
            dops.pack_keys([DeviceColumn(t(bad, dtype=torch.float64), None, pa.float64())])
    # an invalid cell may hold anything
    c = DeviceColumn(
        t([1.0, 0.5], dtype=torch.float64), t([True, False]), pa.float64()
    )
    pk, meta = dops.pack_keys([c])
    assert pk.tolist() == [2, 0] and meta["mins"] == [0]
