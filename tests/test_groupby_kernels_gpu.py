"""GPU tests of the group-by kernel family (``groupby.hip``), called
through ``get_ext()`` and compared with the numpy / Python-int references
of ``kernel_refs.py``.

Sums are compared for BIT equality: the values are integer-valued
doubles with |v| <= 2^20 and far fewer than 2^20 rows per group, so every
partial sum is an integer below 2^53 and every order of atomic addition
is exact.  One real-valued case per sum kernel uses the any-order bound
|got - exact| <= (m - 1) * 2^-53 * sum|v| for a group of m rows, checked
in rational arithmetic.  MIN and MAX are compared by value (a group
holding both zeros may report either).

No table here is smaller than twice its distinct keys: the insert probe
has no bound, and a full table would not terminate.  No key equals
GB_EMPTY at kernel level (the kernels' contract); the engine-level tests
at the end feed it through ``groupby_aggregate``, which takes it out."""
import functools
from fractions import Fraction

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
from fugue_amd.hip.ext import get_ext
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
from fugue_amd.schema import Schema

I64_MIN, I64_MAX = kr.INT64_MIN, kr.INT64_MAX
SUM, MIN, MAX, COUNT = kr.OP_SUM, kr.OP_MIN, kr.OP_MAX, kr.OP_COUNT
EDGE_KEYS = [I64_MAX, I64_MIN + 1, -1, 0, -(2**40) - 7, 2**31]


def _dev(a, dtype=np.int64):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _host(t):
    return t.cpu().numpy()


def _ops(ops):
    return _dev(ops, np.int32)


def _tsize(distinct: int) -> int:
    return dops._next_pow2(max(16, 2 * distinct))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _int_vals(rng, a: int, n: int) -> np.ndarray:
    """[a, n] integer-valued doubles, |v| <= 2^20."""
    return rng.integers(-(2**20), 2**20, (a, n), endpoint=True).astype(np.float64)


def _wrap_keys(tsize: int, count: int = 5) -> np.ndarray:
    """Distinct keys whose home slot is the LAST slot of a ``tsize``
    table, so all but one of them wrap to slot 0 and beyond.  tsize >=
    1024 puts them on the last slot of the 1024-slot LDS tables too."""
    cand = np.arange(1, 64 * tsize, dtype=np.int64)
    hit = cand[kr.slot_of(cand, tsize) == tsize - 1][:count]
    assert len(hit) == count
    return hit


def _key_shape(shape: str, n: int, tsize: int, rng) -> np.ndarray:
    """The key distributions every aggregating kernel is tried on."""
    if shape == "same":  # maximum same-address contention
        return np.full(n, -77, dtype=np.int64)
    if shape == "distinct":
        assert 2 * n <= tsize
        v = np.unique(rng.integers(I64_MIN + 1, I64_MAX, 2 * n + 16, dtype=np.int64))
        return rng.permutation(v)[:n]
    if shape == "wrap":
        return _wrap_keys(tsize)[rng.integers(0, 5, n)]
    assert shape == "edge"  # negative keys, INT64_MAX, the sentinel's neighbour
    return np.array(EDGE_KEYS, dtype=np.int64)[rng.integers(0, len(EDGE_KEYS), n)]


KEY_SHAPES = ["same", "distinct", "wrap", "edge"]


def _groups(out):
    """(keys ascending, counts, aggs [A, G]) of a kernel's (tkeys, gaggs,
    gcount, ...)."""
    return kr.table_groups(_host(out[0]), _host(out[2]), _host(out[1]))


def _check_table(out, keys, vals, valids, ops, tsize=None):
    """A kernel's (tkeys, gaggs, gcount) against ``groupby_ref``: keys and
    row counts exact, SUM and COUNT bit-equal, MIN and MAX equal by value;
    every empty slot still holds its initial count and aggregates."""
    tkeys, gaggs, gcount = (_host(t) for t in out[:3])
    if tsize is not None:
        assert tkeys.shape == (tsize,) and gaggs.shape == (len(ops), tsize)
    rk, rc, ra = kr.groupby_ref(keys, vals, valids, ops)
    gk, gc, ga = kr.table_groups(tkeys, gcount, gaggs)
    np.testing.assert_array_equal(gk, rk)
    np.testing.assert_array_equal(gc, rc)
    for a, op in enumerate(ops):
        if op in (SUM, COUNT):
            np.testing.assert_array_equal(_bits(ga[a]), _bits(ra[a]), err_msg=f"agg {a}")
        else:
            np.testing.assert_array_equal(ga[a], ra[a], err_msg=f"agg {a}")
    empty = tkeys == I64_MIN
    assert (gcount[empty] == 0).all()
    for a, op in enumerate(ops):
        init = {MIN: np.inf, MAX: -np.inf}.get(op, 0.0)
        assert (gaggs[a][empty] == init).all()
    return gk, ga


def _check_sum_bound(keys, v, gk, got):
    """|got - exact| <= (m - 1) * 2^-53 * sum|v| per group of m rows."""
    exact, mag, m = {}, {}, {}
    for k, x in zip(keys.tolist(), v.tolist()):
        f = Fraction(x)
        exact[k] = exact.get(k, 0) + f
        mag[k] = mag.get(k, 0) + abs(f)
        m[k] = m.get(k, 0) + 1
    assert sorted(exact) == gk.tolist()
    for k, g in zip(gk.tolist(), got.tolist()):
        err = abs(Fraction(g) - exact[k])
        assert err <= (m[k] - 1) * Fraction(1, 2**53) * mag[k], (k, g, float(err))


def _real_case(n: int, groups: int, seed: int):
    rng = np.random.default_rng(seed)
    keys = rng.integers(-groups // 2, groups // 2, n).astype(np.int64)
    v = rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))
    return keys, v


# ------------------------------------------------------------------ #
# 1. gb_aggregate, HBM kernel                                         #
# ------------------------------------------------------------------ #

SIX_OPS = [SUM, MIN, MAX, COUNT, SUM, MIN]


def _six_vals(rng, n: int) -> np.ndarray:
    vals = _int_vals(rng, 6, n)
    if n >= 4:
        # -0.0 in a sum; both infinities under MIN and MAX; +inf alone in a sum
        vals[0, :2] = -0.0
        vals[1, 1], vals[1, 2] = np.inf, -np.inf
        vals[2, 0], vals[2, 3] = -np.inf, np.inf
        vals[4, 3] = np.inf
        vals[5, :3] = [0.0, -0.0, 0.0]
    return vals


@pytest.mark.parametrize("mask", ["none", "random", "dead-groups"])
@pytest.mark.parametrize("n", [1, 255, 257, 1025, 5000])
def test_gb_aggregate_hbm_six_aggregates(n, mask):
    rng = np.random.default_rng(n)
    pool = np.concatenate(
        [np.array(EDGE_KEYS, dtype=np.int64), rng.integers(-50, 50, 34)]
    )
    keys = pool[rng.integers(0, len(pool), n)]
    vals = _six_vals(rng, n)
    valids = None
    if mask != "none":
        valids = rng.random((6, n)) < 0.7
        valids[3] = rng.random(n) < 0.2  # COUNT sees few rows
    if mask == "dead-groups":
        # aggregates 1 (MIN) and 4 (SUM) have no valid row in some groups
        dead = np.isin(keys, pool[::3])
        valids[1, dead] = False
        valids[4, dead] = False
    tsize = _tsize(len(pool))
    out = get_ext().gb_aggregate(
        _dev(keys), _dev(vals, np.float64),
        None if valids is None else _dev(valids, np.bool_),
        _ops(SIX_OPS), tsize, False,
    )
    gk, ga = _check_table(out, keys, vals, valids, SIX_OPS, tsize)
    if mask == "dead-groups":
        # identity left in place, while the rows were still counted
        hit = np.isin(gk, pool[::3])
        assert hit.any() or n == 1
        assert (ga[1][hit] == np.inf).all() and (_bits(ga[4][hit]) == 0).all()


@pytest.mark.parametrize("use_lds", [False, True])
@pytest.mark.parametrize("shape", KEY_SHAPES)
def test_gb_aggregate_key_shapes(shape, use_lds):
    n, tsize = 5000, 16384
    rng = np.random.default_rng(len(shape))
    keys = _key_shape(shape, n, tsize, rng)
    ops = [SUM, COUNT, SUM] if use_lds else [SUM, MIN, MAX, COUNT]
    vals = _int_vals(rng, len(ops), n)
    valids = rng.random((len(ops), n)) < 0.8
    out = get_ext().gb_aggregate(
        _dev(keys), _dev(vals, np.float64), _dev(valids, np.bool_),
        _ops(ops), tsize, use_lds,
    )
    _check_table(out, keys, vals, valids, ops, tsize)


@pytest.mark.parametrize("use_lds", [False, True])
def test_gb_aggregate_empty_and_single_row(use_lds):
    ops = [SUM, COUNT] if use_lds else [SUM, MIN]
    e = np.empty(0, dtype=np.int64)
    out = get_ext().gb_aggregate(
        _dev(e), _dev(np.empty((2, 0)), np.float64), None, _ops(ops), 16, use_lds
    )
    _check_table(out, e, np.empty((2, 0)), None, ops, 16)
    assert (_host(out[0]) == I64_MIN).all()
    for key in (I64_MAX, -5):
        keys = np.array([key], dtype=np.int64)
        vals = np.array([[7.0], [-3.0]])
        out = get_ext().gb_aggregate(
            _dev(keys), _dev(vals, np.float64), None, _ops(ops), 16, use_lds
        )
        _check_table(out, keys, vals, None, ops, 16)


@pytest.mark.parametrize("use_lds", [False, True])
def test_gb_aggregate_real_valued_sum(use_lds):
    keys, v = _real_case(5000, 40, 71)
    out = get_ext().gb_aggregate(
        _dev(keys), _dev(v[None, :], np.float64), None, _ops([SUM]), 128, use_lds
    )
    gk, _, ga = _groups(out)
    _check_sum_bound(keys, v, gk, ga[0])


# ------------------------------------------------------------------ #
# 2. gb_aggregate, LDS kernel                                         #
# ------------------------------------------------------------------ #

LDS_OPS = [SUM, COUNT, SUM, COUNT]


@functools.lru_cache(maxsize=None)
def _lds_case(spill: bool):
    """(keys, vals [4, n], valids [4, n]): under 1024 distinct keys, or
    5000 distinct keys in 20 000 rows, which overflow the 16-probe limit
    of the 1024-slot LDS table from inside blocks that also flush."""
    rng = np.random.default_rng(int(spill) + 40)
    n, distinct = (20_000, 5000) if spill else (5000, 300)
    pool = _key_shape("distinct", distinct, 4 * distinct, rng)
    pool[: len(EDGE_KEYS)] = EDGE_KEYS
    keys = pool[np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])]
    keys = rng.permutation(keys)
    vals = _int_vals(rng, 4, n)
    valids = rng.random((4, n)) < 0.75
    for a in (keys, vals, valids):
        a.setflags(write=False)
    return keys, vals, valids


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n_aggs", [1, 2, 3, 4])
@pytest.mark.parametrize("spill", [False, True])
def test_gb_aggregate_lds(spill, n_aggs, masked):
    keys, vals, valids = _lds_case(spill)
    vals = vals[:n_aggs]
    valids = valids[:n_aggs] if masked else None
    ops = LDS_OPS[:n_aggs]
    tsize = _tsize(len(np.unique(keys)))
    out = get_ext().gb_aggregate(
        _dev(keys), _dev(vals, np.float64),
        None if valids is None else _dev(valids, np.bool_),
        _ops(ops), tsize, True,
    )
    _check_table(out, keys, vals, valids, ops, tsize)


def test_gb_aggregate_lds_request_with_five_aggregates():
    """The LDS table holds four aggregates; the launcher sends a wider
    call to the HBM kernel, whatever ``use_lds`` says."""
    keys, vals, valids = _lds_case(True)
    vals5 = np.concatenate([vals, vals[:1] * 2.0])
    valids5 = np.concatenate([valids, valids[1:2]])
    ops = LDS_OPS + [SUM]
    tsize = _tsize(5000)
    out = get_ext().gb_aggregate(
        _dev(keys), _dev(vals5, np.float64), _dev(valids5, np.bool_),
        _ops(ops), tsize, True,
    )
    _check_table(out, keys, vals5, valids5, ops, tsize)


# ------------------------------------------------------------------ #
# 3. gb_aggregate_partitioned, simple path                            #
# ------------------------------------------------------------------ #


def _partitioned(keys, vals, ops, num_parts, tsize, **kw):
    args = dict(
        keys=_dev(keys), vals=_dev(vals, np.float64), ops=_ops(ops),
        num_parts=num_parts, tsize=tsize, scatter_chunk=0, agg_chunk=0,
        narrow=0, record_layout=False, force_simple=True,
    )
    args.update(kw)
    return get_ext().gb_aggregate_partitioned(**args)


@pytest.mark.parametrize("n", [1, 4095, 4097, 3 * 4096 + 5])
@pytest.mark.parametrize("num_parts", [16, 256, 4096])
def test_gb_partitioned_simple(num_parts, n):
    """1 to 4 SUM/COUNT aggregates around the scatter's 4096-row chunk;
    one aggregate takes the simple path by ``force_simple``, more take it
    by themselves."""
    rng = np.random.default_rng(n + num_parts)
    distinct = max(1, n // 3)
    pool = _key_shape("distinct", distinct, 4 * distinct + 16, rng)
    pool[: min(distinct, len(EDGE_KEYS))] = EDGE_KEYS[: min(distinct, len(EDGE_KEYS))]
    keys = pool[rng.integers(0, distinct, n)]
    vals = _int_vals(rng, 4, n)
    tsize = _tsize(distinct)
    for n_aggs in (1, 2, 3, 4):
        ops = LDS_OPS[:n_aggs]
        out = _partitioned(
            keys, vals[:n_aggs], ops, num_parts, tsize, force_simple=n_aggs == 1
        )
        _check_table(out, keys, vals[:n_aggs], None, ops, tsize)
        assert out[5].numel() == 0 and out[4].dtype == torch.int64


@pytest.mark.parametrize("shape", KEY_SHAPES)
def test_gb_partitioned_simple_key_shapes(shape):
    n, tsize = 5000, 16384
    rng = np.random.default_rng(len(shape) + 9)
    keys = _key_shape(shape, n, tsize, rng)
    vals = _int_vals(rng, 2, n)
    out = _partitioned(keys, vals, [SUM, COUNT], 16, tsize)
    _check_table(out, keys, vals, None, [SUM, COUNT], tsize)
    out = _partitioned(keys, vals[:1], [SUM], 256, tsize)
    _check_table(out, keys, vals[:1], None, [SUM], tsize)


def test_gb_partitioned_simple_empty_input():
    e = np.empty(0, dtype=np.int64)
    out = _partitioned(e, np.empty((2, 0)), [SUM, COUNT], 16, 16)
    _check_table(out, e, np.empty((2, 0)), None, [SUM, COUNT], 16)


def test_gb_partitioned_simple_spills():
    """16 partitions of 40 000 distinct keys: about 2500 keys per
    1024-slot LDS table, so most rows run out of their 32 probes and go
    to the global table from blocks that also flush."""
    rng = np.random.default_rng(3)
    distinct, n = 40_000, 60_000
    pool = _key_shape("distinct", distinct, 4 * distinct, rng)
    keys = pool[np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])]
    vals = _int_vals(rng, 2, n)
    tsize = _tsize(distinct)
    out = _partitioned(keys, vals, [SUM, COUNT], 16, tsize)
    _check_table(out, keys, vals, None, [SUM, COUNT], tsize)


def test_gb_partitioned_simple_real_valued_sum():
    keys, v = _real_case(5000, 40, 72)
    out = _partitioned(keys, np.stack([v, v]), [SUM, COUNT], 16, 128)
    gk, _, ga = _groups(out)
    _check_sum_bound(keys, v, gk, ga[0])


def test_gb_partitioned_simple_rejects_five_aggregates():
    """The per-partition LDS table holds four aggregates; the binding
    refuses more before anything is launched."""
    keys = np.arange(100, dtype=np.int64)
    with pytest.raises(RuntimeError, match="at most 4 aggregates"):
        _partitioned(keys, np.ones((5, 100)), [SUM] * 5, 16, 256)


# ------------------------------------------------------------------ #
# 4. recorded layout and replay                                       #
# ------------------------------------------------------------------ #


def _record_and_replay(keys, tsize, rng, parts=512):
    """Record the layout of ``keys`` (reservation chunk 512), check it,
    and replay fresh values through it: with the int64 spill keys, and
    narrowed to int32 where every key is in [0, 2^31)."""
    n = len(keys)
    vals = _int_vals(rng, 1, n)
    out = _partitioned(
        keys, vals, [SUM], parts, tsize, record_layout=True,
        force_simple=False, record_chunk=512,
    )
    _check_table(out, keys, vals, None, [SUM], tsize)
    pkeys, pos = _host(out[4]), _host(out[5]).astype(np.int64)
    assert pkeys.dtype == np.int64 and len(pkeys) == n
    assert out[5].dtype == torch.int32
    np.testing.assert_array_equal(np.sort(pos), np.arange(n))
    np.testing.assert_array_equal(pkeys[pos], keys)
    assert (np.diff(kr.part_of(pkeys, parts)) >= 0).all()
    # fresh values through the recorded layout
    fresh = _int_vals(rng, 1, n)
    narrowings = [out[4]]
    if n == 0 or (keys.min() >= 0 and keys.max() < 2**31):
        narrowings.append(out[4].to(torch.int32))
    for pk in narrowings:
        rep = get_ext().gb_aggregate_replay(
            pkeys=pk, pos=out[5], vals=_dev(fresh, np.float64), ops=_ops([SUM]),
            num_parts=parts, tsize=tsize, agg_chunk=0,
        )
        _check_table(rep, keys, fresh, None, [SUM], tsize)
    return out, len(narrowings)


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("n", [4097, 20_001])
def test_gb_partitioned_record_and_replay(n, negative):
    rng = np.random.default_rng(n + negative)
    distinct = n // 4
    if negative:
        pool = _key_shape("distinct", distinct, 4 * distinct, rng)
        pool[: len(EDGE_KEYS)] = EDGE_KEYS
    else:  # every key fits the int32 replay keys
        pool = rng.permutation(np.unique(rng.integers(0, 2**31, 2 * distinct)))
        pool = pool[:distinct]
        pool[:2] = [0, 2**31 - 1]
    keys = pool[rng.integers(0, len(pool), n)]
    tsize = _tsize(len(pool))
    out, replays = _record_and_replay(keys, tsize, rng)
    assert replays == (1 if negative else 2)
    real = rng.standard_normal(n) * 1e6
    rep = get_ext().gb_aggregate_replay(
        pkeys=out[4], pos=out[5], vals=_dev(real[None, :], np.float64),
        ops=_ops([SUM]), num_parts=512, tsize=tsize, agg_chunk=0,
    )
    gk, _, ga = _groups(rep)
    _check_sum_bound(keys, real, gk, ga[0])


@pytest.mark.parametrize("shape", KEY_SHAPES + ["same-narrow"])
def test_gb_partitioned_record_and_replay_key_shapes(shape):
    """The recording scatter and the replay aggregate on the key shapes
    every aggregating kernel gets; the wrap keys and the non-negative
    repeated key also go through the int32 replay."""
    n, tsize = 5000, 16384
    rng = np.random.default_rng(len(shape) + 21)
    if shape == "same-narrow":
        keys = np.full(n, 2**31 - 1, dtype=np.int64)
    else:
        keys = _key_shape(shape, n, tsize, rng)
    _, replays = _record_and_replay(keys, tsize, rng)
    assert replays == (2 if shape in ("wrap", "same-narrow") else 1)


@pytest.mark.parametrize("key", [None, 0, 12345, -5, I64_MAX])
def test_gb_partitioned_record_and_replay_empty_and_single_row(key):
    keys = np.array([] if key is None else [key], dtype=np.int64)
    _, replays = _record_and_replay(keys, 16, np.random.default_rng(1))
    assert replays == (2 if key in (None, 0, 12345) else 1)


# ------------------------------------------------------------------ #
# 5. reduce_columns                                                   #
# ------------------------------------------------------------------ #

REDUCE_N = [1, 63, 64, 65, 255, 257, 2049, 20_001]
FIVE_RED = [SUM, MIN, MAX, SUM, MIN]


def _check_reduce(vals, valids, ops):
    out, cnt = get_ext().reduce_columns(
        _dev(vals, np.float64),
        None if valids is None else _dev(valids, np.bool_), _ops(ops),
    )
    ro, rc = kr.reduce_cols_ref(vals, valids, ops)
    np.testing.assert_array_equal(_host(cnt), rc)
    got = _host(out)
    for a, op in enumerate(ops):
        if op == SUM:
            assert _bits(got[a]) == _bits(ro[a]), (a, got[a], ro[a])
        else:
            assert got[a] == ro[a], (a, got[a], ro[a])


@pytest.mark.parametrize("mask", ["none", "random", "dead-column"])
@pytest.mark.parametrize("n", REDUCE_N)
def test_reduce_columns_exact(n, mask):
    """Integer-valued columns: the matrix-core wave reduction, the
    shuffle trees and the cross-block atomics must give the exact sum."""
    rng = np.random.default_rng(n)
    vals = _int_vals(rng, 5, n)
    valids = None
    if mask != "none":
        valids = rng.random((5, n)) < 0.6
    if mask == "dead-column":
        valids[0] = False  # count 0, identities left in place
        valids[2] = False
    for k in (1, 5):
        _check_reduce(vals[:k], None if valids is None else valids[:k], FIVE_RED[:k])
    _check_reduce(vals[1:2], None if valids is None else valids[1:2], [MAX])


@pytest.mark.parametrize("n", [65, 2049])
def test_reduce_columns_infinities_and_zeros(n):
    rng = np.random.default_rng(n)
    vals = _int_vals(rng, 5, n)
    vals[0] = -0.0  # sums to +0.0: the accumulators start there
    vals[1, 7], vals[1, 9] = np.inf, -np.inf
    vals[2, 3], vals[2, 64] = -np.inf, np.inf
    vals[3, n - 1] = np.inf
    vals[4] = 0.0
    vals[4, 5] = -0.0
    _check_reduce(vals, None, FIVE_RED)
    valids = np.ones((5, n), dtype=bool)
    valids[1, 9] = valids[2, 64] = valids[3, n - 1] = False
    _check_reduce(vals, valids, FIVE_RED)


def test_reduce_columns_real_valued_sum():
    n = 20_001
    rng = np.random.default_rng(8)
    v = rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))
    out, cnt = get_ext().reduce_columns(
        _dev(v[None, :], np.float64), None, _ops([SUM])
    )
    assert int(cnt.item()) == n
    _check_sum_bound(
        np.zeros(n, dtype=np.int64), v, np.array([0]), _host(out)
    )


# ------------------------------------------------------------------ #
# 6. gb_key_stats                                                     #
# ------------------------------------------------------------------ #


def _dec(x: int) -> int:
    raw = (int(x) & kr.U64) ^ (1 << 63)  # undo the order-preserving bias
    return raw - (1 << 64) if raw >= (1 << 63) else raw


def _stats_columns(k: int, n: int, groups: int, seed: int):
    """k key columns cycling int64 / int16 / int32, every second one with
    a validity mask, whose row tuples take about ``groups`` values."""
    rng = np.random.default_rng(seed)
    code = rng.integers(0, groups, n)
    cols, valids = [], []
    for c in range(k):
        dt = [np.int64, np.int16, np.int32][c % 3]
        span = [40_000, 5, 300][c % 3]
        cols.append(((code // (c + 1)) % span - span // 3).astype(dt))
        valids.append(rng.random(n) < 0.9 if c % 2 == 1 else None)
    return cols, valids


def _key_stats(cols, valids, nsamples, tsize, do_minmax=True):
    st = get_ext().gb_key_stats(
        [_dev(c, c.dtype) for c in cols],
        [None if v is None else _dev(v, np.bool_) for v in valids],
        nsamples, tsize, do_minmax,
    )
    st = _host(st).tolist()
    k = len(cols)
    assert len(st) == 2 * k + 3
    return (
        [_dec(x) for x in st[0 : 2 * k : 2]],
        [_dec(x) for x in st[1 : 2 * k : 2]],
        tuple(st[2 * k :]),
    )


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 1000])
def test_gb_key_stats_unsampled(n, k):
    cols, valids = _stats_columns(k, n, 400, n + k)
    mins, maxs, dff = _key_stats(cols, valids, min(65536, n), 4096)
    rmins, rmaxs, d, f1, f2 = kr.key_stats_ref(cols, valids, min(65536, n))
    assert mins == rmins and maxs == rmaxs
    assert dff == (d, f1, f2)
    if n == 1000:
        assert f1 > 0 and f2 > 0 and d > f1 + f2
    # without min/max the leading slots are not written; d, f1, f2 are
    _, _, dff = _key_stats(cols, valids, min(65536, n), 4096, do_minmax=False)
    assert dff == (d, f1, f2)


def test_gb_key_stats_sampled():
    """n = 3 * 65536 + 17 at 65536 samples: stride 3, rows 0, 3, 6, ..;
    min and max still see every row."""
    n = 3 * 65536 + 17
    cols, valids = _stats_columns(3, n, 50_000, 5)
    cols[0][1], cols[0][n - 1] = -(2**50), 2**50  # rows the sample skips
    mins, maxs, dff = _key_stats(cols, valids, 65536, 131072)
    rmins, rmaxs, d, f1, f2 = kr.key_stats_ref(cols, valids, 65536)
    assert mins == rmins and maxs == rmaxs
    assert mins[0] == -(2**50) and maxs[0] == 2**50
    assert dff == (d, f1, f2)
    assert f1 > 0 and f2 > 0 and d < 65536


def test_gb_key_stats_int64_extremes():
    a = np.array([5, I64_MIN, -1, I64_MAX, 5, 0], dtype=np.int64)
    b = np.array([I64_MAX, I64_MAX, I64_MAX, I64_MIN, I64_MAX, 7], dtype=np.int64)
    c = np.array([-32768, 32767, 0, 1, -32768, -1], dtype=np.int16)
    mins, maxs, dff = _key_stats([a, b, c], [None] * 3, 6, 16)
    assert mins == [I64_MIN, I64_MIN, -32768]
    assert maxs == [I64_MAX, I64_MAX, 32767]
    assert dff == kr.key_stats_ref([a, b, c], [None] * 3, 6)[2:] == (5, 4, 1)


def test_limits_match_the_extension():
    """ops.py sizes its decisions by copies of two relational.h limits."""
    assert dops.PACK_MAX_COLS == get_ext().PACK_MAX_COLS == 8
    assert dops.GB_LDS_MAX_AGGS == get_ext().GB_LDS_MAX_AGGS == 4


def test_gb_key_stats_column_limit():
    cols, valids = _stats_columns(9, 100, 10, 1)
    with pytest.raises(RuntimeError, match="key columns"):
        _key_stats(cols, valids, 100, 256)
    with pytest.raises(RuntimeError, match="key columns"):
        get_ext().pack_columns(
            [_dev(c, c.dtype) for c in cols], [None] * 9, [0] * 9, list(range(9))
        )


# ------------------------------------------------------------------ #
# 7. pack_columns / unpack_column                                     #
# ------------------------------------------------------------------ #

# (dtype, lo, code width, nullable): value range lo .. lo + 2^width - 2
PACK_LAYOUTS = {
    1: [(np.int64, -(2**61), 63, True)],
    2: [(np.int32, -1000, 11, True), (np.int64, -5, 52, False)],
    8: [
        (np.int16, -9, 5, False), (np.int32, -(2**20), 7, True),
        (np.int64, -(2**45), 9, False), (np.int16, 32760, 3, True),
        (np.int32, 0, 11, "all"), (np.int64, 2**40, 8, True),
        (np.int16, -32768, 10, False), (np.int32, 2**31 - 1024, 10, True),
    ],
}


def _pack_case(k: int, n: int):
    rng = np.random.default_rng(100 * k + n)
    cols, valids, mins, widths = [], [], [], []
    for dt, lo, w, nullable in PACK_LAYOUTS[k]:
        hi = lo + 2**w - 2
        c = rng.integers(lo, hi, n, endpoint=True)
        if n >= 2:
            c[0], c[n - 1] = lo, hi
        cols.append(c.astype(dt))
        assert int(cols[-1].min()) >= lo and int(cols[-1].max()) <= hi
        if nullable == "all":
            valids.append(np.zeros(n, dtype=bool))
        else:
            valids.append(rng.random(n) < 0.8 if nullable else None)
        mins.append(lo)
        widths.append(w)
    assert sum(widths) == 63
    return cols, valids, mins, widths


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 257, 513, 9001])
def test_pack_unpack_columns(n, k):
    cols, valids, mins, widths = _pack_case(k, n)
    shifts = kr.pack_shifts(widths)
    packed = get_ext().pack_columns(
        [_dev(c, c.dtype) for c in cols],
        [None if v is None else _dev(v, np.bool_) for v in valids],
        mins, shifts,
    )
    exp = kr.pack_ref(cols, valids, mins, widths)
    np.testing.assert_array_equal(_host(packed), exp)
    # back out through the reference, then through the kernel
    ref_back = kr.unpack_ref(_host(packed), mins, widths)
    for c, v, (rd, rv), lo, w, sh in zip(cols, valids, ref_back, mins, widths, shifts):
        ok = np.ones(n, dtype=bool) if v is None else v
        np.testing.assert_array_equal(rv, ok)
        np.testing.assert_array_equal(rd[ok], c[ok].astype(np.int64))
        for has_nulls in (False, True):
            data, valid = get_ext().unpack_column(
                packed, sh, w, lo, c.dtype.itemsize, has_nulls
            )
            data = _host(data)
            assert data.dtype == c.dtype
            np.testing.assert_array_equal(data[ok], c[ok])
            if has_nulls:
                np.testing.assert_array_equal(_host(valid), ok)
            else:
                assert valid.numel() == 0


# ------------------------------------------------------------------ #
# 8. engine level: dops.groupby_aggregate                             #
# ------------------------------------------------------------------ #


def _frame(keys: dict, vals: dict):
    cols, fields = {}, []
    for name, a in keys.items():
        tp = {np.dtype("int64"): pa.int64(), np.dtype("int32"): pa.int32()}[a.dtype]
        cols[name] = DeviceColumn(_dev(a, a.dtype), None, tp)
        fields.append(pa.field(name, tp))
    for name, a in vals.items():
        cols[name] = DeviceColumn(_dev(a, np.float64), None, pa.float64())
        fields.append(pa.field(name, pa.float64()))
    return HipDataFrame.from_columns(cols, Schema(fields), "cuda")


def _check_engine(keys, vals, aggs, expected_groups):
    """``groupby_aggregate`` over one raw int64 key column against
    ``groupby_ref``: every group once, counts exact, sums bit-equal."""
    df = _frame({"k": keys}, {f"v{i}": v for i, v in enumerate(vals)})
    ok, oa, oc, meta = dops.groupby_aggregate(
        df, ["k"], aggs, expected_groups=expected_groups
    )
    assert meta is None
    ops = [op for _, op, _ in aggs]
    src = np.stack([vals[int(c[1:])] for c, _, _ in aggs])
    rk, rc, ra = kr.groupby_ref(keys, src, None, ops)
    gk = _host(ok)
    order = np.argsort(gk, kind="stable")
    np.testing.assert_array_equal(gk[order], rk)
    np.testing.assert_array_equal(_host(oc)[order], rc)
    for a, (_, op, name) in enumerate(aggs):
        got = _host(oa[name])[order]
        if op in (SUM, COUNT):
            np.testing.assert_array_equal(_bits(got), _bits(ra[a]), err_msg=name)
        else:
            np.testing.assert_array_equal(got, ra[a], err_msg=name)
    return rk, rc


SENTINEL_AGGS = {
    "lds": [("v0", SUM, "s"), ("v1", COUNT, "c")],
    "hbm": [("v0", SUM, "s"), ("v0", MIN, "lo"), ("v1", MAX, "hi")],
}


@pytest.mark.parametrize("path", ["lds", "hbm"])
def test_groupby_sentinel_key_small_table(path):
    """A null-free int64 key column holding GB_EMPTY (INT64_MIN): the
    group is there with its exact count and aggregates, and its
    neighbours INT64_MIN + 1, 0 and INT64_MAX are untouched."""
    rng = np.random.default_rng(12)
    pool = np.array([I64_MIN, I64_MIN + 1, 0, I64_MAX], dtype=np.int64)
    keys = pool[rng.integers(0, 4, 600)]
    keys[:3] = I64_MIN
    vals = _int_vals(rng, 2, 600)
    rk, rc = _check_engine(keys, vals, SENTINEL_AGGS[path], 4)
    assert rk.tolist() == pool.tolist() and rc[0] >= 3


def test_groupby_sentinel_key_only():
    keys = np.full(5, I64_MIN, dtype=np.int64)
    vals = np.arange(10.0).reshape(2, 5)
    rk, rc = _check_engine(keys, vals, SENTINEL_AGGS["hbm"], 4)
    assert rk.tolist() == [I64_MIN] and rc.tolist() == [5]


def test_groupby_sentinel_key_partitioned():
    """20 000 rows of distinct keys at expected_groups = 100 001 take the
    partitioned path; the few GB_EMPTY rows form one more group."""
    rng = np.random.default_rng(13)
    n = 20_000
    keys = _key_shape("distinct", n, 4 * n, rng)
    keys[:4] = [I64_MIN + 1, 0, I64_MAX, -1]
    keys[[10, 4097, n - 1]] = I64_MIN
    vals = _int_vals(rng, 1, n)
    rk, rc = _check_engine(keys, vals, [("v0", SUM, "s")], 100_001)
    assert rk[0] == I64_MIN and rc[0] == 3 and len(rk) == n - 2


@pytest.mark.parametrize("n_aggs", [5, 6])
def test_groupby_many_sum_count_aggregates_high_cardinality(n_aggs):
    """More SUM/COUNT aggregates than the per-partition LDS table holds,
    at a group estimate that would otherwise take the partitioned path."""
    rng = np.random.default_rng(n_aggs)
    n = 20_000
    pool = _key_shape("distinct", 5000, 20_000, rng)
    keys = pool[rng.integers(0, 5000, n)]
    vals = _int_vals(rng, 3, n)
    aggs = [("v0", SUM, "s0"), ("v1", SUM, "s1"), ("v2", COUNT, "c2"),
            ("v2", SUM, "s2"), ("v0", COUNT, "c0"), ("v1", SUM, "s1b")][:n_aggs]
    _check_engine(keys, vals, aggs, 100_001)


def test_groupby_nine_key_columns():
    """More key columns than one pack launch takes: the torch packing
    path handles them, and the result equals pandas."""
    rng = np.random.default_rng(9)
    n = 5000
    keys = {f"k{i}": rng.integers(-1, 2, n).astype(np.int32) for i in range(9)}
    v = _int_vals(rng, 1, n)[0]
    df = _frame(keys, {"v": v})
    names = list(keys)
    ok, oa, oc, meta = dops.groupby_aggregate(df, names, [("v", SUM, "s")])
    cols = dops.unpack_keys(ok, meta, [df.col(c) for c in names])
    got = pd.DataFrame({c: _host(col.data) for c, col in zip(names, cols)})
    assert all(col.valid is None for col in cols)
    got["s"] = _host(oa["s"])
    got["n"] = _host(oc)
    pdf = pd.DataFrame(keys)
    pdf["v"] = v
    exp = pdf.groupby(names, as_index=False).agg(s=("v", "sum"), n=("v", "size"))
    got = got.sort_values(names).reset_index(drop=True)
    exp = exp.sort_values(names).reset_index(drop=True)
    assert len(exp) > 1000
    pd.testing.assert_frame_equal(got, exp, check_dtype=False, check_exact=True)
