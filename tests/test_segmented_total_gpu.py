"""GPU tests of the whole-partition kernels (``seg_total_*``) against the
torch-CPU implementation of the ops layer, which
``test_segmented_total.py`` pins to pandas.  Every size derives from the
kernels' chunk size, the block size and the wave size."""
from typing import Optional

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine
from fugue_amd.hip.ext import get_ext
from fugue_amd.hip.frame import HipDataFrame
from fugue_amd.sql.api import fugue_sql

C = int(get_ext().seg_rank_chunk())
BLOCK = 256
WAVE = 64
SIZES = [
    1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1,
    C - 1, C, C + 1, 3 * C + 17,
]
LAYOUTS = ["one", "singletons", "chunk-start", "chunk-end", "random"]
NULLS = ["none", "random", "straddle", "segment"]
FUNCS = ["sum", "min", "max", "first", "last"]
U = 2.0 ** -53


def _heads(layout: str, n: int, rng: np.random.Generator) -> np.ndarray:
    """Sorted positions at which a new partition starts; the last
    partition always ends at n - 1."""
    if layout == "one":
        return np.array([0])
    if layout == "singletons":
        return np.arange(n)
    if layout == "chunk-start":
        return np.arange(0, n, C)
    if layout == "chunk-end":
        # a one-row partition on a chunk's first position, and partitions
        # whose last row is a chunk's last and first position
        h = {0}
        for c0 in range(0, n, C):
            h.update((c0, c0 + C // 3, c0 + 1))
        return np.array(sorted(x for x in h if x < n))
    lens = rng.integers(1, 201, size=n)
    starts = np.concatenate([[0], np.cumsum(lens)])
    return starts[starts < n]


def _sorted_valid(
    nulls: str, n: int, seg: np.ndarray, rng: np.random.Generator
) -> Optional[np.ndarray]:
    """Validity per SORTED position."""
    if nulls == "none":
        return None
    ok = np.ones(n, dtype=bool)
    if nulls == "random":
        ok = rng.random(n) >= 0.3
    elif nulls == "straddle":
        # a null run across a chunk boundary (or the middle, when the
        # input is shorter than a chunk)
        mid = C if n > C + 5 else n // 2
        ok[max(mid - 5, 0) : mid + 5] = False
    else:
        # every row of the middle position's partition is null
        ok[seg == seg[n // 2]] = False
    return ok


def _case(layout: str, n: int, seed: int, nulls: str = "none"):
    """perm, pkeys, an int value column and its validity (or None), all
    in original row order, plus the partition id per sorted position."""
    rng = np.random.default_rng(seed)
    heads = _heads(layout, n, rng)
    flag = np.zeros(n, dtype=np.int64)
    flag[heads] = 1
    seg = np.cumsum(flag) - 1
    perm = rng.permutation(n)
    ids = rng.permutation(len(heads)).astype(np.int64) * 7919 - 3
    pkeys = np.empty(n, dtype=np.int64)
    pkeys[perm] = ids[seg]
    vals = rng.integers(-1000, 1001, size=n)
    ok = _sorted_valid(nulls, n, seg, rng)
    valid = None
    if ok is not None:
        v = np.empty(n, dtype=bool)
        v[perm] = ok
        valid = torch.from_numpy(v)
    return (
        torch.from_numpy(perm.astype(np.int64)),
        torch.from_numpy(pkeys),
        torch.from_numpy(vals),
        valid,
        seg,
    )


def _gpu(t: Optional["torch.Tensor"]) -> Optional["torch.Tensor"]:
    return None if t is None else t.cuda()


def _check_totals(perm, pkeys, vals, valid, tag, funcs=FUNCS) -> None:
    gp, gk, gval = perm.cuda(), pkeys.cuda(), _gpu(valid)
    for is_float in (False, True):
        # integer-valued doubles far below 2^53: every summation order
        # is exact, so the float results are compared bit for bit too
        data = vals.to(torch.float64) if is_float else vals
        for func in funcs:
            exp_acc, exp_cnt = dops.segmented_total(
                perm, pkeys, (data, valid), func
            )
            acc, cnt = dops.segmented_total(gp, gk, (data.cuda(), gval), func)
            assert acc.is_cuda and acc.dtype == data.dtype
            assert cnt.dtype == torch.int64
            assert torch.equal(cnt.cpu(), exp_cnt), (func, is_float, tag)
            if is_float and func in ("min", "max"):
                # numeric comparison: 0.0 == -0.0
                assert bool((acc.cpu() == exp_acc).all()), (func, tag)
            else:
                assert torch.equal(acc.cpu(), exp_acc), (func, is_float, tag)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_total_sizes_layouts_nulls(n, layout):
    for nulls in NULLS:
        perm, pkeys, vals, valid, _ = _case(
            layout, n, seed=n * 31 + len(layout), nulls=nulls
        )
        _check_totals(perm, pkeys, vals, valid, (layout, n, nulls))


def test_chunk_scans_span_more_than_one_tile():
    # more chunks than one tile of either single-block scan holds
    n = C * (BLOCK + 3) + 17
    perm, pkeys, vals, valid, _ = _case("random", n, seed=99, nulls="random")
    _check_totals(perm, pkeys, vals, valid, "tiles", funcs=["sum", "first", "last"])


def test_long_single_partition_over_many_tiles():
    # one partition over more chunks than a scan tile: the forward carry
    # and the backward "end not seen yet" both have to survive endless
    # chunks AND the tile boundary of their chunk scans
    n = C * (BLOCK + 2) + 1
    perm = torch.arange(n, dtype=torch.int64, device="cuda")
    pkeys = torch.zeros(n, dtype=torch.int64, device="cuda")
    g = torch.Generator().manual_seed(3)
    vals = torch.randint(-1000, 1001, (n,), generator=g).cuda()
    acc, cnt = dops.segmented_total(perm, pkeys, (vals, None), "sum")
    assert bool((cnt == n).all())
    assert bool((acc == vals.sum()).all())
    # |sum| <= 1000 n < 2^53: exact in double in any order
    acc, _ = dops.segmented_total(perm, pkeys, (vals.double(), None), "sum")
    assert bool((acc == vals.sum().double()).all())
    acc, _ = dops.segmented_total(perm, pkeys, (vals, None), "min")
    assert bool((acc == vals.min()).all())
    acc, _ = dops.segmented_total(perm, pkeys, (vals.double(), None), "max")
    assert bool((acc == vals.max().double()).all())
    # nulls everywhere but one row per chunk
    valid = (perm % C) == 5
    acc, cnt = dops.segmented_total(perm, pkeys, (vals, valid), "first")
    assert bool((cnt == (n + C - 6) // C).all())
    assert bool((acc == vals[5]).all())
    acc, _ = dops.segmented_total(perm, pkeys, (vals, valid), "last")
    assert bool((acc == vals[(n - 6) // C * C + 5]).all())


def test_integer_sum_wraps_and_extremes_are_not_sentinels():
    big = np.iinfo(np.int64).max
    perm = torch.arange(6, dtype=torch.int64)
    pkeys = torch.tensor([0, 0, 0, 1, 1, 1])
    vals = torch.tensor([big, 0, 1, -big - 1, big, -big - 1])
    valid = torch.tensor([True, False, True, True, False, True])
    for func in FUNCS:
        exp_acc, exp_cnt = dops.segmented_total(perm, pkeys, (vals, valid), func)
        acc, cnt = dops.segmented_total(
            perm.cuda(), pkeys.cuda(), (vals.cuda(), valid.cuda()), func
        )
        assert torch.equal(acc.cpu(), exp_acc), func
        assert torch.equal(cnt.cpu(), exp_cnt), func
    acc, _ = dops.segmented_total(
        perm.cuda(), pkeys.cuda(), (vals.cuda(), valid.cuda()), "sum"
    )
    assert acc.cpu().tolist() == [-big - 1] * 3 + [0] * 3
    acc, _ = dops.segmented_total(
        perm.cuda(), pkeys.cuda(), (vals.cuda(), valid.cuda()), "max"
    )
    assert acc.cpu().tolist() == [big] * 3 + [-big - 1] * 3
    inf = float("inf")
    f = torch.tensor([inf, 0.0, -inf, float("nan"), float("nan"), inf], dtype=torch.float64)
    acc, cnt = dops.segmented_total(perm.cuda(), pkeys.cuda(), (f.cuda(), None), "min")
    assert acc.cpu().tolist() == [-inf] * 3 + [inf] * 3
    assert cnt.cpu().tolist() == [3] * 3 + [1] * 3  # NaN counts as null
    acc, _ = dops.segmented_total(perm.cuda(), pkeys.cuda(), (f.cuda(), None), "first")
    assert acc.cpu().tolist() == [inf] * 6


def _fractional_case():
    """A float column of wide dynamic range on random partitions, and per
    sorted position: the sequential sum of its partition, the sum of |v|,
    the non-null count, and the partition's last sorted position."""
    n = 3 * C + 17
    perm, pkeys, _, valid, seg = _case("random", n, seed=21, nulls="random")
    rng = np.random.default_rng(21)
    v = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    ok = valid.numpy()[perm.numpy()]
    vz = np.where(ok, v, 0.0)
    ref = np.empty(n)
    ref_abs = np.empty(n)
    m = np.empty(n, dtype=np.int64)
    last = np.empty(n, dtype=np.int64)
    starts = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
    for s, e in zip(starts, np.r_[starts[1:], n]):
        ref[s:e] = np.cumsum(vz[s:e])[-1]
        ref_abs[s:e] = np.sum(np.abs(vz[s:e]))
        m[s:e] = np.sum(ok[s:e])
        last[s:e] = e - 1
    data = np.empty(n)
    data[perm.numpy()] = v
    return perm, pkeys, torch.from_numpy(data), valid, ref, ref_abs, m, last


def test_fractional_float_sum():
    perm, pkeys, data, valid, ref, ref_abs, m, last = _fractional_case()
    args = (perm.cuda(), pkeys.cuda(), (data.cuda(), valid.cuda()))
    p = perm.numpy()
    for func in ("sum", "min", "max"):
        acc, cnt = dops.segmented_total(*args, func)
        racc, rcnt = dops.segmented_scan(*args, func)
        bits = acc.view(torch.int64).cpu().numpy()[p]
        rbits = racc.view(torch.int64).cpu().numpy()[p]
        # all rows of a partition are bit-identical, and each holds the
        # bits the running scan ends on
        np.testing.assert_array_equal(bits, bits[last], err_msg=func)
        np.testing.assert_array_equal(bits, rbits[last], err_msg=func)
        np.testing.assert_array_equal(
            cnt.cpu().numpy()[p], rcnt.cpu().numpy()[p][last]
        )
    acc, cnt = dops.segmented_total(*args, "sum")
    got = acc.cpu().numpy()[p]
    np.testing.assert_array_equal(cnt.cpu().numpy()[p], m)
    # (m-1) u sum|v| bounds the error of ANY summation order; taken once
    # for the kernel's tree and once for the sequential reference
    bound = 2.0 * m * U * ref_abs
    err = np.abs(got - ref)
    print("float total: max err/bound", float(np.max(err / np.maximum(bound, 1e-300))))
    assert bool(np.all(err <= bound))


def test_two_runs_are_bit_identical():
    perm, pkeys, data, valid, *_ = _fractional_case()
    args = (perm.cuda(), pkeys.cuda(), (data.cuda(), valid.cuda()))
    for func in ("sum", "last"):
        a1, c1 = dops.segmented_total(*args, func)
        a2, c2 = dops.segmented_total(*args, func)
        assert torch.equal(a1.view(torch.int64), a2.view(torch.int64))
        assert torch.equal(c1, c2)


def test_empty_input_launches_nothing():
    z = torch.zeros(0, dtype=torch.int64, device="cuda")
    for func in FUNCS:
        acc, cnt = dops.segmented_total(z, z, (z, None), func)
        assert acc.numel() == 0 and cnt.numel() == 0
    with pytest.raises(RuntimeError):
        get_ext().seg_total(z, z, z, None, 5)


# ------------------------------------------------------------------ #
# end to end on the GPU engine                                         #
# ------------------------------------------------------------------ #
def _e2e_frame() -> pd.DataFrame:
    rng = np.random.default_rng(3)
    n = 100_003
    pdf = pd.DataFrame(
        dict(
            k=rng.integers(0, 2000, n),
            o=rng.permutation(n),
            v=rng.integers(-500, 500, n).astype(np.float64),
        )
    )
    pdf["v"] = pdf["v"].mask(pdf.index % 11 == 0)
    return pdf


def test_sql_partition_totals():
    pdf = _e2e_frame()
    e = HipExecutionEngine()
    sql = (
        "SELECT k, o, v, SUM(v) OVER (PARTITION BY k) AS s, "
        "COUNT(*) OVER (PARTITION BY k) AS n, "
        "AVG(v) OVER (PARTITION BY k) AS m FROM df"
    )
    res = fugue_sql(sql, df=e.to_df(pdf), engine=e, as_fugue=True)
    assert e.stats.get("window.device_partition") == 3
    assert e.stats.get("window.device") == 0
    assert e.stats.get("window.device_value") == 0
    assert isinstance(res, HipDataFrame)
    assert res.schema == "k:long,o:long,v:double,s:double,n:long,m:double"
    g = pdf.groupby("k", sort=False)
    # integer-valued doubles: the sum is exact, and so is sum / count
    s, c = g["v"].transform("sum"), g["v"].transform("count")
    exp = pdf.assign(s=s, n=g["k"].transform("size"), m=s / c)
    pd.testing.assert_frame_equal(res.as_pandas(), exp, check_dtype=False)


def test_sql_first_and_last_value():
    pdf = _e2e_frame()
    e = HipExecutionEngine()
    sql = (
        "SELECT k, o, v, FIRST_VALUE(v) OVER (PARTITION BY k ORDER BY o) AS f, "
        "LAST_VALUE(v) OVER (PARTITION BY k ORDER BY o) AS l FROM df"
    )
    res = fugue_sql(sql, df=e.to_df(pdf), engine=e, as_fugue=True)
    assert e.stats.get("window.device_partition") == 2
    assert e.stats.get("window.device") == 0
    assert e.stats.get("window.device_value") == 0
    assert isinstance(res, HipDataFrame)
    g = pdf.sort_values("o", kind="stable").groupby("k", sort=False)["v"]
    exp = pdf.assign(
        f=g.transform("first").sort_index(), l=g.transform("last").sort_index()
    )
    pd.testing.assert_frame_equal(res.as_pandas(), exp, check_dtype=False)
