"""GPU tests of the value-window kernels (``seg_shift`` / ``seg_scan_*``)
against the torch-CPU implementation of the ops layer, which
``test_segmented_scan.py`` pins to pandas.  Every size derives from the
kernels' chunk size, the block size and the wave size."""
from typing import Dict, List, Optional, Tuple

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
FUNCS = ["sum", "min", "max"]
U = 2.0 ** -53


def _heads(layout: str, n: int, rng: np.random.Generator) -> np.ndarray:
    """Sorted positions at which a new segment starts."""
    if layout == "one":
        return np.array([0])
    if layout == "singletons":
        return np.arange(n)
    if layout == "chunk-start":
        return np.arange(0, n, C)
    if layout == "chunk-end":
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
        # every row of the middle position's segment is null
        ok[seg == seg[n // 2]] = False
    return ok


def _case(layout: str, n: int, seed: int, nulls: str = "none"):
    """perm, pkeys, an int value column and its validity (or None), all
    in original row order, plus the segment id per sorted position."""
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


def _check_scans(perm, pkeys, vals, valid, tag) -> None:
    gp, gk, gval = perm.cuda(), pkeys.cuda(), _gpu(valid)
    for is_float in (False, True):
        # integer-valued doubles far below 2^53: every summation order
        # is exact, so the float results are compared bit for bit too
        data = vals.to(torch.float64) if is_float else vals
        for func in FUNCS:
            exp_acc, exp_cnt = dops.segmented_scan(
                perm, pkeys, (data, valid), func
            )
            acc, cnt = dops.segmented_scan(gp, gk, (data.cuda(), gval), func)
            assert acc.is_cuda and acc.dtype == data.dtype
            assert cnt.dtype == torch.int64
            assert torch.equal(cnt.cpu(), exp_cnt), (func, is_float, tag)
            if is_float and func != "sum":
                # numeric comparison: 0.0 == -0.0
                assert bool((acc.cpu() == exp_acc).all()), (func, tag)
            else:
                assert torch.equal(acc.cpu(), exp_acc), (func, is_float, tag)


def _check_shift(perm, pkeys, vals, valid, offsets, tag) -> None:
    gp, gk, gval = perm.cuda(), pkeys.cuda(), _gpu(valid)
    for is_float in (False, True):
        data = vals.to(torch.float64) if is_float else vals
        for d in offsets:
            exp, exp_ok = dops.segmented_shift(perm, pkeys, (data, valid), d)
            got, ok = dops.segmented_shift(gp, gk, (data.cuda(), gval), d)
            assert got.dtype == data.dtype and ok.dtype == torch.bool
            assert torch.equal(ok.cpu(), exp_ok), (d, is_float, tag)
            assert torch.equal(got.cpu(), exp), (d, is_float, tag)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_scan_and_shift_sizes_layouts_nulls(n, layout):
    for nulls in NULLS:
        perm, pkeys, vals, valid, _ = _case(
            layout, n, seed=n * 31 + len(layout), nulls=nulls
        )
        _check_scans(perm, pkeys, vals, valid, (layout, n, nulls))
        _check_shift(perm, pkeys, vals, valid, [1, -1], (layout, n, nulls))


@pytest.mark.parametrize("layout", ["one", "random", "chunk-end"])
def test_shift_offsets(layout):
    n = 3 * C + 17
    perm, pkeys, vals, valid, _ = _case(layout, n, seed=7, nulls="random")
    offsets = [0]
    for d in (1, WAVE, BLOCK + 1, C, C + 1, n, n + 5, 2 ** 62):
        offsets += [d, -d]
    _check_shift(perm, pkeys, vals, valid, offsets, layout)
    # d = 0 is the identity on values and validity
    got, ok = dops.segmented_shift(perm.cuda(), pkeys.cuda(), (vals.cuda(), valid.cuda()), 0)
    assert torch.equal(got.cpu(), vals) and torch.equal(ok.cpu(), valid)
    # |d| >= n: no row has a source
    for d in (n, -n):
        _, ok = dops.segmented_shift(perm.cuda(), pkeys.cuda(), (vals.cuda(), None), d)
        assert not bool(ok.any())


def test_shift_lands_in_original_row_order():
    n = C + WAVE + 1
    perm, pkeys, vals, _, seg = _case("random", n, seed=5)
    got, ok = dops.segmented_shift(perm.cuda(), pkeys.cuda(), (vals.cuda(), None), 1)
    # recompute from the sorted side and scatter by hand
    sv = vals.numpy()[perm.numpy()]
    exp = np.zeros(n, dtype=np.int64)
    exp_ok = np.zeros(n, dtype=bool)
    same = seg[1:] == seg[:-1]
    exp[perm.numpy()[1:][same]] = sv[:-1][same]
    exp_ok[perm.numpy()[1:][same]] = True
    np.testing.assert_array_equal(ok.cpu().numpy(), exp_ok)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)


def test_chunk_scan_spans_more_than_one_tile():
    # more chunks than one tile of the single-block scan holds
    n = C * (BLOCK + 3) + 17
    perm, pkeys, vals, valid, _ = _case("random", n, seed=99, nulls="random")
    gp, gk = perm.cuda(), pkeys.cuda()
    for func, data in (("sum", vals), ("min", vals.to(torch.float64))):
        exp_acc, exp_cnt = dops.segmented_scan(perm, pkeys, (data, valid), func)
        acc, cnt = dops.segmented_scan(gp, gk, (data.cuda(), valid.cuda()), func)
        assert torch.equal(cnt.cpu(), exp_cnt)
        assert torch.equal(acc.cpu(), exp_acc)


def test_long_single_segment_over_many_tiles():
    # one segment over more chunks than a scan tile: the carry has to
    # survive headless chunks AND the tile boundary of the chunk scan
    n = C * (BLOCK + 2) + 1
    perm = torch.arange(n, dtype=torch.int64, device="cuda")
    pkeys = torch.zeros(n, dtype=torch.int64, device="cuda")
    g = torch.Generator().manual_seed(3)
    vals = torch.randint(-1000, 1001, (n,), generator=g).cuda()
    acc, cnt = dops.segmented_scan(perm, pkeys, (vals, None), "sum")
    assert torch.equal(cnt, perm + 1)
    assert torch.equal(acc, torch.cumsum(vals, 0))
    # |sum| <= 1000 n < 2^53: exact in double in any order
    acc, _ = dops.segmented_scan(perm, pkeys, (vals.double(), None), "sum")
    assert torch.equal(acc, torch.cumsum(vals, 0).double())
    acc, _ = dops.segmented_scan(perm, pkeys, (vals, None), "min")
    assert torch.equal(acc, torch.cummin(vals, 0).values)
    acc, _ = dops.segmented_scan(perm, pkeys, (vals.double(), None), "max")
    assert torch.equal(acc, torch.cummax(vals, 0).values.double())
    # nulls everywhere but one row per chunk: the count crosses chunks
    valid = (perm % C) == 5
    acc, cnt = dops.segmented_scan(perm, pkeys, (vals, valid), "sum")
    assert torch.equal(cnt, (perm + C - 5) // C)
    assert torch.equal(acc, torch.cumsum(vals * valid, 0))


def test_integer_sum_wraps_and_extremes_are_not_sentinels():
    big = np.iinfo(np.int64).max
    perm = torch.arange(6, dtype=torch.int64)
    pkeys = torch.tensor([0, 0, 0, 1, 1, 1])
    vals = torch.tensor([big, 0, 1, -big - 1, big, -big - 1])
    valid = torch.tensor([True, False, True, True, False, True])
    for func in FUNCS:
        exp_acc, exp_cnt = dops.segmented_scan(perm, pkeys, (vals, valid), func)
        acc, cnt = dops.segmented_scan(
            perm.cuda(), pkeys.cuda(), (vals.cuda(), valid.cuda()), func
        )
        assert torch.equal(acc.cpu(), exp_acc), func
        assert torch.equal(cnt.cpu(), exp_cnt), func
    acc, _ = dops.segmented_scan(
        perm.cuda(), pkeys.cuda(), (vals.cuda(), valid.cuda()), "sum"
    )
    assert acc.cpu().tolist() == [big, big, -big - 1, -big - 1, -big - 1, 0]
    inf = float("inf")
    f = torch.tensor([inf, 0.0, -inf, float("nan"), 2.0, 1.0], dtype=torch.float64)
    acc, cnt = dops.segmented_scan(perm.cuda(), pkeys.cuda(), (f.cuda(), None), "min")
    assert acc.cpu().tolist() == [inf, 0.0, -inf, 0.0, 2.0, 1.0]
    assert cnt.cpu().tolist() == [1, 2, 3, 0, 1, 2]  # NaN counts as null


def test_two_runs_are_bit_identical():
    n = 3 * C + 17
    perm, pkeys, _, valid, _ = _case("random", n, seed=13, nulls="random")
    rng = np.random.default_rng(13)
    data = torch.from_numpy(rng.standard_normal(n) * 1e3).cuda()
    gp, gk, gv = perm.cuda(), pkeys.cuda(), valid.cuda()
    a1, c1 = dops.segmented_scan(gp, gk, (data, gv), "sum")
    a2, c2 = dops.segmented_scan(gp, gk, (data, gv), "sum")
    assert torch.equal(a1.view(torch.int64), a2.view(torch.int64))
    assert torch.equal(c1, c2)


def _fractional_case():
    """Sorted-side reference of a running float sum: sequential sum, the
    running sum of |v| and the non-null count per sorted position."""
    n = 3 * C + 17
    perm, pkeys, _, valid, seg = _case("random", n, seed=21, nulls="random")
    rng = np.random.default_rng(21)
    v = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    ok = valid.numpy()[perm.numpy()]
    vz = np.where(ok, v, 0.0)
    ref = np.empty(n)
    ref_abs = np.empty(n)
    m = np.empty(n, dtype=np.int64)
    starts = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
    for s, e in zip(starts, np.r_[starts[1:], n]):
        ref[s:e] = np.cumsum(vz[s:e])
        ref_abs[s:e] = np.cumsum(np.abs(vz[s:e]))
        m[s:e] = np.cumsum(ok[s:e])
    data = np.empty(n)
    data[perm.numpy()] = v
    return perm, pkeys, torch.from_numpy(data), valid, ref, ref_abs, m


def test_fractional_float_sum_within_summation_bound():
    perm, pkeys, data, valid, ref, ref_abs, m = _fractional_case()
    acc, cnt = dops.segmented_scan(
        perm.cuda(), pkeys.cuda(), (data.cuda(), valid.cuda()), "sum"
    )
    got = acc.cpu().numpy()[perm.numpy()]
    np.testing.assert_array_equal(cnt.cpu().numpy()[perm.numpy()], m)
    # (m-1) u sum|v| bounds the error of ANY summation order; taken once
    # for the kernel's tree and once for the sequential reference
    bound = 2.0 * m * U * ref_abs
    err = np.abs(got - ref)
    print("float sum: max err/bound", float(np.max(err / np.maximum(bound, 1e-300))))
    assert bool(np.all(err <= bound))


def test_engine_avg_within_summation_bound():
    perm, pkeys, data, valid, ref, ref_abs, m = _fractional_case()
    n = perm.numel()
    order = torch.empty(n, dtype=torch.int64)
    order[perm] = torch.arange(n)
    pdf = pd.DataFrame(
        dict(
            k=pkeys.numpy(),
            o=order.numpy(),
            v=np.where(valid.numpy(), data.numpy(), np.nan),
        )
    )
    e = HipExecutionEngine()
    res = e.window_over(
        e.to_df(pdf), ["k"], [("o", True)], [("a", "avg", "v", None, None)]
    )
    assert isinstance(res, HipDataFrame)
    assert e.stats.get("window.device_value") == 1
    out = res.as_pandas()
    got = out["a"].to_numpy()[perm.numpy()]
    some = m > 0
    assert bool(np.all(np.isnan(got) == ~some))
    exp = ref[some] / m[some]
    bound = 2.0 * m[some] * U * ref_abs[some] / m[some] + 2.0 * U * np.abs(exp)
    err = np.abs(got[some] - exp)
    print("avg: max err/bound", float(np.max(err / np.maximum(bound, 1e-300))))
    assert bool(np.all(err <= bound))


def test_empty_input_launches_nothing():
    z = torch.zeros(0, dtype=torch.int64, device="cuda")
    acc, cnt = dops.segmented_scan(z, z, (z, None), "sum")
    assert acc.numel() == 0 and cnt.numel() == 0
    data, ok = dops.segmented_shift(z, z, (z, None), 1)
    assert data.numel() == 0 and ok.numel() == 0


# ------------------------------------------------------------------ #
# end to end on the GPU engine                                         #
# ------------------------------------------------------------------ #
def test_sql_lag_and_running_sum():
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
    e = HipExecutionEngine()
    sql = (
        "SELECT k, o, v, LAG(v) OVER (PARTITION BY k ORDER BY o) AS p, "
        "SUM(v) OVER (PARTITION BY k ORDER BY o) AS s FROM df"
    )
    res = fugue_sql(sql, df=e.to_df(pdf), engine=e, as_fugue=True)
    assert e.stats.get("window.device_value") == 2
    assert e.stats.get("window.device") == 0
    assert isinstance(res, HipDataFrame)
    g = pdf.sort_values("o", kind="stable").groupby("k", sort=False)["v"]
    exp = pdf.assign(p=g.shift(1).sort_index(), s=g.cumsum().sort_index())
    # integer-valued doubles: the running sum is exact; row order is kept
    pd.testing.assert_frame_equal(res.as_pandas(), exp, check_dtype=False)
