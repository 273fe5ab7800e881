"""GPU tests of the moving-frame kernel (``seg_frame``) against the
torch-CPU implementation of the ops layer, which ``test_window_frames.py``
pins to a brute-force double loop.  Every size derives from the kernel's
tile and reach limits, the block size and the wave size."""
from typing import Optional

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

from fugue_amd.execution.native_execution_engine import NativeExecutionEngine
from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine
from fugue_amd.hip.ext import get_ext
from fugue_amd.hip.frame import HipDataFrame
from fugue_amd.sql.api import fugue_sql

T = int(get_ext().seg_frame_tile())
R = int(get_ext().seg_frame_max_reach())
BLOCK = 256
WAVE = 64
SIZES = [
    1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1,
    T - 1, T, T + 1, 3 * T + 17,
]
LAYOUTS = ["one", "singletons", "tile-start", "tile-end", "random"]
NULLS = ["none", "random", "straddle", "segment"]
FUNCS = ["sum", "min", "max", "first", "last"]
FRAMES = [(0, 0), (-1, 0), (0, 1), (-3, -1), (2, 5), (-64, 64)]


def _heads(layout: str, n: int, rng: np.random.Generator) -> np.ndarray:
    """Sorted positions at which a new segment starts."""
    if layout == "one":
        return np.array([0])
    if layout == "singletons":
        return np.arange(n)
    if layout == "tile-start":
        return np.arange(0, n, T)
    if layout == "tile-end":
        h = {0}
        for t0 in range(0, n, T):
            h.update((t0, t0 + T // 3, t0 + 1))
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
        # a null run across a tile boundary (or the middle, when the
        # input is shorter than a tile)
        mid = T if n > T + 5 else n // 2
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


def _check_frames(perm, pkeys, vals, valid, frames, funcs, tag) -> None:
    gp, gk, gval = perm.cuda(), pkeys.cuda(), _gpu(valid)
    for is_float in (False, True):
        # integer-valued doubles far below 2^53, added in the same order
        # on both sides: the float results are compared exactly too
        data = vals.to(torch.float64) if is_float else vals
        gdata = data.cuda()
        for lo, hi in frames:
            for func in funcs:
                exp_acc, exp_cnt = dops.segmented_frame(
                    perm, pkeys, (data, valid), func, lo, hi
                )
                acc, cnt = dops.segmented_frame(
                    gp, gk, (gdata, gval), func, lo, hi
                )
                assert acc.is_cuda and acc.dtype == data.dtype
                assert cnt.dtype == torch.int64
                what = (func, lo, hi, is_float, tag)
                assert torch.equal(cnt.cpu(), exp_cnt), what
                if is_float and func in ("min", "max"):
                    # numeric comparison: 0.0 == -0.0
                    assert bool((acc.cpu() == exp_acc).all()), what
                else:
                    assert torch.equal(acc.cpu(), exp_acc), what


def test_limits_match_the_python_copies():
    assert R == dops.SEG_FRAME_MAX_REACH
    assert R >= 255 and T >= BLOCK


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_frame_sizes_layouts_nulls(n, layout):
    for nulls in NULLS:
        perm, pkeys, vals, valid, _ = _case(
            layout, n, seed=n * 37 + len(layout), nulls=nulls
        )
        _check_frames(perm, pkeys, vals, valid, FRAMES, FUNCS, (layout, n, nulls))
        # (0, 0) is the identity on values and validity
        ok = valid if valid is not None else torch.ones(n, dtype=torch.bool)
        for func in FUNCS:
            acc, cnt = dops.segmented_frame(
                perm.cuda(), pkeys.cuda(), (vals.cuda(), _gpu(valid)), func, 0, 0
            )
            assert torch.equal(cnt.cpu(), ok.to(torch.int64))
            assert torch.equal(acc.cpu(), torch.where(ok, vals, torch.zeros_like(vals)))


@pytest.mark.parametrize("layout", ["random", "one"])
def test_halo_limits(layout):
    n = 3 * T + 17
    perm, pkeys, vals, valid, _ = _case(layout, n, seed=13, nulls="random")
    frames = [(-R, 0), (0, R), (-(R // 2), R - R // 2), (-(n + 5), -n)]
    _check_frames(perm, pkeys, vals, valid, frames, ["sum", "min", "last"], layout)
    gp, gk, gv, gok = perm.cuda(), pkeys.cuda(), vals.cuda(), valid.cuda()
    # nothing is ever in a frame that lies n rows back
    acc, cnt = dops.segmented_frame(gp, gk, (gv, gok), "sum", -(n + 5), -n)
    assert not bool(cnt.any()) and not bool(acc.any())
    # one past the reach: the op declines before anything is launched
    for lo, hi in [(-R - 1, 0), (0, R + 1), (-(R // 2) - 1, R - R // 2)]:
        with pytest.raises(NotImplementedError):
            dops.segmented_frame(gp, gk, (gv, gok), "sum", lo, hi)


def _fractional_case():
    n = 3 * T + 17
    perm, pkeys, _, valid, seg = _case("random", n, seed=17, nulls="random")
    rng = np.random.default_rng(18)
    vals = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    return perm, pkeys, torch.from_numpy(vals), valid, seg


def test_fractional_sum_equals_the_cpu_op_bit_for_bit():
    perm, pkeys, vals, valid, _ = _fractional_case()
    gp, gk, gv, gok = perm.cuda(), pkeys.cuda(), vals.cuda(), valid.cuda()
    for lo, hi in [(-6, 0), (-64, 64)]:
        exp_acc, exp_cnt = dops.segmented_frame(
            perm, pkeys, (vals, valid), "sum", lo, hi
        )
        acc, cnt = dops.segmented_frame(gp, gk, (gv, gok), "sum", lo, hi)
        assert torch.equal(cnt.cpu(), exp_cnt)
        # same order, adds only: the same bits
        assert torch.equal(acc.cpu().view(torch.int64), exp_acc.view(torch.int64))
        acc2, cnt2 = dops.segmented_frame(gp, gk, (gv, gok), "sum", lo, hi)
        assert torch.equal(acc.view(torch.int64), acc2.view(torch.int64))
        assert torch.equal(cnt, cnt2)


def test_frame_lands_in_original_row_order():
    n = T + WAVE + 1
    perm, pkeys, vals, valid, seg = _case("random", n, seed=5, nulls="random")
    acc, cnt = dops.segmented_frame(
        perm.cuda(), pkeys.cuda(), (vals.cuda(), valid.cuda()), "sum", -1, 0
    )
    # recompute from the sorted side and scatter by hand
    p = perm.numpy()
    sok = valid.numpy()[p]
    sv = np.where(sok, vals.numpy()[p], 0)
    same = seg[1:] == seg[:-1]
    s_acc = sv.copy()
    s_cnt = sok.astype(np.int64)
    s_acc[1:] += np.where(same, sv[:-1], 0)
    s_cnt[1:] += np.where(same, sok[:-1], False)
    exp_acc = np.zeros(n, dtype=np.int64)
    exp_cnt = np.zeros(n, dtype=np.int64)
    exp_acc[p] = s_acc
    exp_cnt[p] = s_cnt
    np.testing.assert_array_equal(cnt.cpu().numpy(), exp_cnt)
    np.testing.assert_array_equal(acc.cpu().numpy(), exp_acc)


def test_integer_sum_wraps_and_extremes_are_not_sentinels():
    big = np.iinfo(np.int64).max
    small = np.iinfo(np.int64).min
    v = [big, 1, small, small, big, big, small, 5, big, -5]
    ok = [True, True, True, False, True, True, False, True, False, True]
    k = [0] * 6 + [1] * 4
    n = len(v)
    perm = torch.arange(n, dtype=torch.int64)
    pk = torch.tensor(k, dtype=torch.int64)
    data = torch.tensor(v, dtype=torch.int64)
    valid = torch.tensor(ok)
    _check_frames(
        perm, pk, data, valid, [(-1, 0), (-1, 1), (0, 2), (-2, -1)], FUNCS, "ext"
    )
    acc, cnt = dops.segmented_frame(
        perm.cuda(), pk.cuda(), (data.cuda(), valid.cuda()), "sum", -1, 0
    )
    assert acc[1].item() == small and cnt[1].item() == 2  # MAX + 1 wraps
    acc, cnt = dops.segmented_frame(
        perm.cuda(), pk.cuda(), (data.cuda(), valid.cuda()), "max", 0, 0
    )
    assert (acc[2].item(), cnt[2].item()) == (small, 1)
    assert (acc[3].item(), cnt[3].item()) == (0, 0)


def test_empty_input_launches_nothing():
    z = torch.zeros(0, dtype=torch.int64, device="cuda")
    acc, cnt = dops.segmented_frame(z, z, (z, None), "sum", -2, 2)
    assert acc.numel() == 0 and cnt.numel() == 0
    acc, cnt = get_ext().seg_frame(z, z, z, None, 0, -2, 2)
    assert acc.numel() == 0 and cnt.numel() == 0


# ------------------------------------------------------------------ #
# end to end on the GPU engine                                         #
# ------------------------------------------------------------------ #
def test_sql_moving_average_sum_and_count():
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
        "SELECT k, o, v, "
        "AVG(v) OVER (PARTITION BY k ORDER BY o ROWS BETWEEN 6 PRECEDING AND CURRENT ROW) AS m, "
        "SUM(v) OVER (PARTITION BY k ORDER BY o ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING) AS s, "
        "COUNT(*) OVER (PARTITION BY k ORDER BY o ROWS BETWEEN 2 PRECEDING AND 2 FOLLOWING) AS c "
        "FROM df"
    )
    res = fugue_sql(sql, df=e.to_df(pdf), engine=e, as_fugue=True)
    assert isinstance(res, HipDataFrame)
    assert e.stats.get("window.device_frame") == 3
    assert e.stats.get("window.device") == 0
    assert e.stats.get("window.device_value") == 0
    assert e.stats.get("window.device_partition") == 0
    exp = fugue_sql(sql, df=pdf, engine=NativeExecutionEngine(), as_fugue=True)
    assert res.schema == exp.schema == "k:long,o:long,v:double,m:double,s:double,c:long"
    got = res.as_pandas()
    # integer-valued doubles: every sum is exact; row order is kept
    pd.testing.assert_frame_equal(got, exp.as_pandas(), check_dtype=False)
    srt = pdf.sort_values("o", kind="stable")
    g = srt.groupby("k", sort=False)["v"]
    roll = (
        g.rolling(7, min_periods=1).mean().reset_index(level=0, drop=True).sort_index()
    )
    pd.testing.assert_series_equal(got["m"], roll, check_names=False)
    # SQL null semantics, not pandas': a null row still sums its
    # neighbours (pandas' rolling sum over [prev, null, next] is null)
    prev, nxt = g.shift(1).sort_index(), g.shift(-1).sort_index()
    at = pdf["v"].isna() & prev.notna() & nxt.notna()
    assert at.any()
    np.testing.assert_array_equal(
        got["s"][at].to_numpy(), (prev[at] + nxt[at]).to_numpy()
    )
    alone = pdf["v"].isna() & prev.isna() & nxt.isna()
    assert got["s"][alone].isna().all()
    assert got["c"].between(1, 5).all()
