"""SQL ``ROWS`` window frames: the parser, the host executor against a
brute-force double loop, the torch-CPU ``segmented_frame`` of the ops layer
against the same loop, the ``frame_over`` lowering of HipExecutionEngine on
CPU tensors against the host executor, and a world-2 gloo run."""
import os
import pickle
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import pandas as pd
import pytest
import torch
import torch.multiprocessing as mp

from fugue_amd.execution.native_execution_engine import NativeExecutionEngine
from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine
from fugue_amd.hip.frame import HipDataFrame
from fugue_amd.sql.api import fugue_sql
from fugue_amd.sql.executor import WindowFunc, parse_select, run_sql_on_pandas

INT64_MAX = int(np.iinfo(np.int64).max)
INT64_MIN = int(np.iinfo(np.int64).min)

FRAMES: List[Tuple[Optional[int], Optional[int]]] = [
    (-2, 0), (-1, 1), (0, 3), (-3, -1), (1, 2), (7, 5),
    (None, 0), (0, None), (None, None), (None, 2), (-2, None), (None, -1),
]


def _bound(b: Optional[int], start: bool) -> str:
    if b is None:
        return "UNBOUNDED PRECEDING" if start else "UNBOUNDED FOLLOWING"
    if b == 0:
        return "CURRENT ROW"
    return f"{-b} PRECEDING" if b < 0 else f"{b} FOLLOWING"


def _frame_sql(lo: Optional[int], hi: Optional[int]) -> str:
    return f"ROWS BETWEEN {_bound(lo, True)} AND {_bound(hi, False)}"


def _wrap(v: int) -> int:
    return (v + 2**63) % 2**64 - 2**63


# ------------------------------------------------------------------ #
# parser                                                               #
# ------------------------------------------------------------------ #
def _window(over_tail: str, func: str = "SUM(v)") -> WindowFunc:
    stmt = parse_select(
        f"SELECT {func} OVER (PARTITION BY k ORDER BY t {over_tail}) AS r FROM df"
    )
    w = stmt.columns[0][0]
    assert isinstance(w, WindowFunc)
    return w


@pytest.mark.parametrize(
    "text,frame",
    [
        ("ROWS 3 PRECEDING", (-3, 0)),
        ("ROWS UNBOUNDED PRECEDING", (None, 0)),
        ("ROWS CURRENT ROW", (0, 0)),
        ("ROWS 0 PRECEDING", (0, 0)),
        ("rows between 6 preceding and current row", (-6, 0)),
        ("ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING", (-1, 1)),
        ("ROWS BETWEEN CURRENT ROW AND 3 FOLLOWING", (0, 3)),
        ("ROWS BETWEEN 3 PRECEDING AND 1 PRECEDING", (-3, -1)),
        ("ROWS BETWEEN 1 FOLLOWING AND 2 FOLLOWING", (1, 2)),
        ("ROWS BETWEEN 5 PRECEDING AND 7 PRECEDING", (-5, -7)),
        ("ROWS BETWEEN 7 FOLLOWING AND 5 FOLLOWING", (7, 5)),
        ("ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW", (None, 0)),
        ("ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING", (0, None)),
        ("ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING", (None, None)),
        ("ROWS BETWEEN UNBOUNDED PRECEDING AND 2 FOLLOWING", (None, 2)),
        ("ROWS BETWEEN 2 PRECEDING AND UNBOUNDED FOLLOWING", (-2, None)),
        ("ROWS BETWEEN UNBOUNDED PRECEDING AND 1 PRECEDING", (None, -1)),
        ("ROWS BETWEEN 0 FOLLOWING AND 0 FOLLOWING", (0, 0)),
    ],
)
def test_parser_accepts(text, frame):
    assert _window(text).frame == frame


def test_parser_frame_without_order_by_and_no_frame():
    stmt = parse_select(
        "SELECT SUM(v) OVER (PARTITION BY k ROWS 1 PRECEDING) AS a, "
        "SUM(v) OVER (PARTITION BY k ORDER BY t) AS b, "
        "LAG(v) OVER (PARTITION BY k) AS c FROM df"
    )
    assert stmt.columns[0][0].frame == (-1, 0)
    assert stmt.columns[0][0].order_by == []
    assert stmt.columns[1][0].frame is None
    assert stmt.columns[2][0].frame is None


@pytest.mark.parametrize(
    "text",
    [
        "ROWS UNBOUNDED FOLLOWING",
        "ROWS BETWEEN UNBOUNDED FOLLOWING AND UNBOUNDED FOLLOWING",
        "ROWS BETWEEN 1 PRECEDING AND UNBOUNDED PRECEDING",
        "ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED PRECEDING",
        "ROWS BETWEEN CURRENT ROW AND 1 PRECEDING",
        "ROWS BETWEEN 1 FOLLOWING AND 1 PRECEDING",
        "ROWS BETWEEN 1 FOLLOWING AND CURRENT ROW",
        "ROWS 2 FOLLOWING",
        "ROWS -1 PRECEDING",
        "ROWS 1.5 PRECEDING",
        "ROWS x PRECEDING",
        "ROWS BETWEEN 1 PRECEDING AND 'a' FOLLOWING",
        "ROWS 1",
        "ROWS BETWEEN 1 PRECEDING",
    ],
)
def test_parser_syntax_errors(text):
    with pytest.raises(SyntaxError):
        _window(text)


@pytest.mark.parametrize(
    "func", ["ROW_NUMBER()", "RANK()", "DENSE_RANK()", "LAG(v)", "LEAD(v, 2)"]
)
def test_parser_frame_on_function_without_one(func):
    with pytest.raises(SyntaxError):
        _window("ROWS 1 PRECEDING", func)


@pytest.mark.parametrize("kind", ["RANGE", "GROUPS"])
def test_parser_range_and_groups_stay_unsupported(kind):
    with pytest.raises(NotImplementedError):
        _window(f"{kind} BETWEEN 1 PRECEDING AND CURRENT ROW")


# ------------------------------------------------------------------ #
# brute force                                                          #
# ------------------------------------------------------------------ #
def _brute_sorted(
    keys: List[Any],
    vals: Optional[List[Any]],
    func: str,
    lo: Optional[int],
    hi: Optional[int],
    integer: bool,
) -> Tuple[List[Any], List[int]]:
    """(aggregate, count) of every position of a sequence whose equal
    keys are contiguous: a plain double loop over partitions and frames.
    ``vals`` holds None for a null (``None`` itself: COUNT(*)).  Integer
    sums are exact Python ints, wrapped to int64; a double sum starts
    from 0.0 and adds from left to right."""
    n = len(keys)
    res: List[Any] = [None] * n
    cnts = [0] * n
    s = 0
    while s < n:
        e = s
        while e < n and keys[e] == keys[s]:
            e += 1
        for i in range(s, e):
            a = s if lo is None else max(s, i + lo)
            b = e - 1 if hi is None else min(e - 1, i + hi)
            if vals is None:
                cnts[i] = max(0, b - a + 1)
                continue
            xs = [vals[j] for j in range(a, b + 1) if vals[j] is not None]
            cnts[i] = len(xs)
            if len(xs) == 0:
                continue
            if func == "sum":
                if integer:
                    res[i] = _wrap(sum(int(x) for x in xs))
                else:
                    acc = 0.0
                    for x in xs:
                        acc += float(x)
                    res[i] = acc
            elif func == "avg":
                acc = 0.0
                for x in xs:
                    acc += float(x)
                res[i] = acc / len(xs)
            elif func == "min":
                res[i] = min(xs)
            elif func == "max":
                res[i] = max(xs)
            elif func == "first":
                res[i] = xs[0]
            else:
                res[i] = xs[-1]
        s = e
    return res, cnts


def _nullable(series: pd.Series) -> List[Any]:
    return [None if pd.isna(v) else v for v in series.tolist()]


def _holds_row(lo: Optional[int], hi: Optional[int]) -> bool:
    return (lo is None or lo <= 0) and (hi is None or hi >= 0)


def _base_frame(seed: int = 3, n: int = 500) -> pd.DataFrame:
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 9, n)
    k[rng.choice(n, 5, replace=False)] = np.arange(100, 105)  # single rows
    pdf = pd.DataFrame(
        dict(
            k=k,
            a=rng.integers(0, 6, n),  # many duplicates: ties by row order
            i8=rng.integers(-100, 100, n).astype(np.int8),
            i16=rng.integers(-3000, 3000, n).astype(np.int16),
            i32=rng.integers(-(2**30), 2**30, n).astype(np.int32),
            i64=rng.integers(-(2**40), 2**40, n),
            f=rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n)),
            g=rng.integers(-40, 40, n).astype(np.float64),  # exact sums
            w=(rng.standard_normal(n) * 3).astype(np.float32),
        )
    )
    for c in ("f", "g"):
        pdf[c] = pdf[c].mask(rng.random(n) < 0.25)
        pdf.loc[pdf["k"] == 3, c] = np.nan  # an all-null partition
    pdf.loc[rng.choice(n, 20, replace=False), "f"] = None
    pdf["w"] = pdf["w"].mask(rng.random(n) < 0.2)
    assert pdf["w"].dtype == np.float32
    return pdf


_ORDERS = {"asc": "ORDER BY a", "desc": "ORDER BY a DESC", "none": ""}


def _sorted_frame(pdf: pd.DataFrame, order: str) -> pd.DataFrame:
    if order == "none":
        return pdf.sort_values(["k"], kind="stable")
    return pdf.sort_values(
        ["k", "a"], ascending=[True, order == "asc"], kind="stable"
    )


def _expected(
    pdf: pd.DataFrame, order: str, col: Optional[str], func: str,
    lo: Optional[int], hi: Optional[int],
) -> pd.Series:
    """The column the statement must yield, in original row order, typed
    by the table of the issue."""
    s = _sorted_frame(pdf, order)
    integer = col is not None and pdf[col].dtype.kind == "i"
    vals = None if col is None else _nullable(s[col])
    res, cnts = _brute_sorted(
        s["k"].tolist(), vals, "sum" if func == "count" else func, lo, hi,
        integer,
    )
    if func == "count":
        out = pd.Series(cnts, index=s.index, dtype="int64")
    elif integer and func != "avg" and _holds_row(lo, hi):
        assert all(r is not None for r in res)
        out = pd.Series(res, index=s.index, dtype="int64")
    else:
        out = pd.Series(
            [np.nan if r is None else float(r) for r in res],
            index=s.index, dtype="float64",
        )
    return out.sort_index()


def _bits(s: pd.Series) -> List[Any]:
    if s.dtype.kind != "f":
        return s.tolist()
    a = s.to_numpy(dtype="float64")
    # every null is one value; everything else compares by its bits
    return [None if x != x else int(np.float64(x).view(np.int64)) for x in a]


_SQL_FUNCS = {
    "sum": "SUM", "min": "MIN", "max": "MAX", "count": "COUNT", "avg": "AVG",
    "first": "FIRST_VALUE", "last": "LAST_VALUE",
}


# ------------------------------------------------------------------ #
# host executor vs brute force                                         #
# ------------------------------------------------------------------ #
@pytest.mark.parametrize("order", list(_ORDERS))
@pytest.mark.parametrize("frame", FRAMES, ids=str)
def test_host_executor_matches_brute_force(frame, order):
    lo, hi = frame
    pdf = _base_frame()
    bounded = lo is not None and hi is not None
    # bounded frames are compared bit for bit on fractional doubles;
    # half-unbounded ones leave the order open: exactly summable values
    dcol = "f" if bounded else "g"
    cases = [(f, dcol) for f in _SQL_FUNCS] + [
        ("sum", "i64"), ("min", "i32"), ("max", "i16"), ("first", "i8"),
        ("last", "i64"), ("avg", "i32"), ("count", "i8"), ("count", None),
    ]
    if bounded:
        cases += [("sum", "w"), ("avg", "w"), ("min", "w")]
    items = ", ".join(
        f"{_SQL_FUNCS[f]}({c or '*'}) OVER (PARTITION BY k {_ORDERS[order]} "
        f"{_frame_sql(lo, hi)}) AS r{j}"
        for j, (f, c) in enumerate(cases)
    )
    res, _ = run_sql_on_pandas(f"SELECT {items} FROM df", {"df": pdf})
    for j, (f, c) in enumerate(cases):
        exp = _expected(pdf, order, c, f, lo, hi)
        got = res[f"r{j}"]
        assert got.dtype == exp.dtype, (f, c, got.dtype, exp.dtype)
        assert _bits(got) == _bits(exp), (f, c)


@pytest.mark.parametrize(
    "col,long_type",
    [("i8", True), ("i16", True), ("i32", True), ("i64", True),
     ("f", False), ("w", False)],
)
def test_host_executor_result_types(col, long_type):
    pdf = _base_frame()
    over = "PARTITION BY k ORDER BY a"
    sql = (
        f"SELECT SUM({col}) OVER ({over} ROWS 2 PRECEDING) AS s_in, "
        f"MIN({col}) OVER ({over} ROWS BETWEEN UNBOUNDED PRECEDING AND 1 FOLLOWING) AS m_in, "
        f"LAST_VALUE({col}) OVER ({over} ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING) AS l_in, "
        f"SUM({col}) OVER ({over} ROWS BETWEEN 3 PRECEDING AND 1 PRECEDING) AS s_out, "
        f"MAX({col}) OVER ({over} ROWS BETWEEN 1 FOLLOWING AND UNBOUNDED FOLLOWING) AS m_out, "
        f"FIRST_VALUE({col}) OVER ({over} ROWS BETWEEN 7 FOLLOWING AND 5 FOLLOWING) AS f_out, "
        f"AVG({col}) OVER ({over} ROWS 2 PRECEDING) AS a, "
        f"COUNT({col}) OVER ({over} ROWS BETWEEN 3 PRECEDING AND 1 PRECEDING) AS c, "
        f"COUNT(*) OVER ({over} ROWS BETWEEN 7 FOLLOWING AND 5 FOLLOWING) AS n FROM df"
    )
    res, _ = run_sql_on_pandas(sql, {"df": pdf})
    inside = "int64" if long_type else "float64"
    for name in ("s_in", "m_in", "l_in"):
        assert res[name].dtype == inside, name
    for name in ("s_out", "m_out", "f_out", "a"):
        assert res[name].dtype == "float64", name
    for name in ("c", "n"):
        assert res[name].dtype == "int64", name
    assert res["f_out"].isna().all() and (res["n"] == 0).all()


def test_host_executor_nullable_integer_series_is_double():
    pdf = _base_frame()
    pdf["q"] = pdf["i32"].astype("Int64").mask(pdf.index % 5 == 0)
    sql = (
        "SELECT SUM(q) OVER (PARTITION BY k ORDER BY a ROWS 2 PRECEDING) AS s, "
        "COUNT(q) OVER (PARTITION BY k ORDER BY a ROWS 2 PRECEDING) AS c FROM df"
    )
    res, _ = run_sql_on_pandas(sql, {"df": pdf})
    assert res["s"].dtype == "float64" and res["c"].dtype == "int64"
    s = _sorted_frame(pdf, "asc")
    exp, cnts = _brute_sorted(
        s["k"].tolist(), _nullable(s["q"]), "sum", -2, 0, True
    )
    exp_s = pd.Series(
        [np.nan if r is None else float(r) for r in exp], index=s.index
    ).sort_index()
    assert _bits(res["s"]) == _bits(exp_s)
    assert res["c"].tolist() == pd.Series(cnts, index=s.index).sort_index().tolist()


def test_unframed_windows_keep_their_pandas_semantics():
    # the legacy running path copies pandas cumsum (a null row is null);
    # the framed form of the same window skips nulls instead
    pdf = pd.DataFrame(dict(k=[1, 1, 1], a=[1, 2, 3], v=[1.0, np.nan, 2.0]))
    res, _ = run_sql_on_pandas(
        "SELECT SUM(v) OVER (PARTITION BY k ORDER BY a) AS legacy, "
        "SUM(v) OVER (PARTITION BY k ORDER BY a ROWS UNBOUNDED PRECEDING) AS framed "
        "FROM df",
        {"df": pdf},
    )
    assert _bits(res["legacy"]) == _bits(pd.Series([1.0, np.nan, 3.0]))
    assert _bits(res["framed"]) == _bits(pd.Series([1.0, 1.0, 3.0]))


# ------------------------------------------------------------------ #
# ops layer (torch CPU) vs brute force                                 #
# ------------------------------------------------------------------ #
def _ops_case(pdf: pd.DataFrame, col: str, asc: bool):
    hdf = HipDataFrame(pdf, device="cpu")
    pk, _ = dops.pack_keys([hdf.col("k")])
    pk = pk.contiguous()
    perm = dops.sort_indices_exact(hdf, ["a"], [asc], "last", key_tensor=pk)
    s = pdf.iloc[perm.numpy()]
    return hdf, pk, perm, s


def _check_ops(pdf: pd.DataFrame, col: str, asc: bool, frames) -> None:
    hdf, pk, perm, s = _ops_case(pdf, col, asc)
    integer = pdf[col].dtype.kind == "i"
    keys = pk.index_select(0, perm).tolist()
    vals = _nullable(s[col])
    for lo, hi in frames:
        for func in ("sum", "min", "max", "first", "last"):
            acc, cnt = dops.segmented_frame(perm, pk, hdf.col(col), func, lo, hi)
            assert cnt.dtype == torch.int64
            assert acc.dtype == (torch.int64 if integer else torch.float64)
            exp, cnts = _brute_sorted(keys, vals, func, lo, hi, integer)
            got_acc = acc.index_select(0, perm)
            assert cnt.index_select(0, perm).tolist() == cnts, (func, lo, hi)
            want = [0 if r is None else r for r in exp]
            if integer:
                assert got_acc.tolist() == want, (func, lo, hi)
            else:
                w = torch.tensor(want, dtype=torch.float64)
                assert torch.equal(
                    got_acc.view(torch.int64), w.view(torch.int64)
                ), (func, lo, hi)


_BOUNDED = [(lo, hi) for lo, hi in FRAMES if lo is not None and hi is not None]


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("col", ["i64", "i16", "f", "w"])
def test_ops_frame_matches_brute_force(col, asc):
    pdf = _base_frame()
    if col == "w":
        # the brute force adds the widened values
        pdf["w"] = pdf["w"].astype(np.float64)
    _check_ops(pdf, col, asc, _BOUNDED + [(0, 0), (-6, 0), (-20, 20)])


def test_ops_int64_extremes_wrap_and_are_not_sentinels():
    k = [0] * 6 + [1] * 4 + [2] * 3
    v = [INT64_MAX, 1, INT64_MIN, INT64_MIN, INT64_MAX, INT64_MAX,
         INT64_MIN, 5, INT64_MAX, -5,
         7, INT64_MIN, INT64_MAX]
    ok = [True, True, True, False, True, True,
          False, True, False, True,
          False, True, True]
    n = len(k)
    pk = torch.tensor(k, dtype=torch.int64)
    perm = torch.arange(n, dtype=torch.int64)
    data = torch.tensor(v, dtype=torch.int64)
    valid = torch.tensor(ok)
    vals = [x if o else None for x, o in zip(v, ok)]
    for lo, hi in [(-1, 0), (-1, 1), (0, 2), (-2, -1), (-5, 5)]:
        for func in ("sum", "min", "max", "first", "last"):
            acc, cnt = dops.segmented_frame(perm, pk, (data, valid), func, lo, hi)
            exp, cnts = _brute_sorted(k, vals, func, lo, hi, True)
            assert cnt.tolist() == cnts
            assert acc.tolist() == [0 if r is None else r for r in exp], (func, lo, hi)
    # the wrap itself: MAX + 1 over the first two rows
    acc, cnt = dops.segmented_frame(perm, pk, (data, valid), "sum", -1, 0)
    assert acc[1].item() == INT64_MIN and cnt[1].item() == 2
    # a lone extreme is a value, and a null next to it leaves it alone
    acc, cnt = dops.segmented_frame(perm, pk, (data, valid), "min", 0, 1)
    assert (acc[2].item(), cnt[2].item()) == (INT64_MIN, 1)
    acc, cnt = dops.segmented_frame(perm, pk, (data, valid), "max", 0, 0)
    assert (acc[3].item(), cnt[3].item()) == (0, 0)
    assert (acc[4].item(), cnt[4].item()) == (INT64_MAX, 1)


def test_ops_offsets_beyond_n_empty_input_and_bad_arguments():
    pdf = _base_frame(n=40)
    hdf, pk, perm, s = _ops_case(pdf, "g", True)
    n = len(pdf)
    keys = pk.index_select(0, perm).tolist()
    vals = _nullable(s["g"])
    for lo, hi in [(-n, 0), (0, n), (-(10**15), 10**15), (-n - 3, n + 3),
                   (n, n + 5), (-n - 5, -n), (10**15, 2 * 10**15),
                   (-(10**15), -(10**15) + 2), (3, -10**15)]:
        acc, cnt = dops.segmented_frame(perm, pk, hdf.col("g"), "sum", lo, hi)
        exp, cnts = _brute_sorted(keys, vals, "sum", lo, hi, False)
        assert cnt.index_select(0, perm).tolist() == cnts, (lo, hi)
        assert acc.index_select(0, perm).tolist() == [
            0.0 if r is None else r for r in exp
        ], (lo, hi)
    empty = torch.empty(0, dtype=torch.int64)
    for data in (empty, torch.empty(0, dtype=torch.float64)):
        acc, cnt = dops.segmented_frame(empty, empty, (data, None), "max", -2, 2)
        assert acc.numel() == 0 and cnt.numel() == 0
        assert acc.dtype == data.dtype and cnt.dtype == torch.int64
    with pytest.raises(ValueError):
        dops.segmented_frame(perm, pk, hdf.col("g"), "avg", -1, 0)


def test_ops_reach_beyond_the_limit():
    R = dops.SEG_FRAME_MAX_REACH
    assert R >= 255
    n = R + 50
    pk = torch.zeros(n, dtype=torch.int64)
    perm = torch.arange(n, dtype=torch.int64)
    data = torch.ones(n, dtype=torch.int64)
    acc, cnt = dops.segmented_frame(perm, pk, (data, None), "sum", -R, 0)
    assert cnt.tolist() == [min(i, R) + 1 for i in range(n)]
    assert torch.equal(acc, cnt)
    for lo, hi in [(-R - 1, 0), (0, R + 1), (-R // 2 - 1, R - R // 2)]:
        with pytest.raises(NotImplementedError):
            dops.segmented_frame(perm, pk, (data, None), "sum", lo, hi)
    # empty for every row whatever the distance: nothing to reach
    acc, cnt = dops.segmented_frame(perm, pk, (data, None), "sum", -n - 5, -n)
    assert not cnt.any() and not acc.any()


# ------------------------------------------------------------------ #
# FugueSQL lowering on HipExecutionEngine (CPU tensors)                #
# ------------------------------------------------------------------ #
def _rows(pdf: pd.DataFrame) -> List[Tuple]:
    def _norm(v: Any) -> Any:
        if pd.isna(v):
            return None
        if isinstance(v, (int, float, np.integer, np.floating)):
            return float(v)
        return v

    return sorted(
        (tuple(_norm(v) for v in r) for r in pdf.itertuples(index=False)),
        key=repr,
    )


def _sql_frame() -> pd.DataFrame:
    rng = np.random.default_rng(11)
    n = 300
    pdf = pd.DataFrame(
        dict(
            k=rng.integers(0, 7, n),
            s=rng.choice(["p", "q", "r"], n),
            a=rng.integers(0, 5, n),
            i=rng.integers(-20, 20, n),
            j=rng.integers(-20, 20, n).astype(np.int32),
            v=rng.standard_normal(n) * np.exp(rng.uniform(-4, 4, n)),
            g=rng.integers(0, 12, n).astype(np.float64) / 2,  # exact sums
            w=(rng.integers(0, 12, n) / 4).astype(np.float32),
        )
    )
    for c in ("v", "g"):
        pdf[c] = pdf[c].mask(pdf.index % 8 == 0)
        pdf.loc[pdf["k"] == 2, c] = np.nan
    return pdf


def _both(sql: str, pdf: pd.DataFrame, e: HipExecutionEngine):
    got = fugue_sql(sql, df=pdf, engine=e, as_fugue=True)
    exp = fugue_sql(sql, df=pdf, engine=NativeExecutionEngine(), as_fugue=True)
    return got, exp


def _assert_same(got, exp) -> None:
    assert got.schema == exp.schema
    gp, ep = got.as_pandas(), exp.as_pandas()
    # ties follow original row order on both paths and the lowered frame
    # keeps the input row order
    pd.testing.assert_frame_equal(gp, ep, check_dtype=False)
    assert _rows(gp) == _rows(ep)


def _other_window_counters(e: HipExecutionEngine) -> int:
    return (
        e.stats.get("window.device")
        + e.stats.get("window.device_value")
        + e.stats.get("window.device_partition")
    )


# bounded frames on fractional doubles (bit for bit through both paths);
# frames that go through the scan / total kernels on exact values
_LOWERED_ITEMS = [
    ("SUM(v)", (-2, 0)), ("SUM(v)", (-1, 1)), ("AVG(v)", (-6, 0)),
    ("MIN(v)", (0, 3)), ("MAX(v)", (-3, -1)), ("FIRST_VALUE(v)", (1, 2)),
    ("LAST_VALUE(v)", (-2, 0)), ("COUNT(v)", (-1, 1)), ("COUNT(*)", (-1, 1)),
    ("SUM(v)", (7, 5)), ("COUNT(*)", (7, 5)), ("COUNT(*)", (-3, -1)),
    ("SUM(i)", (-2, 0)), ("SUM(i)", (-3, -1)), ("MIN(j)", (-1, 1)),
    ("MAX(j)", (1, 2)), ("FIRST(i)", (0, 3)), ("LAST(j)", (-3, -1)),
    ("AVG(i)", (-2, 0)), ("MEAN(j)", (1, 2)), ("COUNT(i)", (-3, -1)),
    ("SUM(w)", (-2, 0)), ("AVG(w)", (-1, 1)), ("MIN(w)", (-3, -1)),
    ("SUM(g)", (None, 0)), ("MIN(g)", (None, 0)), ("MAX(i)", (None, 0)),
    ("COUNT(g)", (None, 0)), ("COUNT(*)", (None, 0)), ("AVG(g)", (None, 0)),
    ("SUM(i)", (None, 0)), ("AVG(j)", (None, 0)),
    ("SUM(g)", (None, None)), ("MIN(i)", (None, None)),
    ("FIRST_VALUE(g)", (None, None)), ("LAST_VALUE(j)", (None, None)),
    ("COUNT(*)", (None, None)), ("COUNT(g)", (None, None)),
    ("AVG(g)", (None, None)), ("SUM(w)", (None, None)),
]


@pytest.mark.parametrize(
    "over",
    ["PARTITION BY k ORDER BY a", "PARTITION BY s, k ORDER BY a DESC, i",
     "PARTITION BY k"],
)
@pytest.mark.parametrize(
    "item,frame", _LOWERED_ITEMS, ids=[f"{i}{f}" for i, f in _LOWERED_ITEMS]
)
def test_sql_frame_lowered(item, frame, over):
    pdf = _sql_frame()
    e = HipExecutionEngine()
    sql = f"SELECT *, {item} OVER ({over} {_frame_sql(*frame)}) AS r FROM df"
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device_frame") == 1
    assert _other_window_counters(e) == 0
    _assert_same(got, exp)
    if frame[0] is not None and frame[1] is not None:
        assert _bits(got.as_pandas()["r"]) == _bits(exp.as_pandas()["r"])


def test_sql_two_frames_share_one_over():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    over = "PARTITION BY k ORDER BY a"
    sql = (
        f"SELECT k, a, AVG(v) OVER ({over} ROWS BETWEEN 6 PRECEDING AND CURRENT ROW) AS m, "
        f"v, SUM(i) OVER ({over} ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING) AS t, "
        f"COUNT(*) OVER ({over} ROWS BETWEEN 2 PRECEDING AND 2 FOLLOWING) AS c, "
        f"MAX(i) OVER ({over} ROWS BETWEEN 2 PRECEDING AND 1 PRECEDING) AS x FROM df"
    )
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device_frame") == 4
    assert _other_window_counters(e) == 0
    assert got.schema == "k:long,a:long,m:double,v:double,t:long,c:long,x:double"
    _assert_same(got, exp)


def test_sql_frame_after_where():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    sql = (
        "SELECT k, a, i, SUM(i) OVER (PARTITION BY k ORDER BY a ROWS 2 PRECEDING) AS r, "
        "COUNT(*) OVER (PARTITION BY k ORDER BY a ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING) AS c "
        "FROM df WHERE a > 1"
    )
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device_frame") == 2
    assert got.schema == exp.schema
    assert _rows(got.as_pandas()) == _rows(exp.as_pandas())
    # a frame never counts a row the WHERE removed
    assert got.as_pandas()["c"].max() == 3


_FAR = dops.SEG_FRAME_MAX_REACH + 1
_DECLINED = {
    "framed-and-unframed": (
        "SELECT k, a, SUM(g) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS r, "
        "SUM(g) OVER (PARTITION BY k ORDER BY a) AS q FROM df"
    ),
    "framed-and-ranking": (
        "SELECT k, a, SUM(g) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS r, "
        "ROW_NUMBER() OVER (PARTITION BY k ORDER BY a) AS q FROM df"
    ),
    "two-overs": (
        "SELECT k, a, SUM(g) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS r, "
        "SUM(g) OVER (PARTITION BY k ORDER BY a DESC ROWS 1 PRECEDING) AS q FROM df"
    ),
    "expr-arg": (
        "SELECT k, a, SUM(g + 1) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS r FROM df"
    ),
    "expr-key": (
        "SELECT k, a, SUM(g) OVER (PARTITION BY k + 1 ORDER BY a ROWS 1 PRECEDING) AS r FROM df"
    ),
    "nullable-int": (
        "SELECT k, a, SUM(n) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS r FROM df"
    ),
    "string": (
        "SELECT k, a, COUNT(s) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS r, "
        "LAST_VALUE(s) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS q FROM df"
    ),
    "bool": (
        "SELECT k, a, COUNT(b) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS r FROM df"
    ),
    "current-to-end": (
        "SELECT k, a, SUM(g) OVER (PARTITION BY k ORDER BY a "
        "ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING) AS r FROM df"
    ),
    "start-to-following": (
        "SELECT k, a, MAX(i) OVER (PARTITION BY k ORDER BY a "
        "ROWS BETWEEN UNBOUNDED PRECEDING AND 2 FOLLOWING) AS r FROM df"
    ),
    "start-to-preceding": (
        "SELECT k, a, COUNT(*) OVER (PARTITION BY k ORDER BY a "
        "ROWS BETWEEN UNBOUNDED PRECEDING AND 1 PRECEDING) AS r FROM df"
    ),
    "preceding-to-end": (
        "SELECT k, a, MIN(g) OVER (PARTITION BY k ORDER BY a "
        "ROWS BETWEEN 2 PRECEDING AND UNBOUNDED FOLLOWING) AS r FROM df"
    ),
    "running-first": (
        "SELECT k, a, FIRST_VALUE(g) OVER (PARTITION BY k ORDER BY a "
        "ROWS UNBOUNDED PRECEDING) AS r FROM df"
    ),
    "reach": (
        f"SELECT k, a, SUM(g) OVER (PARTITION BY k ORDER BY a ROWS {_FAR} PRECEDING) AS r, "
        f"COUNT(*) OVER (PARTITION BY k ORDER BY a ROWS BETWEEN 1 PRECEDING AND {_FAR - 1} FOLLOWING) AS q "
        "FROM df"
    ),
    "group-by": (
        "SELECT k, SUM(MAX(i)) OVER (PARTITION BY k ROWS 1 PRECEDING) AS r FROM df GROUP BY k"
    ),
    "distinct": (
        "SELECT DISTINCT k, SUM(i) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS r FROM df"
    ),
}


@pytest.mark.parametrize("shape", list(_DECLINED))
def test_sql_frame_declined_shapes(shape):
    sql = _DECLINED[shape]
    pdf = _sql_frame()
    pdf["b"] = pdf["a"] % 2 == 0
    pdf["n"] = pdf["i"].astype("Int64").mask(pdf.index % 5 == 0)
    e = HipExecutionEngine()
    try:
        exp = fugue_sql(sql, df=pdf, engine=NativeExecutionEngine(), as_fugue=True)
    except Exception as ex:  # the host rejects the statement: so must we
        with pytest.raises(type(ex)):
            fugue_sql(sql, df=pdf, engine=e, as_fugue=True)
        assert e.stats.get("window.device_frame") == 0
        return
    got = fugue_sql(sql, df=pdf, engine=e, as_fugue=True)
    assert e.stats.get("window.device_frame") == 0
    assert _other_window_counters(e) == 0
    assert got.schema == exp.schema
    assert _rows(got.as_pandas()) == _rows(exp.as_pandas())


def test_frame_over_declines_directly():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    hdf = e.to_df(pdf)
    ok = ("r", "sum", "g", -1, 0)
    R = dops.SEG_FRAME_MAX_REACH
    for args in (
        (hdf, [], [("a", True)], [ok]),
        (hdf, ["k"], [("a", True)], []),
        (hdf, ["k"], [("a", True)], [("g", "sum", "g", -1, 0)]),
        (hdf, ["k"], [("a", True)], [ok, ok]),
        (hdf, ["k"], [("a", True)], [("r", "lag", "g", -1, 0)]),
        (hdf, ["k"], [("a", True)], [("r", "sum", None, -1, 0)]),
        (hdf, ["k"], [("a", True)], [("r", "sum", "zz", -1, 0)]),
        (hdf, ["k"], [("a", True)], [("r", "sum", "s", -1, 0)]),
        (hdf, ["k"], [("a", True)], [("r", "sum", "g", -1.5, 0)]),
        (hdf, ["k"], [("a", True)], [("r", "sum", "g", 0, None)]),
        (hdf, ["k"], [("a", True)], [("r", "sum", "g", None, 1)]),
        (hdf, ["k"], [("a", True)], [("r", "first_value", "g", None, 0)]),
        (hdf, ["k"], [("a", True)], [("r", "sum", "g", -R - 1, 0)]),
        (hdf, ["k"], [("a", True)], [("r", "sum", "g", -1, R)]),
        (hdf, ["k"], [("s", True)], [ok]),
        (hdf, ["g"], [("a", True)], [ok]),
    ):
        with pytest.raises(NotImplementedError):
            e.frame_over(*args)
    empty = e.to_df(pdf.iloc[:0])
    with pytest.raises(NotImplementedError):
        e.frame_over(empty, ["k"], [("a", True)], [ok])
    os.environ["FUGUE_HIP_FORCE_HOST_WINDOW"] = "1"
    try:
        with pytest.raises(NotImplementedError):
            e.frame_over(hdf, ["k"], [("a", True)], [ok])
    finally:
        del os.environ["FUGUE_HIP_FORCE_HOST_WINDOW"]
    assert e.stats.get("window.device_frame") == 0
    res = e.frame_over(
        hdf, ["k"], [("a", True)],
        [ok, ("c", "count", None, -2, 2), ("x", "max", "i", -R, 0),
         ("y", "min", "j", -3, -1), ("z", "sum", "g", 9, 3)],
    )
    assert e.stats.get("window.device_frame") == 5
    assert res.schema == hdf.schema + "r:double,c:long,x:long,y:double,z:double"
    assert res.as_pandas()["z"].isna().all()


def test_reserved_temporary_name_in_input():
    pdf = _sql_frame()[["k", "a", "g"]]
    pdf["_fugue_window_value_2"] = 1
    e = HipExecutionEngine()
    sql = "SELECT k, a, SUM(g) OVER (PARTITION BY k ORDER BY a ROWS 1 PRECEDING) AS r FROM df"
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device_frame") == 0
    assert got.schema == exp.schema
    assert _rows(got.as_pandas()) == _rows(exp.as_pandas())


# ------------------------------------------------------------------ #
# distributed (gloo, world 2)                                          #
# ------------------------------------------------------------------ #
WORLD = 2
_NO_GPU_ENV = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}


def _run_worker(rank: int, world: int, port: int, fn_bytes: bytes, out_q) -> None:
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["WORLD_SIZE"] = str(world)
    os.environ["RANK"] = str(rank)
    os.environ["LOCAL_RANK"] = str(rank)
    try:
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        from fugue_amd.parallel.comm import reset_communicator

        reset_communicator()
        fn = pickle.loads(fn_bytes)
        out_q.put((rank, "ok", fn(rank)))
    except Exception:  # pragma: no cover
        import traceback

        out_q.put((rank, "error", traceback.format_exc()))
    finally:
        try:
            import torch.distributed as dist

            if dist.is_initialized():
                dist.destroy_process_group()
        except Exception:
            pass


def run_distributed(fn: Callable[[int], Any], port: int) -> Dict[int, Any]:
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [
        ctx.Process(target=_run_worker, args=(r, WORLD, port, pickle.dumps(fn), q))
        for r in range(WORLD)
    ]
    # gloo/CPU ranks must not see a GPU the host may have
    saved = {k: os.environ.get(k) for k in _NO_GPU_ENV}
    os.environ.update(_NO_GPU_ENV)
    try:
        for p in procs:
            p.start()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    results: Dict[int, Any] = {}
    try:
        for _ in range(WORLD):
            rank, status, res = q.get(timeout=180)
            if status == "error":
                raise RuntimeError(f"rank {rank} failed:\n{res}")
            results[rank] = res
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    return results


def _dist_frame() -> pd.DataFrame:
    rng = np.random.default_rng(23)
    n = 1000
    pdf = pd.DataFrame(
        dict(
            k=rng.integers(0, 37, n),
            o=rng.permutation(n),  # unique: no ties across the shuffle
            v=rng.integers(-30, 30, n).astype(np.float64),
            i=rng.integers(-30, 30, n),
        )
    )
    pdf["v"] = pdf["v"].mask(pdf.index % 7 == 0)
    return pdf


_SPLITS = {"uneven": 700, "one-empty": 1000}
_DIST_ITEMS = [
    ("m", "avg", "v", -6, 0),
    ("t", "sum", "v", -1, 1),
    ("c", "count", None, -2, 2),
    ("x", "max", "i", -3, -1),
    ("u", "sum", "i", None, 0),
    ("l", "last_value", "v", None, None),
]


def _dist_job(rank: int):
    from fugue_amd.hip.execution_engine import HipExecutionEngine as Eng
    from fugue_amd.hip.frame import HipDataFrame as Hdf

    e = Eng()
    assert e.is_distributed and e.world_size == 2
    pdf = _dist_frame()
    out: Dict[str, Any] = {}
    for name, cut in _SPLITS.items():
        part = pdf.iloc[:cut] if rank == 0 else pdf.iloc[cut:]
        shard = Hdf(
            part.reset_index(drop=True), "k:long,o:long,v:double,i:long",
            device="cpu",
        )
        before = e.stats.get("window.device_frame")
        res = e.frame_over(shard, ["k"], [("o", False)], _DIST_ITEMS)
        assert e.stats.get("window.device_frame") == before + len(_DIST_ITEMS)
        out[name] = res.as_pandas().to_dict("list")
    return out


def test_distributed_frame_over():
    results = run_distributed(_dist_job, 29573)
    pdf = _dist_frame()
    single = HipExecutionEngine()
    exp = single.frame_over(
        HipDataFrame(pdf, "k:long,o:long,v:double,i:long", device="cpu"),
        ["k"], [("o", False)], _DIST_ITEMS,
    ).as_pandas()
    # the single-process result itself is the brute force's
    s = pdf.sort_values(["k", "o"], ascending=[True, False], kind="stable")
    brute, _ = _brute_sorted(s["k"].tolist(), _nullable(s["v"]), "avg", -6, 0, False)
    want = pd.Series(
        [np.nan if r is None else r for r in brute], index=s.index
    ).sort_index()
    assert _bits(exp["m"]) == _bits(want)
    for name in _SPLITS:
        shards = [pd.DataFrame(results[r][name]) for r in range(2)]
        allr = pd.concat(shards)
        assert len(allr) == len(pdf)
        assert list(allr.columns) == list(exp.columns)
        assert _rows(allr) == _rows(exp)
        # every partition lives on one rank
        assert set(shards[0]["k"]).isdisjoint(set(shards[1]["k"]))
