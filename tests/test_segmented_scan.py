"""Value windows (LAG/LEAD, running SUM/MIN/MAX/COUNT/AVG): the torch-CPU
implementations of the ops layer against pandas, the HipExecutionEngine
``window_over`` path and its FugueSQL lowering on CPU tensors against the
host executor, and a world-2 gloo run."""
import os
import pickle
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch
import torch.multiprocessing as mp

from fugue_amd.execution.native_execution_engine import NativeExecutionEngine
from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
from fugue_amd.schema import Schema
from fugue_amd.sql.api import fugue_sql

INT64_MAX = np.iinfo(np.int64).max


# ------------------------------------------------------------------ #
# ops layer vs pandas                                                  #
# ------------------------------------------------------------------ #
def _base_frame(seed: int = 0, n: int = 500) -> pd.DataFrame:
    rng = np.random.default_rng(seed)
    pdf = pd.DataFrame(
        dict(
            k=rng.integers(0, 9, n),
            a=rng.integers(0, 6, n),  # many duplicates: ties by row order
            i=rng.integers(-50, 50, n),
            f=rng.integers(-40, 40, n).astype(np.float64) / 4,  # exact sums
        )
    )
    pdf["f"] = pdf["f"].mask(rng.random(n) < 0.25)
    pdf.loc[pdf["k"] == 3, "f"] = np.nan  # an all-null partition
    return pdf


def _sorted_perm(
    pdf: pd.DataFrame, asc: bool, hdf: Optional[HipDataFrame] = None
) -> Tuple[HipDataFrame, torch.Tensor, torch.Tensor, Any]:
    hdf = hdf if hdf is not None else HipDataFrame(pdf, device="cpu")
    pk, _ = dops.pack_keys([hdf.col("k")])
    pk = pk.contiguous()
    perm = dops.sort_indices_exact(hdf, ["a"], [asc], "last", key_tensor=pk)
    s = pdf.sort_values("a", ascending=asc, kind="stable")
    return hdf, pk, perm, s.groupby("k", sort=False, dropna=False)


def _expanding(gv: Any, how: str) -> pd.Series:
    return getattr(gv.expanding(), how)().reset_index(level=0, drop=True)


def _check_scan(pdf: pd.DataFrame, col: str, asc: bool,
                hdf: Optional[HipDataFrame] = None) -> None:
    pdf = pdf.reset_index(drop=True)
    hdf, pk, perm, g = _sorted_perm(pdf, asc, hdf)
    gv = g[col]
    isnull = pdf[col].isna().to_numpy()
    want = dict(sum=gv.cumsum(), min=gv.cummin(), max=gv.cummax())
    for func, exp in want.items():
        acc, cnt = dops.segmented_scan(perm, pk, hdf.col(col), func)
        exp = exp.sort_index()
        assert acc.dtype in (torch.int64, torch.float64)
        got = acc.numpy()
        # the aggregate is null at a null row; elsewhere it is exact
        np.testing.assert_array_equal(exp.isna().to_numpy(), isnull)
        np.testing.assert_array_equal(
            got[~isnull], exp.to_numpy()[~isnull].astype(got.dtype), err_msg=func
        )
        exp_cnt = _expanding(gv, "count").sort_index().to_numpy()
        np.testing.assert_array_equal(cnt.numpy(), exp_cnt.astype(np.int64))
        assert bool((acc[cnt == 0] == 0).all())
    # AVG as the engine forms it: float64 running sum / count
    acc, cnt = dops.segmented_scan(
        perm, pk, (hdf.col(col).data.to(torch.float64), hdf.col(col).valid), "sum"
    )
    mean = _expanding(gv, "mean").sort_index().to_numpy()
    some = cnt.numpy() > 0
    np.testing.assert_array_equal(np.isnan(mean), ~some)
    np.testing.assert_array_equal(acc.numpy()[some] / cnt.numpy()[some], mean[some])


def _check_shift(pdf: pd.DataFrame, col: str, asc: bool, k: int,
                 hdf: Optional[HipDataFrame] = None) -> None:
    pdf = pdf.reset_index(drop=True)
    hdf, pk, perm, g = _sorted_perm(pdf, asc, hdf)
    for d in (k, -k):
        data, valid = dops.segmented_shift(perm, pk, hdf.col(col), d)
        exp = g[col].shift(d).sort_index()
        assert valid.dtype == torch.bool
        np.testing.assert_array_equal(valid.numpy(), exp.notna().to_numpy())
        ok = valid.numpy()
        np.testing.assert_array_equal(
            data.numpy()[ok], exp.to_numpy()[ok].astype(data.numpy().dtype)
        )
        for default in (7, -2.5):  # what the engine does with a default
            filled = torch.where(
                valid, data.to(torch.float64), torch.full((len(pdf),), float(default), dtype=torch.float64)
            )
            np.testing.assert_array_equal(
                filled.numpy(), exp.astype("float64").fillna(default).to_numpy()
            )


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("col", ["i", "f"])
def test_scan_matches_pandas(col, asc):
    _check_scan(_base_frame(1), col, asc)


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("col", ["i", "f"])
@pytest.mark.parametrize("k", [0, 1, 3, 1000])
def test_shift_matches_pandas(col, asc, k):
    _check_shift(_base_frame(2), col, asc, k)


def test_null_on_first_row_and_all_null_partition():
    pdf = pd.DataFrame(
        dict(
            k=[0, 0, 0, 0, 1, 1, 2, 2, 2],
            a=[1, 2, 3, 4, 1, 2, 1, 2, 3],
            f=[np.nan, 2.0, np.nan, -1.0, np.nan, np.nan, 5.0, np.nan, 5.5],
        )
    )
    _check_scan(pdf, "f", True)
    _check_scan(pdf, "f", False)
    for k in (0, 1, 3, 10):
        _check_shift(pdf, "f", True, k)
    hdf, pk, perm, _ = _sorted_perm(pdf, True)
    acc, cnt = dops.segmented_scan(perm, pk, hdf.col("f"), "min")
    assert cnt.tolist() == [0, 1, 1, 2, 0, 0, 1, 1, 2]
    assert acc.tolist() == [0.0, 2.0, 2.0, -1.0, 0.0, 0.0, 5.0, 5.0, 5.0]


def test_nan_counts_as_null():
    perm = torch.arange(5)
    pk = torch.zeros(5, dtype=torch.int64)
    f = torch.tensor([1.0, float("nan"), 3.0, float("nan"), -1.0], dtype=torch.float64)
    valid = torch.tensor([True, True, False, True, True])
    acc, cnt = dops.segmented_scan(perm, pk, (f, valid), "sum")
    assert cnt.tolist() == [1, 1, 1, 1, 2]
    assert acc.tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]
    acc, _ = dops.segmented_scan(perm, pk, (f, None), "max")
    assert acc.tolist() == [1.0, 1.0, 3.0, 3.0, 3.0]
    _, ok = dops.segmented_shift(perm, pk, (f, valid), 1)
    assert ok.tolist() == [False, True, False, False, False]
    # float32 widens
    acc, _ = dops.segmented_scan(perm, pk, (f.to(torch.float32), None), "min")
    assert acc.dtype == torch.float64 and acc.tolist() == [1.0, 1.0, 1.0, 1.0, -1.0]


def test_int64_max_next_to_null():
    pdf = pd.DataFrame(
        dict(
            k=[1, 1, 1, 1, 2, 2, 2],
            a=[1, 2, 3, 4, 1, 2, 3],
            i=pd.array(
                [INT64_MAX, None, 5, INT64_MAX, None, INT64_MAX, None],
                dtype="Int64",
            ),
        )
    )
    # built from tensors: the arrow loader routes nullable ints through
    # float64, which cannot hold INT64_MAX
    vals = [INT64_MAX, 0, 5, INT64_MAX, 0, INT64_MAX, 0]
    hdf = HipDataFrame.from_columns(
        dict(
            k=DeviceColumn(torch.tensor(pdf["k"].to_numpy()), None, pa.int64()),
            a=DeviceColumn(torch.tensor(pdf["a"].to_numpy()), None, pa.int64()),
            i=DeviceColumn(
                torch.tensor(vals, dtype=torch.int64),
                torch.tensor(pdf["i"].notna().to_numpy()),
                pa.int64(),
            ),
        ),
        Schema("k:long,a:long,i:long"),
        "cpu",
    )
    _, pk, perm, g = _sorted_perm(pdf, True, hdf)
    c = hdf.col("i")
    acc, cnt = dops.segmented_scan(perm, pk, c, "min")
    assert acc.tolist() == [INT64_MAX, INT64_MAX, 5, 5, 0, INT64_MAX, INT64_MAX]
    assert cnt.tolist() == [1, 1, 2, 3, 0, 1, 1]
    acc, _ = dops.segmented_scan(perm, pk, c, "max")
    assert acc.tolist() == [INT64_MAX] * 4 + [0, INT64_MAX, INT64_MAX]
    # the sum wraps exactly like pandas' int64 cumsum
    acc, _ = dops.segmented_scan(perm, pk, c, "sum")
    with np.errstate(over="ignore"):
        exp = g["i"].cumsum().sort_index()
    ok = pdf["i"].notna().to_numpy()
    np.testing.assert_array_equal(
        acc.numpy()[ok], exp.to_numpy(dtype="int64", na_value=0)[ok]
    )
    assert acc.tolist()[3] == (2 * INT64_MAX + 5 + 2 ** 63) % 2 ** 64 - 2 ** 63
    data, valid = dops.segmented_shift(perm, pk, c, 1)
    assert valid.tolist() == [False, True, False, True, False, False, True]
    assert data.tolist()[1] == INT64_MAX and data.tolist()[6] == INT64_MAX


def test_empty_and_bad_arguments():
    z = torch.zeros(0, dtype=torch.int64)
    acc, cnt = dops.segmented_scan(z, z, (z, None), "sum")
    assert acc.numel() == 0 and cnt.numel() == 0
    data, ok = dops.segmented_shift(z, z, (z.double(), None), 2)
    assert data.numel() == 0 and ok.dtype == torch.bool
    with pytest.raises(ValueError):
        dops.segmented_scan(z, z, (z, None), "avg")


# ------------------------------------------------------------------ #
# FugueSQL value windows                                               #
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
            v=rng.integers(0, 12, n).astype(np.float64) / 2,
            w=(rng.integers(0, 12, n) / 4).astype(np.float32),
        )
    )
    pdf["v"] = pdf["v"].mask(pdf.index % 8 == 0)
    pdf.loc[pdf["k"] == 2, "v"] = np.nan
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


ITEMS = [
    "LAG(v)", "LEAD(v)", "LAG(i)", "LAG(v, 0)", "LAG(i, 0)", "LAG(v, 3)",
    "LEAD(i, 2)", "LAG(v, 1000)", "LAG(v, 1, 9)", "LAG(v, 2, 0.5)",
    "LEAD(i, 1, 7)", "LEAD(i, 1, 7.5)", "LAG(w, 1, 2)", "LAG(j, 0, 3)",
    "SUM(v)", "SUM(i)", "SUM(j)", "MIN(v)", "MIN(i)", "MAX(v)", "MAX(w)",
    "COUNT(v)", "COUNT(i)", "COUNT(*)", "AVG(v)", "AVG(i)", "AVG(w)",
    "MEAN(j)",
]


@pytest.mark.parametrize("item", ITEMS)
@pytest.mark.parametrize(
    "over",
    [
        "PARTITION BY k ORDER BY a",
        "PARTITION BY s, k ORDER BY a DESC, v",
    ],
)
def test_sql_value_window_lowered(item, over):
    pdf = _sql_frame()
    e = HipExecutionEngine()
    got, exp = _both(f"SELECT *, {item} OVER ({over}) AS r FROM df", pdf, e)
    assert e.stats.get("window.device_value") == 1
    assert e.stats.get("window.device") == 0
    _assert_same(got, exp)


def test_sql_lag_without_order_by():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    got, exp = _both("SELECT k, v, LAG(v) OVER (PARTITION BY k) AS r FROM df", pdf, e)
    assert e.stats.get("window.device_value") == 1
    _assert_same(got, exp)


def test_sql_two_items_share_one_over():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    sql = (
        "SELECT k, a, LAG(v, 1, 0) OVER (PARTITION BY k ORDER BY a) AS p, v, "
        "SUM(v) OVER (PARTITION BY k ORDER BY a) AS t FROM df"
    )
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device_value") == 2
    assert e.stats.get("window.device") == 0
    assert got.schema == "k:long,a:long,p:double,v:double,t:double"
    _assert_same(got, exp)


def test_sql_value_window_after_where():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    sql = (
        "SELECT k, a, i, MAX(i) OVER (PARTITION BY k ORDER BY a) AS r, "
        "LEAD(i) OVER (PARTITION BY k ORDER BY a) AS q FROM df WHERE a > 1"
    )
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device_value") == 2
    assert got.schema == exp.schema
    assert _rows(got.as_pandas()) == _rows(exp.as_pandas())


def test_sql_value_window_types_match_executor():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    table = {
        "i": dict(lag="double", lag0="long", agg="long"),
        "j": dict(lag="double", lag0="int", agg="int"),
        "v": dict(lag="double", lag0="double", agg="double"),
        "w": dict(lag="float", lag0="float", agg="float"),
    }
    n = 0
    for c, t in table.items():
        cases = [
            (f"LAG({c})", t["lag"]), (f"LEAD({c}, 2, 1)", t["lag"]),
            (f"LAG({c}, 0)", t["lag0"]), (f"MIN({c})", t["agg"]),
            (f"MAX({c})", t["agg"]), (f"COUNT({c})", "double"),
            (f"AVG({c})", "double"), ("COUNT(*)", "long"),
        ]
        if c != "w":
            cases.append((f"SUM({c})", t["agg"]))
        for item, tp in cases:
            got, exp = _both(
                f"SELECT k, {item} OVER (PARTITION BY k ORDER BY a) AS r FROM df",
                pdf, e,
            )
            n += 1
            assert e.stats.get("window.device_value") == n, item
            assert str(got.schema["r"].type) == str(exp.schema["r"].type), item
            assert got.schema == exp.schema == f"k:long,r:{tp}", item


@pytest.mark.parametrize(
    "sql",
    [
        "SELECT k, SUM(v) OVER (PARTITION BY k) AS r FROM df",
        "SELECT k, LAG(v) OVER (ORDER BY a, i, v) AS r FROM df",
        "SELECT k, LAG(s) OVER (PARTITION BY k ORDER BY a, i) AS r FROM df",
        "SELECT k, LAG(b) OVER (PARTITION BY k ORDER BY a, i) AS r FROM df",
        "SELECT k, SUM(w) OVER (PARTITION BY k ORDER BY a) AS r FROM df",
        "SELECT k, LAG(v, -1) OVER (PARTITION BY k ORDER BY a) AS r FROM df",
        "SELECT k, LAG(v + 1) OVER (PARTITION BY k ORDER BY a) AS r FROM df",
        "SELECT k, LAG(v) OVER (PARTITION BY v ORDER BY a) AS r FROM df",
        "SELECT k, MIN(i) OVER (PARTITION BY k ORDER BY s, a) AS r FROM df",
        "SELECT k, LAG(v) OVER (PARTITION BY k + 1 ORDER BY a) AS r FROM df",
        "SELECT k, LAG(n) OVER (PARTITION BY k ORDER BY a) AS r FROM df",
        "SELECT k, SUM(n) OVER (PARTITION BY k ORDER BY a) AS r FROM df",
        "SELECT k, LAG(v) OVER (PARTITION BY k ORDER BY a) AS r, "
        "SUM(v) OVER (PARTITION BY k ORDER BY a DESC) AS t FROM df",
        "SELECT k, LAG(v) OVER (PARTITION BY k ORDER BY a) AS r, "
        "ROW_NUMBER() OVER (PARTITION BY k ORDER BY a) AS t FROM df",
        "SELECT k, FIRST_VALUE(v) OVER (PARTITION BY k ORDER BY a) AS r FROM df",
        "SELECT k, MAX(LAG(i) OVER (PARTITION BY k ORDER BY a)) AS r FROM df GROUP BY k",
    ],
    ids=[
        "agg-unordered", "no-partition", "string-value", "bool-value",
        "float-sum", "negative-k", "expr-arg", "float-key", "string-order",
        "expr-key", "nullable-int-lag", "nullable-int-sum", "two-overs",
        "mixed-ranking", "first-value", "group-by",
    ],
)
def test_sql_value_window_declined_shapes(sql):
    pdf = _sql_frame()
    pdf["b"] = pdf["a"] % 2 == 0
    pdf["n"] = pdf["i"].astype("Int64").mask(pdf.index % 5 == 0)
    # unique order inside a partition where a statement orders by (a, i)
    e = HipExecutionEngine()
    try:
        exp = fugue_sql(sql, df=pdf, engine=NativeExecutionEngine(), as_fugue=True)
    except Exception as ex:  # the host rejects the statement: so must we
        with pytest.raises(type(ex)):
            fugue_sql(sql, df=pdf, engine=e, as_fugue=True)
        assert e.stats.get("window.device_value") == 0
        return
    got = fugue_sql(sql, df=pdf, engine=e, as_fugue=True)
    assert e.stats.get("window.device_value") == 0
    assert e.stats.get("window.device") == 0
    if "(n)" not in sql:
        # (the engine hands a nullable integer column to the host executor
        # as float64, so those two come back double from this engine)
        assert got.schema == exp.schema
    assert _rows(got.as_pandas()) == _rows(exp.as_pandas())


def test_window_over_declines_directly():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    hdf = e.to_df(pdf)
    ok = ("r", "lag", "v", 1, None)
    for args in (
        (hdf, [], [("a", True)], [ok]),
        (hdf, ["k"], [("a", True)], []),
        (hdf, ["k"], [("a", True)], [("v", "lag", "v", 1, None)]),
        (hdf, ["k"], [("a", True)], [ok, ok]),
        (hdf, ["k"], [("a", True)], [("r", "lag", "v", -1, None)]),
        (hdf, ["k"], [("a", True)], [("r", "lag", "v", 1.5, None)]),
        (hdf, ["k"], [("a", True)], [("r", "lag", "v", 1, "x")]),
        (hdf, ["k"], [("a", True)], [("r", "first_value", "v", None, None)]),
        (hdf, ["k"], [("a", True)], [("r", "sum", None, None, None)]),
        (hdf, ["k"], [], [("r", "count", None, None, None)]),
        (hdf, ["k"], [("s", True)], [ok]),
        (hdf, ["v"], [("a", True)], [ok]),
    ):
        with pytest.raises(NotImplementedError):
            e.window_over(*args)
    empty = e.to_df(pdf.iloc[:0])
    with pytest.raises(NotImplementedError):
        e.window_over(empty, ["k"], [("a", True)], [ok])
    assert e.stats.get("window.device_value") == 0
    res = e.window_over(hdf, ["k"], [("a", True)], [ok, ("c", "count", None, None, None)])
    assert e.stats.get("window.device_value") == 2
    assert res.schema == hdf.schema + "r:double,c:long"


def test_reserved_temporary_name_in_input():
    pdf = _sql_frame()[["k", "a", "v"]]
    pdf["_fugue_window_value_2"] = 1
    e = HipExecutionEngine()
    sql = "SELECT k, a, LAG(v) OVER (PARTITION BY k ORDER BY a) AS r FROM df"
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device_value") == 0
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
    rng = np.random.default_rng(21)
    n = 1000
    pdf = pd.DataFrame(
        dict(
            k=rng.integers(0, 37, n),
            o=rng.permutation(n),  # unique: no ties across the shuffle
            v=rng.integers(-30, 30, n).astype(np.float64),
        )
    )
    pdf["v"] = pdf["v"].mask(pdf.index % 7 == 0)
    return pdf


_SPLITS = {"uneven": 700, "one-empty": 1000}
_DIST_ITEMS = [
    ("p", "lag", "v", 1, None),
    ("q", "lead", "v", 2, -1.0),
    ("t", "sum", "v", None, None),
    ("c", "count", "v", None, None),
    ("m", "avg", "v", None, None),
    ("x", "max", "v", None, None),
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
        shard = Hdf(part.reset_index(drop=True), "k:long,o:long,v:double", device="cpu")
        before = e.stats.get("window.device_value")
        res = e.window_over(shard, ["k"], [("o", False)], _DIST_ITEMS)
        assert e.stats.get("window.device_value") == before + len(_DIST_ITEMS)
        assert e.stats.get("window.device") == 0
        out[name] = res.as_pandas().to_dict("list")
    return out


def test_distributed_window_over():
    results = run_distributed(_dist_job, 29567)
    pdf = _dist_frame()
    g = pdf.sort_values("o", ascending=False, kind="stable").groupby("k", sort=False)["v"]
    exp = pdf.assign(
        p=g.shift(1).sort_index(),
        q=g.shift(-2).fillna(-1.0).sort_index(),
        t=g.cumsum().sort_index(),
        c=_expanding(g, "count").sort_index(),
        m=_expanding(g, "mean").sort_index(),
        x=g.cummax().sort_index(),
    )
    for name in _SPLITS:
        shards = [pd.DataFrame(results[r][name]) for r in range(2)]
        allr = pd.concat(shards)
        assert len(allr) == len(pdf)
        assert list(allr.columns) == list(exp.columns)
        assert _rows(allr) == _rows(exp)
        # every partition lives on one rank
        assert set(shards[0]["k"]).isdisjoint(set(shards[1]["k"]))
