"""Segmented rank / per-partition take: torch-CPU implementations against
a pandas oracle, the HipExecutionEngine take and ranking-window paths on
CPU tensors, the FugueSQL lowering, and a world-2 gloo run."""
import os
import pickle
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch
import torch.multiprocessing as mp

import fugue_amd.api as fa
from fugue_amd.execution.native_execution_engine import NativeExecutionEngine
from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
from fugue_amd.schema import Schema
from fugue_amd.sql.api import fugue_sql

INT64_MAX = np.iinfo(np.int64).max
KINDS = ["row_number", "rank", "dense_rank"]


# ------------------------------------------------------------------ #
# ops layer vs pandas                                                  #
# ------------------------------------------------------------------ #
def _frame(pdf: pd.DataFrame) -> HipDataFrame:
    return HipDataFrame(pdf, device="cpu")


def _pkeys(hdf: HipDataFrame, keys: List[str]) -> torch.Tensor:
    pk, _ = dops.pack_keys([hdf.col(k) for k in keys])
    return pk.contiguous()


def _oracle_sorted(
    pdf: pd.DataFrame, keys: List[str], by: List[str], asc: List[bool],
    na_position: str = "last",
) -> pd.DataFrame:
    """Stable sort by order columns, then grouped in that order."""
    s = pdf
    if by:
        s = pdf.sort_values(
            by, ascending=asc, kind="stable", na_position=na_position
        )
    return s


def _oracle_ranks(
    pdf: pd.DataFrame, keys: List[str], by: List[str], asc: List[bool]
) -> Dict[str, np.ndarray]:
    s = _oracle_sorted(pdf, keys, by, asc)
    g = s.groupby(keys, dropna=False, sort=False)
    out = {"row_number": (g.cumcount() + 1).sort_index().to_numpy()}
    if len(by) == 1:
        col = g[by[0]]
        for kind, method in (("rank", "min"), ("dense_rank", "dense")):
            r = col.rank(method=method, ascending=asc[0], na_option="bottom")
            out[kind] = r.sort_index().to_numpy().astype(np.int64)
    else:
        # several order columns: s is sorted by them, so numbering the
        # distinct tuples in order of appearance gives a code that sorts
        # like the tuple; rank that code inside each partition
        code = s.groupby(by, dropna=False, sort=False).ngroup()
        tmp = s.assign(__code=code.to_numpy())
        col = tmp.groupby(keys, dropna=False, sort=False)["__code"]
        for kind, method in (("rank", "min"), ("dense_rank", "dense")):
            r = col.rank(method=method, ascending=True)
            out[kind] = r.sort_index().to_numpy().astype(np.int64)
    return out


def _check_ranks(
    pdf: pd.DataFrame, keys: List[str], by: List[str], asc: List[bool],
    hdf: Optional[HipDataFrame] = None,
) -> None:
    pdf = pdf.reset_index(drop=True)
    hdf = hdf if hdf is not None else _frame(pdf)
    pk = _pkeys(hdf, keys)
    perm = dops.sort_indices_exact(hdf, by, asc, "last", key_tensor=pk)
    expected = _oracle_ranks(pdf, keys, by, asc)
    for kind in KINDS:
        got = dops.segmented_rank(
            perm, pk, [hdf.col(c) for c in by], kind
        )
        assert got.dtype == torch.int64
        np.testing.assert_array_equal(got.numpy(), expected[kind], err_msg=kind)


def _check_take(
    pdf: pd.DataFrame, keys: List[str], by: List[str], asc: List[bool],
    n: int, na_position: str = "last",
) -> None:
    pdf = pdf.reset_index(drop=True)
    hdf = _frame(pdf)
    pk = _pkeys(hdf, keys)
    perm = dops.sort_indices_exact(hdf, by, asc, na_position, key_tensor=pk)
    idx = dops.take_per_group_indices(perm, pk, n)
    s = _oracle_sorted(pdf, keys, by, asc, na_position)
    exp = s.groupby(keys, dropna=False, sort=False).head(n).index.to_numpy()
    assert sorted(idx.tolist()) == sorted(exp.tolist())
    # emitted in sorted order: partitions contiguous, presort kept inside
    got = pdf.iloc[idx.numpy()]
    for _, sub in got.groupby(keys, dropna=False, sort=False):
        want = [i for i in s.index if i in set(sub.index)]
        assert list(sub.index) == want


def _base_frame(seed: int = 0, n: int = 400) -> pd.DataFrame:
    rng = np.random.default_rng(seed)
    return pd.DataFrame(
        dict(
            k=rng.integers(0, 9, n),
            a=rng.integers(0, 6, n),  # many duplicates: tie rule
            f=rng.integers(0, 8, n).astype(np.float64) / 2,
        )
    )


@pytest.mark.parametrize("asc", [True, False])
def test_ranks_int_order_key(asc):
    _check_ranks(_base_frame(1), ["k"], ["a"], [asc])


@pytest.mark.parametrize("asc", [True, False])
def test_ranks_float_order_key(asc):
    _check_ranks(_base_frame(2), ["k"], ["f"], [asc])


def test_ranks_two_order_keys():
    _check_ranks(_base_frame(3), ["k"], ["a", "f"], [True, False])


def test_ranks_nulls_in_keys_and_order():
    pdf = _base_frame(4)
    pdf["k"] = pdf["k"].astype("Int64").mask(pdf.index % 7 == 0)
    pdf["a"] = pdf["a"].astype("Int64").mask(pdf.index % 5 == 0)
    _check_ranks(pdf, ["k"], ["a"], [True])
    _check_ranks(pdf, ["k"], ["a"], [False])
    for n in (1, 2):
        _check_take(pdf, ["k"], ["a"], [True], n, "last")
        _check_take(pdf, ["k"], ["a"], [True], n, "first")
        _check_take(pdf, ["k"], ["a"], [False], n, "first")


def test_ranks_nan_order_values():
    pdf = _base_frame(5)
    pdf.loc[pdf.index % 4 == 0, "f"] = np.nan
    # pandas reads NaN as null: NaN rows sort last and are peers
    _check_ranks(pdf, ["k"], ["f"], [True])
    _check_ranks(pdf, ["k"], ["f"], [False])
    _check_take(pdf, ["k"], ["f"], [True], 3, "first")


def test_nan_is_peer_of_nan_but_not_of_null():
    data = torch.tensor([float("nan"), float("nan"), 0.0, -0.0, float("nan")])
    valid = torch.tensor([True, True, True, True, False])
    pk = torch.zeros(5, dtype=torch.int64)
    perm = torch.tensor([2, 3, 0, 1, 4])
    r = dops.segmented_rank(perm, pk, [(data.double(), valid)], "rank")
    assert r.tolist() == [3, 3, 1, 1, 5]
    d = dops.segmented_rank(perm, pk, [(data.double(), valid)], "dense_rank")
    assert d.tolist() == [2, 2, 1, 1, 3]


def test_int64_max_next_to_null():
    pdf = pd.DataFrame(
        dict(
            k=[1, 1, 1, 1, 2, 2, 2],
            a=pd.array(
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
            a=DeviceColumn(
                torch.tensor(vals, dtype=torch.int64),
                torch.tensor(pdf["a"].notna().to_numpy()),
                pa.int64(),
            ),
        ),
        Schema("k:long,a:long"),
        "cpu",
    )
    _check_ranks(pdf, ["k"], ["a"], [True], hdf)
    _check_ranks(pdf, ["k"], ["a"], [False], hdf)
    pk = _pkeys(hdf, ["k"])
    # nulls last: INT64_MAX sorts before the null, not among the nulls
    perm = dops.sort_indices_exact(hdf, ["a"], [True], "last", key_tensor=pk)
    assert perm.tolist() == [2, 0, 3, 1, 5, 4, 6]
    perm = dops.sort_indices_exact(hdf, ["a"], [True], "first", key_tensor=pk)
    assert perm.tolist() == [1, 2, 0, 3, 4, 6, 5]
    perm = dops.sort_indices_exact(hdf, ["a"], [False], "last", key_tensor=pk)
    assert perm.tolist() == [0, 3, 2, 1, 5, 4, 6]
    r = dops.segmented_rank(perm, pk, [hdf.col("a")], "rank")
    assert r.tolist() == [1, 4, 3, 1, 2, 1, 2]


def test_inf_next_to_null():
    pdf = pd.DataFrame(
        dict(k=[1, 1, 1, 1], f=[np.inf, np.nan, -np.inf, np.inf])
    )
    _check_ranks(pdf, ["k"], ["f"], [True])
    _check_ranks(pdf, ["k"], ["f"], [False])


@pytest.mark.parametrize("n", [0, 1, 3, 10_000])
def test_take_sizes(n):
    pdf = _base_frame(6)
    _check_take(pdf, ["k"], ["a"], [True], n)
    _check_take(pdf, ["k"], ["a", "f"], [False, True], n)
    _check_take(pdf, ["k"], [], [], n)  # no presort: first n rows per group


def test_tie_rule_is_original_row_order():
    pdf = pd.DataFrame(dict(k=[0] * 6 + [1] * 4, a=[1] * 10))
    hdf = _frame(pdf)
    pk = _pkeys(hdf, ["k"])
    perm = dops.sort_indices_exact(hdf, ["a"], [False], "last", key_tensor=pk)
    assert dops.take_per_group_indices(perm, pk, 2).tolist() == [0, 1, 6, 7]
    rn = dops.segmented_rank(perm, pk, [hdf.col("a")], "row_number")
    assert rn.tolist() == [1, 2, 3, 4, 5, 6, 1, 2, 3, 4]
    rk = dops.segmented_rank(perm, pk, [hdf.col("a")], "rank")
    assert rk.tolist() == [1] * 10


def test_empty_frame():
    pdf = pd.DataFrame(
        dict(k=pd.Series([], dtype="int64"), a=pd.Series([], dtype="int64"))
    )
    hdf = _frame(pdf)
    pk = _pkeys(hdf, ["k"])
    perm = dops.sort_indices_exact(hdf, ["a"], [True], "last", key_tensor=pk)
    assert perm.numel() == 0
    for kind in KINDS:
        assert dops.segmented_rank(perm, pk, [hdf.col("a")], kind).numel() == 0
    assert dops.take_per_group_indices(perm, pk, 3).numel() == 0


def test_bad_arguments():
    z = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        dops.segmented_rank(z, z, [], "ntile")
    with pytest.raises(ValueError):
        dops.sort_indices_exact(_frame(_base_frame()), ["a"], [True], "middle")


# ------------------------------------------------------------------ #
# engine: fa.take with partition                                       #
# ------------------------------------------------------------------ #
def _rows(pdf: pd.DataFrame) -> List[Tuple]:
    def _norm(v: Any) -> Any:
        if pd.isna(v):
            return None
        if isinstance(v, (int, float, np.integer, np.floating)):
            return float(v)  # nullable ints come back as float
        return v

    return sorted(
        (tuple(_norm(v) for v in r) for r in pdf.itertuples(index=False)),
        key=repr,
    )


def _engine_frame() -> pd.DataFrame:
    rng = np.random.default_rng(7)
    n = 600
    pdf = pd.DataFrame(
        dict(
            k=rng.integers(0, 11, n),
            s=rng.choice(["x", "yy", "zzz", "w"], n),
            v=rng.permutation(n).astype(np.float64),  # unique: exact sets
            w=rng.permutation(n),
        )
    )
    pdf["v"] = pdf["v"].mask(pdf.index % 9 == 0)
    return pdf


def _pandas_take(
    pdf: pd.DataFrame, n: int, by: List[str], asc: List[bool],
    keys: List[str], na_position: str = "last",
) -> pd.DataFrame:
    s = pdf
    if by:
        s = pdf.sort_values(
            by, ascending=asc, na_position=na_position, kind="stable"
        )
    return s.groupby(keys, dropna=False, sort=False).head(n)


@pytest.mark.parametrize(
    "keys,presort,by,asc,na_position",
    [
        (["k"], "v desc", ["v"], [False], "last"),
        (["s"], "v", ["v"], [True], "last"),
        (["k", "s"], "v desc, w", ["v", "w"], [False, True], "last"),
        (["k"], "v", ["v"], [True], "first"),
        (["s"], "v desc", ["v"], [False], "first"),
        (["k"], "", [], [], "last"),
    ],
    ids=["int", "str", "int+str", "int-nafirst", "str-nafirst", "nopresort"],
)
def test_engine_take_partitioned(monkeypatch, keys, presort, by, asc, na_position):
    pdf = _engine_frame()
    e = HipExecutionEngine()
    hdf = e.to_df(pdf)
    assert isinstance(hdf, HipDataFrame)
    calls: List[int] = []
    orig = HipDataFrame.as_pandas

    def _spy(self):
        calls.append(1)
        return orig(self)

    before = e.stats.get("take.device_partitioned")
    monkeypatch.setattr(HipDataFrame, "as_pandas", _spy)
    res = fa.take(
        hdf, 3, presort=presort, na_position=na_position,
        partition=dict(by=keys), engine=e, as_fugue=True,
    )
    n_calls = len(calls)
    monkeypatch.undo()
    assert n_calls == 0, "partitioned take left the device"
    assert e.stats.get("take.device_partitioned") == before + 1
    assert isinstance(res, HipDataFrame)
    expected = _pandas_take(pdf, 3, by, asc, keys, na_position)
    assert _rows(res.as_pandas()) == _rows(expected)


def test_engine_take_null_keys_form_a_group():
    pdf = _engine_frame()
    pdf["k"] = pdf["k"].astype("Int64").mask(pdf.index % 6 == 0)
    e = HipExecutionEngine()
    before = e.stats.get("take.device_partitioned")
    res = fa.take(
        e.to_df(pdf), 2, presort="w", partition=dict(by=["k"]),
        engine=e, as_fugue=True,
    )
    assert e.stats.get("take.device_partitioned") == before + 1
    expected = _pandas_take(pdf, 2, ["w"], [True], ["k"])
    assert _rows(res.as_pandas()) == _rows(expected)


def test_engine_take_partition_presort_and_fallbacks():
    pdf = _engine_frame()
    e = HipExecutionEngine()
    # presort from the partition spec
    res = fa.take(
        e.to_df(pdf), 2, presort=None,
        partition=dict(by=["k"], presort="w desc"), engine=e, as_fugue=True,
    )
    assert e.stats.get("take.device_partitioned") == 1
    assert _rows(res.as_pandas()) == _rows(
        _pandas_take(pdf, 2, ["w"], [False], ["k"])
    )
    # string presort keeps the host path and its answer
    res = fa.take(
        e.to_df(pdf), 1, presort="s, w", partition=dict(by=["k"]),
        engine=e, as_fugue=True,
    )
    assert e.stats.get("take.device_partitioned") == 1
    assert _rows(res.as_pandas()) == _rows(
        _pandas_take(pdf, 1, ["s", "w"], [True, True], ["k"])
    )


# ------------------------------------------------------------------ #
# FugueSQL ranking windows                                             #
# ------------------------------------------------------------------ #
def _sql_frame() -> pd.DataFrame:
    rng = np.random.default_rng(11)
    n = 300
    pdf = pd.DataFrame(
        dict(
            k=rng.integers(0, 7, n),
            s=rng.choice(["p", "q", "r"], n),
            a=rng.integers(0, 5, n),
            v=rng.integers(0, 12, n).astype(np.float64),
        )
    )
    pdf["v"] = pdf["v"].mask(pdf.index % 8 == 0)
    return pdf


def _both(sql: str, pdf: pd.DataFrame, e: HipExecutionEngine):
    got = fugue_sql(sql, df=pdf, engine=e, as_fugue=True)
    exp = fugue_sql(sql, df=pdf, engine=NativeExecutionEngine(), as_fugue=True)
    return got, exp


@pytest.mark.parametrize("fn", ["ROW_NUMBER", "RANK", "DENSE_RANK"])
@pytest.mark.parametrize(
    "over",
    [
        "PARTITION BY k ORDER BY v DESC",
        "PARTITION BY s ORDER BY a, v DESC",
        "PARTITION BY k, s ORDER BY a ASC",
    ],
)
def test_sql_window_lowered(fn, over):
    pdf = _sql_frame()
    e = HipExecutionEngine()
    sql = f"SELECT *, {fn}() OVER ({over}) AS r FROM df"
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device") == 1
    assert got.schema == exp.schema
    gp, ep = got.as_pandas(), exp.as_pandas()
    if fn == "ROW_NUMBER":
        # ties are numbered in original row order on both paths, and the
        # lowered frame keeps the input row order
        pd.testing.assert_frame_equal(gp, ep, check_dtype=False)
    assert _rows(gp) == _rows(ep)


def test_sql_window_types_match_executor():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    for fn, tp in (("ROW_NUMBER", "long"), ("RANK", "double"), ("DENSE_RANK", "long")):
        got, exp = _both(
            f"SELECT k, {fn}() OVER (PARTITION BY k ORDER BY a) AS r FROM df",
            pdf, e,
        )
        assert str(got.schema["r"].type) == str(exp.schema["r"].type)
        assert got.schema == exp.schema == f"k:long,r:{tp}"
    assert e.stats.get("window.device") == 3


def test_sql_top_k_subquery():
    pdf = _sql_frame()
    pdf["u"] = np.random.default_rng(3).permutation(len(pdf))
    e = HipExecutionEngine()
    sql = (
        "SELECT k, s, u FROM (SELECT *, ROW_NUMBER() OVER "
        "(PARTITION BY k ORDER BY u DESC) AS rn FROM df) WHERE rn <= 3"
    )
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device") == 1
    assert got.schema == exp.schema
    assert _rows(got.as_pandas()) == _rows(exp.as_pandas())
    assert got.count() == 3 * pdf["k"].nunique()


def test_sql_window_after_where():
    pdf = _sql_frame()
    e = HipExecutionEngine()
    sql = (
        "SELECT k, a, DENSE_RANK() OVER (PARTITION BY k ORDER BY a) AS r "
        "FROM df WHERE a > 1"
    )
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device") == 1
    assert got.schema == exp.schema
    assert _rows(got.as_pandas()) == _rows(exp.as_pandas())


@pytest.mark.parametrize(
    "sql",
    [
        "SELECT k, a, LAG(a) OVER (PARTITION BY k ORDER BY a, v) AS r FROM df",
        "SELECT k, a, SUM(a) OVER (PARTITION BY k) AS r FROM df",
        "SELECT k, ROW_NUMBER() OVER (PARTITION BY k ORDER BY a) AS r1, "
        "RANK() OVER (PARTITION BY k ORDER BY a) AS r2 FROM df",
        "SELECT k, RANK() OVER (PARTITION BY k + 1 ORDER BY a) AS r FROM df",
    ],
    ids=["lag", "agg-window", "two-windows", "expr-key"],
)
def test_sql_window_fallback_shapes(sql):
    pdf = _sql_frame()[["k", "a", "v"]].dropna()
    e = HipExecutionEngine()
    got, exp = _both(sql, pdf, e)
    assert e.stats.get("window.device") == 0
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
    return pd.DataFrame(
        dict(
            k=rng.integers(0, 37, n),
            s=rng.choice(["a", "bb", "ccc"], n),
            v=rng.permutation(n).astype(np.float64),
        )
    )


_SPLITS = {"uneven": 700, "one-empty": 1000}


def _dist_job(rank: int):
    from fugue_amd.hip.execution_engine import HipExecutionEngine as Eng
    from fugue_amd.hip.frame import HipDataFrame as Hdf

    e = Eng()
    assert e.is_distributed and e.world_size == 2
    pdf = _dist_frame()
    out: Dict[str, Any] = {}
    for name, cut in _SPLITS.items():
        part = pdf.iloc[:cut] if rank == 0 else pdf.iloc[cut:]
        shard = Hdf(part.reset_index(drop=True), "k:long,s:str,v:double", device="cpu")
        for keys in (["k"], ["s", "k"]):
            before = e.stats.get("take.device_partitioned")
            res = fa.take(
                shard, 2, presort="v desc", partition=dict(by=keys),
                engine=e, as_fugue=True,
            )
            assert e.stats.get("take.device_partitioned") == before + 1
            out[f"take/{name}/{'+'.join(keys)}"] = res.as_pandas().to_dict("list")
        ranked = e.rank_over(shard, ["k"], [("v", False)], "row_number", "rn")
        out[f"rank/{name}"] = ranked.as_pandas().to_dict("list")
    return out


def test_distributed_take_and_rank():
    results = run_distributed(_dist_job, 29561)
    pdf = _dist_frame()
    for name in _SPLITS:
        for keys in (["k"], ["s", "k"]):
            key = f"take/{name}/{'+'.join(keys)}"
            shards = [pd.DataFrame(results[r][key]) for r in range(2)]
            expected = _pandas_take(pdf, 2, ["v"], [False], keys)
            # globally correct and sharded: the shards add up to the
            # answer exactly once, and each partition lives on one rank
            assert len(shards[0]) + len(shards[1]) == len(expected)
            assert _rows(pd.concat(shards)) == _rows(expected)
            g0 = set(map(tuple, shards[0][keys].drop_duplicates().to_numpy()))
            g1 = set(map(tuple, shards[1][keys].drop_duplicates().to_numpy()))
            assert g0.isdisjoint(g1)
            assert len(shards[0]) > 0 and len(shards[1]) > 0
        shards = [pd.DataFrame(results[r][f"rank/{name}"]) for r in range(2)]
        allr = pd.concat(shards)
        assert len(allr) == len(pdf)
        exp = pdf.assign(
            rn=pdf.groupby("k")["v"].rank(method="first", ascending=False).astype("int64")
        )
        assert _rows(allr) == _rows(exp)
