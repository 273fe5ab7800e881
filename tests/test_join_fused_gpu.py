"""GPU tests of the fused join + filter + projection of the engine
(``HipExecutionEngine.join_select`` through the SQL planner) and of the
join build-table memo (``ops._JOIN_BUILD_MEMO``).

Every result is compared with the same SQL run with ``FUGUE_JOIN_FUSED=0``
(the join and the select one after the other), as sorted row sets: keys,
counts and dimension values exactly, sums within the tolerance the replay
tests use for sums (``allclose(rtol=1e-12)`` with torch's default
``atol=1e-8``), because the group-by's add order is not fixed."""
import gc

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

import fugue_amd.api as fa
from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine

RTOL, ATOL = 1e-12, 1e-8

FLAGSHIP = """
agg = SELECT k, SUM(v) AS s, COUNT(v) AS n FROM fact GROUP BY k
res = SELECT agg.k, s, n, w FROM agg INNER JOIN dims ON agg.k = dims.k
      WHERE s > w
YIELD DATAFRAME AS result
"""


@pytest.fixture(autouse=True)
def _fresh_memo(monkeypatch):
    monkeypatch.delenv("FUGUE_JOIN_FUSED", raising=False)
    monkeypatch.delenv("FUGUE_JOIN_BUILD_MEMO", raising=False)
    dops._JOIN_BUILD_MEMO.clear()
    yield
    dops._JOIN_BUILD_MEMO.clear()


@pytest.fixture(scope="module")
def tables():
    rng = np.random.default_rng(11)
    fact = pd.DataFrame(
        dict(k=rng.integers(0, 1000, 20_000), v=rng.random(20_000))
    )
    w = rng.random(1000)
    return fact, w


def _run(engine, fact, dims, sql=FLAGSHIP, **tables_):
    out = fa.fugue_sql(
        sql, fact=fact, dims=dims, engine=engine, as_fugue=True, **tables_
    )
    return out.as_pandas().sort_values("k").reset_index(drop=True)


def _same(a: pd.DataFrame, b: pd.DataFrame) -> None:
    assert list(a.columns) == list(b.columns)
    assert len(a) == len(b)
    for name in a.columns:
        if name == "s":
            np.testing.assert_allclose(
                a[name].values, b[name].values, rtol=RTOL, atol=ATOL
            )
        else:
            np.testing.assert_array_equal(a[name].values, b[name].values)


def _both(monkeypatch, fact, dims):
    """(fused result, unfused result, fused engine's counters)"""
    e1 = HipExecutionEngine()
    d1 = e1.to_df(dims)
    fused = _run(e1, fact, d1)
    monkeypatch.setenv("FUGUE_JOIN_FUSED", "0")
    e0 = HipExecutionEngine()
    plain = _run(e0, fact, e0.to_df(dims))
    monkeypatch.delenv("FUGUE_JOIN_FUSED")
    assert e0.stats.get("join.fused_select") == 0
    assert e0.stats.get("joins") == e1.stats.get("joins") == 1
    return fused, plain, e1.stats.snapshot()


def test_flagship_sql_fused_equals_unfused(monkeypatch, tables):
    fact, w = tables
    dims = pd.DataFrame(dict(k=np.arange(1000), w=w))
    fused, plain, stats = _both(monkeypatch, fact, dims)
    assert stats.get("join.fused_select") == 1
    assert len(fused) == 1000  # this predicate passes every row
    _same(fused, plain)
    want = fact.groupby("k", as_index=False).agg(s=("v", "sum"), n=("v", "count"))
    np.testing.assert_array_equal(fused["n"].values, want["n"].values)
    np.testing.assert_allclose(fused["s"].values, want["s"].values,
                               rtol=RTOL, atol=ATOL)


def test_predicate_rejects_rows(monkeypatch, tables):
    fact, w = tables
    # sums are about 10 (20 rows of mean 0.5 per key): w in [0, 20) rejects
    # about half the rows
    dims = pd.DataFrame(dict(k=np.arange(1000), w=w * 20.0))
    s = fact.groupby("k")["v"].sum().reindex(np.arange(1000)).values
    gap = np.abs(s - dims["w"].values)
    assert (gap > 100 * (ATOL + RTOL * np.abs(s))).all(), "a row sits on the edge"
    fused, plain, stats = _both(monkeypatch, fact, dims)
    assert stats.get("join.fused_select") == 1
    assert len(fused) == int((s > dims["w"].values).sum())
    assert 300 < len(fused) < 700
    _same(fused, plain)
    np.testing.assert_array_equal(
        fused["k"].values, np.flatnonzero(s > dims["w"].values)
    )
    np.testing.assert_array_equal(
        fused["w"].values, dims["w"].values[fused["k"].values]
    )


def test_duplicate_build_key_takes_the_unfused_path(monkeypatch, tables):
    fact, w = tables
    k = np.arange(1000)
    k[999] = 5  # key 5 twice, key 999 absent
    dims = pd.DataFrame(dict(k=k, w=w))
    e1 = HipExecutionEngine()
    d1 = e1.to_df(dims)
    first = _run(e1, fact, d1)
    again = _run(e1, fact, d1)  # the memo knows the flag now
    assert e1.stats.get("join.fused_select") == 0
    assert e1.stats.get("joins") == 2
    monkeypatch.setenv("FUGUE_JOIN_FUSED", "0")
    e0 = HipExecutionEngine()
    plain = _run(e0, fact, e0.to_df(dims))
    assert len(first) == 1000 and (first["k"] == 5).sum() == 2
    for got in (first, again):
        got = got.sort_values(["k", "w"]).reset_index(drop=True)
        _same(got, plain.sort_values(["k", "w"]).reset_index(drop=True))


def test_build_memo_hits_and_dead_tensor_misses(tables):
    fact, w = tables
    engine = HipExecutionEngine()
    dims = engine.to_df(pd.DataFrame(dict(k=np.arange(1000), w=w)))
    a = _run(engine, fact, dims)
    assert engine.stats.get("join.build_memo_miss") == 1
    assert engine.stats.get("join.build_memo_hit") == 0
    b = _run(engine, fact, dims)
    assert engine.stats.get("join.build_memo_miss") == 1
    assert engine.stats.get("join.build_memo_hit") == 1
    assert engine.stats.get("join.fused_select") == 2
    _same(a, b)
    (ref, tab), = list(dops._JOIN_BUILD_MEMO.values())
    assert ref() is dims.col("k").data and tab.dup == 0


def test_dead_key_tensor_never_hits():
    """a new tensor of the same size, at the same address or not, is a
    miss once the memoized one is gone, and joins by its own values"""
    from fugue_amd.utils.stats import EngineStats

    stats = EngineStats()
    probe = torch.arange(0, 3000, dtype=torch.int64, device="cuda")
    keys = torch.arange(0, 2000, dtype=torch.int64, device="cuda")
    vals = torch.arange(0, 2000, dtype=torch.float64, device="cuda")
    specs = [(0, probe), (1, vals)]
    first = dops.join_unique_select(probe, keys, None, specs, stats)
    again = dops.join_unique_select(probe, keys, None, specs, stats)
    assert stats.get("join.build_memo_miss") == 1
    assert stats.get("join.build_memo_hit") == 1
    assert first[0].numel() == again[0].numel() == 2000
    addr = keys.data_ptr()
    (key, (ref, _)), = list(dops._JOIN_BUILD_MEMO.items())
    del keys
    gc.collect()
    assert ref() is None
    keys2 = torch.arange(1000, 3000, dtype=torch.int64, device="cuda")
    out = dops.join_unique_select(probe, keys2, None, specs, stats)
    assert stats.get("join.build_memo_miss") == 2
    assert stats.get("join.build_memo_hit") == 1
    pk, bv = out[0].cpu().numpy(), out[1].cpu().numpy()
    order = np.argsort(pk)
    np.testing.assert_array_equal(pk[order], np.arange(1000, 3000))
    np.testing.assert_array_equal(bv[order], np.arange(2000, dtype=np.float64))
    if keys2.data_ptr() == addr:  # the allocator handed the block out again
        assert key in dops._JOIN_BUILD_MEMO
    # hash_join_indices shares the memo
    pi, bi = dops.hash_join_indices(probe, keys2, "inner", stats=stats)
    assert stats.get("join.build_memo_hit") == 2
    assert pi.numel() == 2000


def test_memo_knob_off_builds_every_time(monkeypatch, tables):
    fact, w = tables
    monkeypatch.setenv("FUGUE_JOIN_BUILD_MEMO", "0")
    engine = HipExecutionEngine()
    dims = engine.to_df(pd.DataFrame(dict(k=np.arange(1000), w=w)))
    a = _run(engine, fact, dims)
    b = _run(engine, fact, dims)
    assert engine.stats.get("join.build_memo_hit") == 0
    assert len(dops._JOIN_BUILD_MEMO) == 0
    assert engine.stats.get("join.fused_select") == 2
    _same(a, b)


THREE = """
res = SELECT a.k1, x, y, z FROM a INNER JOIN b ON a.k1 = b.k1
      INNER JOIN c ON b.k2 = c.k2 WHERE x > z
YIELD DATAFRAME AS result
"""


def test_three_table_join_with_where(monkeypatch):
    rng = np.random.default_rng(3)
    a = pd.DataFrame(dict(k1=np.arange(3000), x=rng.random(3000)))
    b = pd.DataFrame(dict(k1=rng.permutation(4000)[:3500],
                          k2=rng.integers(0, 500, 3500), y=rng.random(3500)))
    c = pd.DataFrame(dict(k2=rng.permutation(600)[:450], z=rng.random(450)))

    def run(engine):
        out = fa.fugue_sql(THREE, a=a, b=b, c=c, engine=engine, as_fugue=True)
        return out.as_pandas().sort_values("k1").reset_index(drop=True)

    e1 = HipExecutionEngine()
    fused = run(e1)
    monkeypatch.setenv("FUGUE_JOIN_FUSED", "0")
    e0 = HipExecutionEngine()
    plain = run(e0)
    assert e1.stats.get("join.fused_select") == 1  # the last join only
    assert e1.stats.get("joins") == e0.stats.get("joins") == 2
    want = a.merge(b, on="k1").merge(c, on="k2")
    want = want[want.x > want.z].sort_values("k1").reset_index(drop=True)
    assert len(fused) == len(want) > 0
    for got in (fused, plain):
        assert list(got.columns) == ["k1", "x", "y", "z"]
        for name in got.columns:
            np.testing.assert_array_equal(got[name].values, want[name].values)
