"""The planner hands the last join its consumer (``engine.join_select``)
only for an inner join followed by plain columns and at most one
comparison; every other plan shape, and an engine without the entry point
or one that declines, joins and selects apart as before.  CPU only."""
import numpy as np
import pandas as pd
import pytest

import fugue_amd.api as fa
from fugue_amd.column.expressions import col, lit
from fugue_amd.column.sql import SelectColumns
from fugue_amd.execution.native_execution_engine import NativeExecutionEngine
from fugue_amd.hip.execution_engine import (
    HipExecutionEngine,
    _post_join_request,
)
from fugue_amd.sql.executor import parse_select
from fugue_amd.sql.planner import UnsupportedPlan, execute_plan


class _Spy(NativeExecutionEngine):
    """records what the planner asks for; answers ``join_select`` the slow
    way, or declines when ``decline`` is set"""

    def __init__(self, decline: bool = False):
        super().__init__()
        self.calls = []
        self.decline = decline

    def join(self, df1, df2, how, on=None):
        self.calls.append(("join", how))
        return super().join(df1, df2, how=how, on=on)

    def select(self, df, cols, where=None, having=None):
        self.calls.append(("select", where is not None))
        return super().select(df, cols, where=where, having=having)

    def join_select(self, df1, df2, how, on, cols, where=None):
        self.calls.append(("join_select", how, where is not None))
        if self.decline:
            raise NotImplementedError("declined")
        joined = NativeExecutionEngine.join(self, df1, df2, how=how, on=on)
        return NativeExecutionEngine.select(self, joined, cols, where=where)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(0)
    a = pd.DataFrame(dict(k=np.arange(50), s=rng.random(50), n=np.arange(50) % 7))
    d = pd.DataFrame(dict(k=np.arange(10, 70), w=rng.random(60)))
    c = pd.DataFrame(dict(n=np.arange(7), z=rng.random(7)))
    return a, d, c


def _plan(sql, engine, frames):
    a, d, c = frames
    tables = dict(a=engine.to_df(a), d=engine.to_df(d), c=engine.to_df(c))
    res = execute_plan(parse_select(sql), tables, engine)
    return res.as_pandas()


def _kinds(engine):
    return [c[0] for c in engine.calls]


BASE = "SELECT a.k, s, w FROM a INNER JOIN d ON a.k = d.k"


@pytest.mark.parametrize(
    "sql,has_where",
    [
        (BASE, False),
        (BASE + " WHERE s > w", True),
        # a single-table comparison is pushed below the join: none is left
        (BASE + " WHERE s <= 0.5", False),
        # the key belongs to both tables, so this one stays above the join
        (BASE + " WHERE 20 <= k", True),
        ("SELECT a.k AS key, w AS weight FROM a INNER JOIN d ON a.k = d.k "
         "WHERE s > w", True),
    ],
)
def test_hands_over_in_the_plain_shape(frames, sql, has_where):
    spy = _Spy()
    got = _plan(sql, spy, frames)
    assert spy.calls[-1] == ("join_select", "inner", has_where)
    assert "join" not in _kinds(spy)
    plain = _plan(sql, NativeExecutionEngine(), frames)
    pd.testing.assert_frame_equal(
        got.sort_values(got.columns[0]).reset_index(drop=True),
        plain.sort_values(plain.columns[0]).reset_index(drop=True),
    )


@pytest.mark.parametrize(
    "sql",
    [
        # an expression in the select list
        "SELECT a.k, s + w AS t FROM a INNER JOIN d ON a.k = d.k",
        # a window
        "SELECT a.k, s, ROW_NUMBER() OVER (PARTITION BY n ORDER BY s) AS r "
        "FROM a INNER JOIN d ON a.k = d.k",
        # two residual conjuncts
        BASE + " WHERE s > w AND s + w < 1.5",
        # an expression inside the comparison
        BASE + " WHERE s + 1 > w",
        # a left join
        "SELECT a.k, s, w FROM a LEFT JOIN d ON a.k = d.k",
        # aggregate, distinct, star
        "SELECT n, SUM(w) AS t FROM a INNER JOIN d ON a.k = d.k GROUP BY n",
        "SELECT DISTINCT n FROM a INNER JOIN d ON a.k = d.k",
        "SELECT * FROM a INNER JOIN d ON a.k = d.k",
    ],
)
def test_does_not_hand_over(frames, sql):
    spy = _Spy()
    try:
        got = _plan(sql, spy, frames)
    except UnsupportedPlan:
        # the planner lowers no window over a join at all (the statement
        # goes to the host executor); it has joined by then
        assert "OVER" in sql
        got = None
    assert "join_select" not in _kinds(spy)
    assert "join" in _kinds(spy)
    if got is None:
        return
    plain = _plan(sql, NativeExecutionEngine(), frames)
    key = list(got.columns)
    pd.testing.assert_frame_equal(
        got.sort_values(key).reset_index(drop=True),
        plain.sort_values(key).reset_index(drop=True),
    )


def test_only_the_last_join_gets_the_consumer(frames):
    sql = ("SELECT a.k, s, w, z FROM a INNER JOIN d ON a.k = d.k "
           "INNER JOIN c ON a.n = c.n WHERE s > z")
    spy = _Spy()
    got = _plan(sql, spy, frames)
    kinds = [k for k in _kinds(spy) if k != "select"]
    assert kinds == ["join", "join_select"]
    a, d, c = frames
    want = a.merge(d, on="k").merge(c, on="n")
    want = want[want.s > want.z]
    assert len(got) == len(want) > 0


def test_a_declining_engine_falls_back_to_join_then_select(frames):
    spy = _Spy(decline=True)
    got = _plan(BASE + " WHERE s > w", spy, frames)
    kinds = _kinds(spy)
    assert kinds.index("join_select") < kinds.index("join")
    assert spy.calls[-1] == ("select", True)
    plain = _plan(BASE + " WHERE s > w", NativeExecutionEngine(), frames)
    pd.testing.assert_frame_equal(
        got.sort_values("k").reset_index(drop=True),
        plain.sort_values("k").reset_index(drop=True),
    )


def test_request_shapes_the_engine_takes():
    k, s, w = col("k"), col("s"), col("w")
    r = _post_join_request(SelectColumns(k, s.alias("t")), s > w)
    assert r.columns == [("k", "k"), ("s", "t")]
    assert r.where == (4, [("col", "s"), ("col", "w")])
    assert _post_join_request(SelectColumns(k), None).where is None
    assert _post_join_request(SelectColumns(k), lit(2) <= w).where == (
        3, [("lit", 2), ("col", "w")])
    for cols, where in [
        (SelectColumns(k, (s + w).alias("t")), None),
        (SelectColumns(k, s.cast("int")), None),
        (SelectColumns(k), (s > w) & (s < 1)),
        (SelectColumns(k), s + 1 > w),
        (SelectColumns(k), s > "x"),
        (SelectColumns(k), s > True),
        (SelectColumns(k), s > (1 << 64)),
        (SelectColumns(*[col(f"c{i}") for i in range(9)]), None),
    ]:
        assert _post_join_request(cols, where) is None


FLAGSHIP = """
agg = SELECT k, SUM(v) AS s, COUNT(v) AS n FROM fact GROUP BY k
res = SELECT agg.k, s, n, w FROM agg INNER JOIN dims ON agg.k = dims.k
      WHERE s > w
YIELD DATAFRAME AS result
"""


@pytest.mark.parametrize("knob", [None, "0"])
def test_hip_engine_on_host_tensors_equals_native(monkeypatch, knob):
    """CPU-tensor frames never take the fused kernel: join_select runs the
    join and the select apart and gives the native engine's rows (on a GPU
    host the same frames are device frames and do take it)"""
    if knob is not None:
        monkeypatch.setenv("FUGUE_JOIN_FUSED", knob)
    else:
        monkeypatch.delenv("FUGUE_JOIN_FUSED", raising=False)
    rng = np.random.default_rng(0)
    fact = pd.DataFrame(dict(k=rng.integers(0, 1000, 20000), v=rng.random(20000)))
    dims = pd.DataFrame(dict(k=np.arange(1000), w=rng.random(1000) * 20))
    engine = HipExecutionEngine()
    got = fa.fugue_sql(FLAGSHIP, fact=fact, dims=dims, engine=engine,
                       as_fugue=True).as_pandas()
    want = fa.fugue_sql(FLAGSHIP, fact=fact, dims=dims, engine="native",
                        as_fugue=True).as_pandas()
    fused = 0 if engine.device == "cpu" or knob == "0" else 1
    assert engine.stats.get("join.fused_select") == fused
    assert engine.stats.get("joins") == 1
    assert 300 < len(got) < 700
    got = got.sort_values("k").reset_index(drop=True)
    want = want.sort_values("k").reset_index(drop=True)
    assert list(got.columns) == list(want.columns) == ["k", "s", "n", "w"]
    for name in ("k", "n", "w"):
        np.testing.assert_array_equal(got[name].values, want[name].values)
    # sums: the tolerance of the replay tests (the add order is not fixed)
    np.testing.assert_allclose(got["s"].values, want["s"].values,
                               rtol=1e-12, atol=1e-8)
