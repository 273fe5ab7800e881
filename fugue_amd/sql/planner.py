"""SQL plan → ExecutionEngine lowering.

Takes the parsed ``SelectStmt`` AST (``fugue_amd/sql/executor.py``) and
executes it through ``ExecutionEngine`` relational ops (join / filter /
select / aggregate / union / take), so a FugueSQL SELECT runs on the HIP
engine's device kernels with the distributed shuffle — instead of
gathering to pandas.  Raises :class:`UnsupportedPlan` for shapes outside
the lowering (CASE/LIKE, non-equi joins, correlated subqueries, ...); the
SQL facet then falls back to the pandas executor.
"""
from typing import Any, Dict, List, Optional, Tuple

from fugue_amd.column import functions as F
from fugue_amd.column.expressions import ColumnExpr, col, lit
from fugue_amd.column.sql import SelectColumns
from fugue_amd.dataframe.dataframe import DataFrame
from fugue_amd.schema import Schema
from fugue_amd.sql import executor as X


class UnsupportedPlan(Exception):
    pass


def _to_column_expr(e: X.Expr, schema: Schema, alias_map: Dict[str, str]) -> ColumnExpr:
    if isinstance(e, X.ColRef):
        name = e.name
        if name not in schema:
            raise UnsupportedPlan(f"column {name} not in {schema}")
        return col(name)
    if isinstance(e, X.Lit):
        v = e.value
        if v is None or isinstance(v, (bool, int, float, str)):
            return lit(v)
        raise UnsupportedPlan(f"literal {v!r}")
    if isinstance(e, X.BinOp):
        l = _to_column_expr(e.left, schema, alias_map)
        r = _to_column_expr(e.right, schema, alias_map)
        op = e.op
        if op == "AND":
            return l & r
        if op == "OR":
            return l | r
        m = {
            "+": lambda: l + r,
            "-": lambda: l - r,
            "*": lambda: l * r,
            "/": lambda: l / r,
            "=": lambda: l == r,
            "==": lambda: l == r,
            "<>": lambda: l != r,
            "!=": lambda: l != r,
            "<": lambda: l < r,
            "<=": lambda: l <= r,
            ">": lambda: l > r,
            ">=": lambda: l >= r,
        }
        if op not in m:
            raise UnsupportedPlan(f"operator {op}")
        return m[op]()
    if isinstance(e, X.UnOp):
        inner = _to_column_expr(e.operand, schema, alias_map)
        if e.op == "-":
            return -inner
        if e.op == "NOT":
            return ~inner
        if e.op == "ISNULL":
            return inner.is_null()
        if e.op == "NOTNULL":
            return inner.not_null()
        raise UnsupportedPlan(f"unary {e.op}")
    if isinstance(e, X.Between):
        inner = _to_column_expr(e.expr, schema, alias_map)
        lo = _to_column_expr(e.low, schema, alias_map)
        hi = _to_column_expr(e.high, schema, alias_map)
        res = (inner >= lo) & (inner <= hi)
        return ~res if e.negate else res
    if isinstance(e, X.InList):
        inner = _to_column_expr(e.expr, schema, alias_map)
        res: Optional[ColumnExpr] = None
        for v in e.values:
            term = inner == _to_column_expr(v, schema, alias_map)
            res = term if res is None else (res | term)
        if res is None:
            raise UnsupportedPlan("empty IN list")
        return ~res if e.negate else res
    if isinstance(e, X.Cast):
        inner = _to_column_expr(e.expr, schema, alias_map)
        try:
            return inner.cast(e.type_name)
        except Exception:
            raise UnsupportedPlan(f"cast to {e.type_name}")
    if isinstance(e, X.FuncCall):
        name = e.name
        if name in ("SUM", "MIN", "MAX", "AVG", "COUNT", "FIRST", "LAST"):
            if len(e.args) != 1:
                raise UnsupportedPlan(f"{name} with {len(e.args)} args")
            arg = e.args[0]
            if isinstance(arg, X.Star):
                if name != "COUNT":
                    raise UnsupportedPlan(f"{name}(*)")
                inner = col("*")
            else:
                inner = _to_column_expr(arg, schema, alias_map)
            fn = {
                "SUM": F.sum,
                "MIN": F.min,
                "MAX": F.max,
                "AVG": F.avg,
                "COUNT": F.count_distinct if e.distinct else F.count,
                "FIRST": F.first,
                "LAST": F.last,
            }[name]
            if e.distinct and name in ("FIRST", "LAST"):
                # FIRST/LAST over a deduplicated argument has no device
                # decomposition and silently dropping the qualifier can
                # change the answer — route to the host executor instead
                raise UnsupportedPlan(f"{name}(DISTINCT ...)")
            res = fn(inner)
            if e.distinct and name in ("SUM", "AVG", "MIN", "MAX"):
                from fugue_amd.column.expressions import _UnaryAggFuncExpr

                res = _UnaryAggFuncExpr(name, inner, arg_distinct=True)
            return res
        if name == "COALESCE":
            return F.coalesce(
                *[_to_column_expr(a, schema, alias_map) for a in e.args]
            )
        raise UnsupportedPlan(f"function {name}")
    if isinstance(e, X.Like):
        inner = _to_column_expr(e.expr, schema, alias_map)
        res = F.like(inner, e.pattern)
        return ~res if e.negate else res
    if isinstance(e, X.Case):
        whens = [
            (
                _to_column_expr(c, schema, alias_map),
                _to_column_expr(v, schema, alias_map),
            )
            for c, v in e.whens
        ]
        else_ = (
            _to_column_expr(e.else_, schema, alias_map)
            if e.else_ is not None
            else lit(None)
        )
        return F.case_when(*whens, else_=else_)
    raise UnsupportedPlan(f"expression {type(e).__name__}")


_JOIN_MAP = {
    "inner": "inner",
    "left": "left_outer",
    "right": "right_outer",
    "outer": "full_outer",
    "cross": "cross",
    "semi": "semi",
    "anti": "anti",
}


def _extract_on_names(on: X.Expr) -> List[Tuple[str, str]]:
    """ON must be a conjunction of colA = colB equalities."""
    pairs: List[Tuple[str, str]] = []

    def _walk(e: X.Expr) -> None:
        if isinstance(e, X.BinOp) and e.op == "AND":
            _walk(e.left)
            _walk(e.right)
            return
        if (
            isinstance(e, X.BinOp)
            and e.op in ("=", "==")
            and isinstance(e.left, X.ColRef)
            and isinstance(e.right, X.ColRef)
        ):
            pairs.append((e.left.name, e.right.name))
            return
        raise UnsupportedPlan("non-equi join condition")

    _walk(on)
    return pairs


def execute_plan(
    stmt: X.SelectStmt, tables: Dict[str, DataFrame], engine: Any
) -> DataFrame:
    """Execute the statement on the engine; raises UnsupportedPlan."""
    res = _execute_core(stmt, tables, engine)
    for op, all_, rhs in stmt.set_ops:
        other = _execute_core(rhs, tables, engine)
        if op == "UNION":
            res = engine.union(res, other, distinct=not all_)
        elif op == "INTERSECT":
            res = engine.intersect(res, other, distinct=True)
        elif op == "EXCEPT":
            res = engine.subtract(res, other, distinct=True)
    if stmt.order_by or stmt.limit is not None:
        res = _order_limit(res, stmt, engine)
    return res


def _order_limit(res: DataFrame, stmt: X.SelectStmt, engine: Any) -> DataFrame:
    for o in stmt.order_by:
        if not isinstance(o.expr, X.ColRef):
            raise UnsupportedPlan("ORDER BY must use output columns")
    if stmt.limit is not None and stmt.order_by:
        presort = ",".join(
            f"{o.expr.name} {'asc' if o.asc else 'desc'}" for o in stmt.order_by
        )
        return engine.take(res, stmt.limit, presort=presort)
    # full sort (no limit) or limit without order: do it locally (results
    # at this point are post-projection; a full global sort is a later
    # optimization)
    local = res.as_local_bounded() if hasattr(res, "as_local_bounded") else res
    pdf = local.as_pandas()
    if stmt.order_by:
        pdf = pdf.sort_values(
            [o.expr.name for o in stmt.order_by],
            ascending=[o.asc for o in stmt.order_by],
        ).reset_index(drop=True)
    if stmt.limit is not None:
        pdf = pdf.head(stmt.limit)
    from fugue_amd.dataframe.pandas_dataframe import PandasDataFrame

    return engine.to_df(PandasDataFrame(pdf, res.schema))


def _resolve_from(item: X.FromItem, tables: Dict[str, DataFrame], engine: Any) -> DataFrame:
    if item.subquery is not None:
        return execute_plan(item.subquery, tables, engine)
    if item.table not in tables:
        raise UnsupportedPlan(f"table {item.table} not found")
    return engine.to_df(tables[item.table])


def _split_conjuncts(e: Optional[X.Expr]) -> List[X.Expr]:
    if e is None:
        return []
    if isinstance(e, X.BinOp) and e.op == "AND":
        return _split_conjuncts(e.left) + _split_conjuncts(e.right)
    return [e]


def _mentioned_cols(e: X.Expr) -> List[str]:
    out: List[str] = []

    def _walk(x: X.Expr) -> None:
        if isinstance(x, X.ColRef):
            out.append(x.name)
        elif isinstance(x, X.BinOp):
            _walk(x.left)
            _walk(x.right)
        elif isinstance(x, X.UnOp):
            _walk(x.operand)
        elif isinstance(x, X.Between):
            _walk(x.expr)
            _walk(x.low)
            _walk(x.high)
        elif isinstance(x, X.InList):
            _walk(x.expr)
            for v in x.values:
                _walk(v)
        elif isinstance(x, X.Cast):
            _walk(x.expr)
        elif isinstance(x, X.FuncCall):
            for a in x.args:
                _walk(a)
        elif isinstance(x, X.Like):
            _walk(x.expr)
        elif isinstance(x, X.Case):
            for cnd, val in x.whens:
                _walk(cnd)
                _walk(val)
            if x.else_ is not None:
                _walk(x.else_)

    _walk(e)
    return out


def _needed_columns(
    stmt: X.SelectStmt, where: Optional[X.Expr]
) -> Optional[set]:
    """All column names the statement can reference; None when a ``*``
    makes every column live.  ``where`` is the residual (post-pushdown)
    predicate — columns only used by already-pushed filters are dead."""
    needed: set = set()
    for e, _alias in stmt.columns:
        if isinstance(e, X.Star):
            return None
        needed.update(_mentioned_cols(e))
    for e in (where, stmt.having):
        if e is not None:
            needed.update(_mentioned_cols(e))
    for e in stmt.group_by:
        if not isinstance(e, X.Star):
            needed.update(_mentioned_cols(e))
    for o in stmt.order_by:
        needed.update(_mentioned_cols(o.expr))
    for j in stmt.joins:
        if j.on is not None:
            needed.update(_mentioned_cols(j.on))
        if j.using is not None:
            needed.update(j.using)
    return needed


_WINDOW_TMP = "_fugue_window_rank_"

# Ranking windows the engine computes with its segmented rank kernels.
# The lowered column keeps the type the pandas executor gives the same
# text (measured on ``executor.WindowFunc.eval``): ROW_NUMBER is
# ``cumcount() + 1`` and DENSE_RANK a ``cumsum`` of int64 flags, both
# long; RANK goes through ``where``/``ffill`` and comes out double.
# ``engine.rank_over`` yields exactly those types.  (Over an empty frame
# the executor returns an empty float64 series for all three, so
# ``rank_over`` declines empty input and the statement falls back.)
_RANKING_WINDOWS = {
    "ROW_NUMBER": "row_number",
    "RANK": "rank",
    "DENSE_RANK": "dense_rank",
}


def _find_ranking_window(
    stmt: X.SelectStmt, schema: Schema
) -> Optional[Tuple[int, str, List[str], List[Tuple[str, bool]]]]:
    """(select index, kind, partition columns, order (column, asc) pairs)
    of the statement's single lowerable ranking window; None when the
    select list has no window item.  Raises UnsupportedPlan for every
    other window shape."""
    found = [
        i for i, (e, _a) in enumerate(stmt.columns)
        if isinstance(e, X.WindowFunc)
    ]
    if len(found) == 0:
        return None
    if len(found) > 1:
        raise UnsupportedPlan("more than one window item")
    if stmt.group_by or stmt.having is not None or stmt.distinct:
        raise UnsupportedPlan("window with GROUP BY/HAVING/DISTINCT")
    if stmt.joins:
        raise UnsupportedPlan("window over a join")
    w = stmt.columns[found[0]][0]
    kind = _RANKING_WINDOWS.get(w.func.name)
    if kind is None or len(w.func.args) > 0 or w.func.distinct:
        raise UnsupportedPlan(f"window function {w.func.name}")
    pcols: List[str] = []
    for e in w.partition_by:
        if not isinstance(e, X.ColRef) or e.name not in schema:
            raise UnsupportedPlan("PARTITION BY expression")
        pcols.append(e.name)
    if len(pcols) == 0:
        raise UnsupportedPlan("window without PARTITION BY")
    ocols: List[Tuple[str, bool]] = []
    for o in w.order_by:
        if not isinstance(o.expr, X.ColRef) or o.expr.name not in schema:
            raise UnsupportedPlan("window ORDER BY expression")
        ocols.append((o.expr.name, bool(o.asc)))
    if kind != "row_number" and len(ocols) == 0:
        raise UnsupportedPlan(f"{w.func.name} requires ORDER BY")
    if _WINDOW_TMP in schema:
        raise UnsupportedPlan("reserved column name in input")
    return found[0], kind, pcols, ocols


_VALUE_TMP = "_fugue_window_value_"  # + the select index of the item

# Value windows the engine computes with its segmented shift and scan
# kernels (``engine.window_over``).  With ORDER BY the aggregates are
# running ones.  Result types measured on ``executor.WindowFunc.eval``
# for a null-free integer column / a double column (nulls allowed) / a
# float column:
#
#   function            byte,short,int,long   double    float
#   LAG/LEAD(x, k>=1)   double                double    float
#   LAG/LEAD(x, 0)      the input type        double    float
#   SUM MIN MAX         the input type        double    float
#   COUNT(x)            double                double    double
#   AVG(x)              double                double    double
#   COUNT(*)            long                  long      long
#
# LAG/LEAD go through ``shift``, which turns integers into float64 as
# soon as one row has no source (k >= 1 on a non-empty frame); a default
# (``fillna``) does not turn them back.  SUM is ``cumsum`` in the input
# type (int sums wrap); COUNT(x) and AVG are ``expanding().count()`` /
# ``.mean()``, always float64.  An integer column that carries nulls
# reaches the executor as a nullable or float series with other result
# types, a float SUM accumulates in float32 and a bool column keeps bool:
# ``window_over`` declines those, and the statement falls back.
_VALUE_WINDOWS = {
    "LAG": "lag",
    "LEAD": "lead",
    "SUM": "sum",
    "MIN": "min",
    "MAX": "max",
    "COUNT": "count",
    "AVG": "avg",
    "MEAN": "avg",
}


def _window_over_clause(
    w: X.WindowFunc, schema: Schema
) -> Tuple[List[str], List[Tuple[str, bool]]]:
    pcols: List[str] = []
    for e in w.partition_by:
        if not isinstance(e, X.ColRef) or e.name not in schema:
            raise UnsupportedPlan("PARTITION BY expression")
        pcols.append(e.name)
    if len(pcols) == 0:
        raise UnsupportedPlan("window without PARTITION BY")
    ocols: List[Tuple[str, bool]] = []
    for o in w.order_by:
        if not isinstance(o.expr, X.ColRef) or o.expr.name not in schema:
            raise UnsupportedPlan("window ORDER BY expression")
        ocols.append((o.expr.name, bool(o.asc)))
    return pcols, ocols


# Whole-partition windows the engine computes with its segmented total
# kernels (``engine.partition_over``): an aggregate without ORDER BY
# (``transform`` over the partition) and FIRST_VALUE/LAST_VALUE with or
# without one (``transform("first"|"last")``: the first/last non-null
# value, given to every row).  Result types measured on
# ``executor.WindowFunc.eval`` for a null-free integer column / a double
# column (nulls allowed) / a float column:
#
#   function            byte,short,int        long     double    float
#   SUM                 the input type (*)    long     double    float
#   MIN MAX             the input type        long     double    float
#   FIRST_/LAST_VALUE   the input type        long     double    float
#   COUNT(x)            long                  long     long      long
#   AVG(x)              double                double   double    float
#   COUNT(*)            long                  long     long      long
#
# (*) pandas sums in int64 and narrows the result back only when every
# partition's total fits the input type; otherwise the column is long.
# ``partition_over`` makes the same test.  COUNT(x) is an integer here
# (the running one is ``expanding().count()``, double).  Over an all-null
# partition SUM is 0 and COUNT 0, the others are null.  SUM and AVG of a
# float column accumulate in float32, an integer column that carries
# nulls arrives as another type and bool keeps bool: ``partition_over``
# declines those (and an empty frame, typed double), and the statement
# falls back.
_PARTITION_WINDOWS = {
    "SUM": "sum",
    "MIN": "min",
    "MAX": "max",
    "COUNT": "count",
    "AVG": "avg",
    "MEAN": "avg",
}
_PARTITION_ORDERED_WINDOWS = {
    "FIRST_VALUE": "first_value",
    "FIRST": "first_value",
    "LAST_VALUE": "last_value",
    "LAST": "last_value",
}


def _find_partition_windows(
    stmt: X.SelectStmt, schema: Schema
) -> Optional[Tuple[List[str], List[Tuple[str, bool]], Dict[int, Tuple]]]:
    """(partition columns, order (column, asc) pairs, {select index:
    ``partition_over`` item}) when every window item of the statement is a
    whole-partition window, all share one OVER clause and the statement
    has the plain shape the lowering needs.  None otherwise: the value
    and ranking lowerings look at the statement next, and what they do
    not take falls back to the host."""
    found = [
        i for i, (e, _a) in enumerate(stmt.columns)
        if isinstance(e, X.WindowFunc)
    ]
    if len(found) == 0:
        return None
    if stmt.group_by or stmt.having is not None or stmt.distinct or stmt.joins:
        return None
    over: Optional[Tuple[List[str], List[Tuple[str, bool]]]] = None
    items: Dict[int, Tuple] = {}
    for i in found:
        w = stmt.columns[i][0]
        fname = w.func.name
        if fname in _PARTITION_ORDERED_WINDOWS:
            func = _PARTITION_ORDERED_WINDOWS[fname]
        elif fname in _PARTITION_WINDOWS and len(w.order_by) == 0:
            func = _PARTITION_WINDOWS[fname]
        else:
            return None  # a running or ranking item: not this lowering
        if w.func.distinct or len(w.func.args) != 1:
            return None
        try:
            this = _window_over_clause(w, schema)
        except UnsupportedPlan:
            return None
        if over is not None and this != over:
            return None
        over = this
        arg: Optional[str] = None
        a0 = w.func.args[0]
        if isinstance(a0, X.Star):
            if func != "count":
                return None
        elif isinstance(a0, X.ColRef) and a0.name in schema:
            arg = a0.name
        else:
            return None
        name = f"{_VALUE_TMP}{i}"
        if name in schema:
            return None
        items[i] = (name, func, arg)
    assert over is not None
    return over[0], over[1], items


# Framed windows (an explicit ``ROWS`` frame) the engine computes with its
# segmented frame kernel, or with the scan / total kernels where the frame
# is one of theirs (``engine.frame_over``).  They have plain SQL null
# semantics, not the pandas ones of the unframed forms above: nulls are
# skipped, COUNT is never null and everything else is null exactly when
# the frame holds no value.  Result types of ``executor.WindowFunc.
# _eval_frame``; they depend on the column type and the frame shape only,
# never on the data:
#
#   function                   null-free byte,short,int,long       double,
#                              frame always    frame that can      float
#                              holds the row   be empty
#   SUM MIN MAX                long            double              double
#   FIRST_/LAST_VALUE          long            double              double
#   COUNT(x) COUNT(*)          long            long                long
#   AVG(x)                     double          double              double
#
# A frame always holds the current row when lo <= 0 <= hi (an unbounded
# side counts as satisfied).  Integers are computed in int64 (SUM wraps)
# and converted at the end; float is widened to double before anything is
# added.  An integer column that carries nulls reaches the executor as
# another series type (double results): ``frame_over`` declines it, as it
# does strings, bools, dates, the half-unbounded frames other than
# UNBOUNDED PRECEDING..CURRENT ROW and a reach beyond the kernel's, and
# the statement falls back.
_FRAME_WINDOWS = dict(_PARTITION_WINDOWS, **_PARTITION_ORDERED_WINDOWS)


def _find_frame_windows(
    stmt: X.SelectStmt, schema: Schema
) -> Optional[Tuple[List[str], List[Tuple[str, bool]], Dict[int, Tuple]]]:
    """(partition columns, order (column, asc) pairs, {select index:
    ``frame_over`` item}) when every window item of the statement carries
    a ``ROWS`` frame, all share one OVER clause (the frames may differ)
    and the statement has the plain shape the lowering needs.  None when
    no window item carries a frame: the other lowerings look at the
    statement next.  Raises UnsupportedPlan for every other statement
    with a framed item, so none of them ever sees one."""
    found = [
        i for i, (e, _a) in enumerate(stmt.columns)
        if isinstance(e, X.WindowFunc)
    ]
    if not any(stmt.columns[i][0].frame is not None for i in found):
        return None
    if stmt.group_by or stmt.having is not None or stmt.distinct:
        raise UnsupportedPlan("window with GROUP BY/HAVING/DISTINCT")
    if stmt.joins:
        raise UnsupportedPlan("window over a join")
    over: Optional[Tuple[List[str], List[Tuple[str, bool]]]] = None
    items: Dict[int, Tuple] = {}
    for i in found:
        w = stmt.columns[i][0]
        if w.frame is None:
            raise UnsupportedPlan("framed and unframed window items")
        func = _FRAME_WINDOWS.get(w.func.name)
        if func is None or w.func.distinct or len(w.func.args) != 1:
            raise UnsupportedPlan(f"framed window function {w.func.name}")
        this = _window_over_clause(w, schema)
        if over is not None and this != over:
            raise UnsupportedPlan("window items with different OVER clauses")
        over = this
        arg: Optional[str] = None
        a0 = w.func.args[0]
        if isinstance(a0, X.Star):
            if func != "count":
                raise UnsupportedPlan(f"{w.func.name}(*)")
        elif isinstance(a0, X.ColRef) and a0.name in schema:
            arg = a0.name
        else:
            raise UnsupportedPlan("window argument expression")
        name = f"{_VALUE_TMP}{i}"
        if name in schema:
            raise UnsupportedPlan("reserved column name in input")
        items[i] = (name, func, arg, w.frame[0], w.frame[1])
    assert over is not None
    return over[0], over[1], items


def _find_value_windows(
    stmt: X.SelectStmt, schema: Schema
) -> Optional[Tuple[List[str], List[Tuple[str, bool]], Dict[int, Tuple]]]:
    """(partition columns, order (column, asc) pairs, {select index:
    ``window_over`` item}) when every window item of the statement is a
    value window and all share one OVER clause.  None when the select list
    has no value window (ranking windows are looked for next); raises
    UnsupportedPlan for a value window outside the lowering."""
    found = [
        i for i, (e, _a) in enumerate(stmt.columns)
        if isinstance(e, X.WindowFunc)
    ]
    if not any(
        stmt.columns[i][0].func.name in _VALUE_WINDOWS for i in found
    ):
        return None
    if stmt.group_by or stmt.having is not None or stmt.distinct:
        raise UnsupportedPlan("window with GROUP BY/HAVING/DISTINCT")
    if stmt.joins:
        raise UnsupportedPlan("window over a join")
    over: Optional[Tuple[List[str], List[Tuple[str, bool]]]] = None
    items: Dict[int, Tuple] = {}
    for i in found:
        w = stmt.columns[i][0]
        func = _VALUE_WINDOWS.get(w.func.name)
        if func is None or w.func.distinct:
            raise UnsupportedPlan(f"window function {w.func.name}")
        this = _window_over_clause(w, schema)
        if over is not None and this != over:
            raise UnsupportedPlan("window items with different OVER clauses")
        over = this
        args = w.func.args
        if len(args) == 0 or len(args) > (3 if func in ("lag", "lead") else 1):
            raise UnsupportedPlan(f"{w.func.name} with {len(args)} args")
        arg: Optional[str] = None
        if isinstance(args[0], X.Star):
            if func != "count":
                raise UnsupportedPlan(f"{w.func.name}(*)")
        elif isinstance(args[0], X.ColRef) and args[0].name in schema:
            arg = args[0].name
        else:
            raise UnsupportedPlan("window argument expression")
        if func not in ("lag", "lead") and len(this[1]) == 0:
            raise UnsupportedPlan("whole-partition aggregate window")
        k: Optional[int] = None
        default: Any = None
        if len(args) > 1:
            if not isinstance(args[1], X.Lit):
                raise UnsupportedPlan("LAG/LEAD offset is not a literal")
            k = args[1].value
            if isinstance(k, bool) or not isinstance(k, int) or k < 0:
                raise UnsupportedPlan("LAG/LEAD offset")
        if len(args) > 2:
            if not isinstance(args[2], X.Lit):
                raise UnsupportedPlan("LAG/LEAD default is not a literal")
            default = args[2].value
            if default is not None and (
                isinstance(default, bool)
                or not isinstance(default, (int, float))
            ):
                raise UnsupportedPlan("LAG/LEAD default")
        name = f"{_VALUE_TMP}{i}"
        if name in schema:
            raise UnsupportedPlan("reserved column name in input")
        items[i] = (name, func, arg, k, default)
    assert over is not None
    return over[0], over[1], items


_COMPARISONS = ("=", "==", "<>", "!=", "<", "<=", ">", ">=")


def _plain_join_consumer(
    stmt: X.SelectStmt, residual_where: Optional[X.Expr]
) -> bool:
    """True when all that follows the joins is a projection of plain
    columns (no window, group-by, distinct or expression) and the WHERE
    left after pushdown is absent or one comparison of columns and
    numeric literals: the shape an engine's ``join_select`` takes."""
    if stmt.distinct or stmt.group_by or stmt.having is not None:
        return False
    if len(stmt.columns) == 0 or not all(
        isinstance(e, X.ColRef) for e, _ in stmt.columns
    ):
        return False
    if residual_where is None:
        return True
    w = residual_where
    if not isinstance(w, X.BinOp) or w.op not in _COMPARISONS:
        return False
    for side in (w.left, w.right):
        if isinstance(side, X.ColRef):
            continue
        if (
            isinstance(side, X.Lit)
            and isinstance(side.value, (int, float))
            and not isinstance(side.value, bool)
        ):
            continue
        return False
    return True


def _join_with_consumer(
    stmt: X.SelectStmt,
    residual_where: Optional[X.Expr],
    left: DataFrame,
    right: DataFrame,
    keys: List[str],
    engine: Any,
) -> Optional[DataFrame]:
    """The last (inner) join together with the statement's projection and
    residual WHERE through ``engine.join_select``; None when the engine
    has no such entry point or declines the request, and the caller joins
    and selects apart."""
    join_select = getattr(engine, "join_select", None)
    if join_select is None:
        return None
    from fugue_amd.dataframe.utils import get_join_schemas

    _, schema = get_join_schemas(left, right, how="inner", on=keys)
    where_expr = (
        None
        if residual_where is None
        else _to_column_expr(residual_where, schema, {})
    )
    cols: List[ColumnExpr] = []
    for e, alias in stmt.columns:
        ce = _to_column_expr(e, schema, {})
        cols.append(ce if alias is None else ce.alias(alias))
    try:
        return join_select(
            left, right, "inner", keys, SelectColumns(*cols), where_expr
        )
    except NotImplementedError:
        return None


def _execute_core(
    stmt: X.SelectStmt, tables: Dict[str, DataFrame], engine: Any
) -> DataFrame:
    if stmt.from_item is None:
        raise UnsupportedPlan("SELECT without FROM")
    res = _resolve_from(stmt.from_item, tables, engine)
    # predicate pushdown: when ALL joins are inner, single-table conjuncts
    # of WHERE filter their source table before the joins
    join_inputs: List[DataFrame] = []
    residual_where: Optional[X.Expr] = stmt.where
    pushed: Dict[int, List[X.Expr]] = {}
    all_inner = all(j.how == "inner" for j in stmt.joins)
    if stmt.joins and all_inner and stmt.where is not None:
        frames: List[DataFrame] = [res] + [
            _resolve_from(j.item, tables, engine) for j in stmt.joins
        ]
        remaining: List[X.Expr] = []
        for conj in _split_conjuncts(stmt.where):
            cols = set(_mentioned_cols(conj))
            target = None
            for idx, fr in enumerate(frames):
                if cols <= set(fr.schema.names):
                    # unique owner only (ambiguous cols stay post-join)
                    owners = [
                        i
                        for i, f2 in enumerate(frames)
                        if cols <= set(f2.schema.names)
                    ]
                    if len(owners) == 1:
                        target = idx
                    break
            if target is None:
                remaining.append(conj)
            else:
                pushed.setdefault(target, []).append(conj)
        res = frames[0]
        join_inputs = frames[1:]
        residual_where = None
        for conj in remaining:
            residual_where = (
                conj
                if residual_where is None
                else X.BinOp("AND", residual_where, conj)
            )
    # projection pushdown fused with the pushed filters: each base table
    # keeps only the columns referenced downstream, and a pushed filter
    # runs as select(keep, where=...) so the compaction never gathers
    # columns (strings especially) that the filter output drops
    if stmt.joins:
        frames2: List[DataFrame] = [res] + [
            join_inputs[i]
            if i < len(join_inputs)
            else _resolve_from(stmt.joins[i].item, tables, engine)
            for i in range(len(stmt.joins))
        ]
        needed = _needed_columns(stmt, residual_where)
        pruned: List[DataFrame] = []
        for idx, fr in enumerate(frames2):
            conjs = pushed.get(idx, [])
            where_ce = None
            for conj in conjs:
                ce = _to_column_expr(conj, fr.schema, {})
                where_ce = ce if where_ce is None else (where_ce & ce)
            if needed is not None:
                keep = [n for n in fr.schema.names if n in needed]
            else:
                keep = list(fr.schema.names)
            if len(keep) == 0:
                keep = [fr.schema.names[0]]
            if where_ce is not None:
                fr = engine.select(
                    fr,
                    SelectColumns(*[col(n) for n in keep]),
                    where=where_ce,
                )
            elif len(keep) < len(fr.schema.names):
                fr = engine.select(
                    fr, SelectColumns(*[col(n) for n in keep])
                )
            pruned.append(fr)
        frames2 = pruned
        res = frames2[0]
        join_inputs = frames2[1:]
    for ji, j in enumerate(stmt.joins):
        right = (
            join_inputs[ji]
            if ji < len(join_inputs)
            else _resolve_from(j.item, tables, engine)
        )
        how = _JOIN_MAP.get(j.how)
        if how is None:
            raise UnsupportedPlan(f"join {j.how}")
        if j.using is not None:
            keys = list(j.using)
        elif j.on is not None:
            pairs = _extract_on_names(j.on)
            keys = []
            for a, b in pairs:
                if a in res.schema and b in right.schema:
                    if a != b:
                        raise UnsupportedPlan(
                            "join keys with different names need rename"
                        )
                    keys.append(a)
                elif b in res.schema and a in right.schema:
                    if a != b:
                        raise UnsupportedPlan(
                            "join keys with different names need rename"
                        )
                    keys.append(a)
                else:
                    raise UnsupportedPlan("can't resolve join key sides")
        elif how == "cross":
            keys = []
        else:
            raise UnsupportedPlan("JOIN without ON/USING")
        common = [n for n in res.schema.names if n in right.schema]
        if how != "cross" and set(keys) != set(common):
            raise UnsupportedPlan(
                f"join keys {keys} != common columns {common} "
                "(fugue joins use all common columns)"
            )
        if (
            ji == len(stmt.joins) - 1
            and how == "inner"
            and _plain_join_consumer(stmt, residual_where)
        ):
            # the last join runs with its consumer when the engine offers it
            fused = _join_with_consumer(
                stmt, residual_where, res, right, keys, engine
            )
            if fused is not None:
                return fused
        res = engine.join(res, right, how=how, on=keys if keys else None)
    # select columns
    schema = res.schema
    where_expr: Optional[ColumnExpr] = None
    if residual_where is not None:
        where_expr = _to_column_expr(residual_where, schema, {})
    cols: List[ColumnExpr] = []
    from fugue_amd.column.expressions import all_cols

    frame_windows = _find_frame_windows(stmt, schema)
    partition_windows = None
    if frame_windows is None:
        partition_windows = _find_partition_windows(stmt, schema)
    value_windows = None
    if frame_windows is None and partition_windows is None:
        value_windows = _find_value_windows(stmt, schema)
    value_items: Dict[int, Tuple] = {}
    window = None
    if frame_windows is not None:
        # WHERE filters the rows the windows see, so it runs first
        if where_expr is not None:
            res = engine.select(
                res, SelectColumns(all_cols()), where=where_expr
            )
            where_expr = None
        pcols, ocols, value_items = frame_windows
        res = engine.frame_over(
            res, pcols, ocols, [value_items[i] for i in sorted(value_items)]
        )
    elif partition_windows is not None:
        # WHERE filters the rows the windows see, so it runs first
        if where_expr is not None:
            res = engine.select(
                res, SelectColumns(all_cols()), where=where_expr
            )
            where_expr = None
        pcols, ocols, value_items = partition_windows
        res = engine.partition_over(
            res, pcols, ocols, [value_items[i] for i in sorted(value_items)]
        )
    elif value_windows is not None:
        # WHERE filters the rows the windows see, so it runs first
        if where_expr is not None:
            res = engine.select(
                res, SelectColumns(all_cols()), where=where_expr
            )
            where_expr = None
        pcols, ocols, value_items = value_windows
        res = engine.window_over(
            res, pcols, ocols, [value_items[i] for i in sorted(value_items)]
        )
        window = None
    else:
        window = _find_ranking_window(stmt, schema)
    if window is not None:
        # WHERE filters the rows the window sees, so it runs first
        if where_expr is not None:
            res = engine.select(
                res, SelectColumns(all_cols()), where=where_expr
            )
            where_expr = None
        win_idx, kind, pcols, ocols = window
        res = engine.rank_over(res, pcols, ocols, kind, _WINDOW_TMP)
    for i, (e, alias) in enumerate(stmt.columns):
        if isinstance(e, X.Star):
            if e.qualifier is not None:
                raise UnsupportedPlan("qualified * in select")
            if window is not None or value_items:
                # the pre-window columns only: the window columns are
                # projected under their own names below
                cols.extend(col(n) for n in schema.names)
            else:
                cols.append(all_cols())
            continue
        if window is not None and i == window[0]:
            cols.append(col(_WINDOW_TMP).alias(alias or e.default_name()))
            continue
        if i in value_items:
            cols.append(
                col(value_items[i][0]).alias(alias or e.default_name())
            )
            continue
        ce = _to_column_expr(e, schema, {})
        name = alias or e.default_name() or f"_col{i}"
        if isinstance(e, X.ColRef) and alias is None:
            cols.append(ce)
        else:
            cols.append(ce.alias(name))
    having_expr: Optional[ColumnExpr] = None
    sc = SelectColumns(*cols, arg_distinct=stmt.distinct)
    # GROUP BY validation: keys must match the non-agg select columns
    if stmt.group_by:
        if not sc.has_agg:
            raise UnsupportedPlan("GROUP BY without aggregates")
        group_names = set()
        for g in stmt.group_by:
            if isinstance(g, X.ColRef):
                group_names.add(g.name)
            elif isinstance(g, X.Lit) and isinstance(g.value, int):
                e0 = stmt.columns[g.value - 1][0]
                if isinstance(e0, X.ColRef):
                    group_names.add(e0.name)
                else:
                    raise UnsupportedPlan("positional GROUP BY on expression")
            else:
                raise UnsupportedPlan("GROUP BY expression")
        sel_keys = {k.output_name or k.name for k in sc.group_keys}
        if group_names != sel_keys:
            raise UnsupportedPlan(
                f"GROUP BY {group_names} != selected keys {sel_keys}"
            )
    if stmt.having is not None:
        # having references output aggregate aliases
        out_schema_names = [c.output_name for c in sc.all_cols]
        having_expr = _to_column_expr(
            stmt.having, Schema([(n, "double") for n in out_schema_names if n]), {}
        )
    return engine.select(res, sc, where=where_expr, having=having_expr)
