"""Plain-Python references of the engine's joins and set operations, and
the case builders that ``test_join_setop_refs.py`` (reference against the
native engine), ``test_join_engine.py`` (device engine on CPU tensors) and
``test_join_engine_gpu.py`` (device engine on the GPU) share.

The references work on rows of Python objects with ``None`` for null; they
use neither torch nor a pandas merge.  Keys are equal by VALUE:

* null never matches in a join;
* ``0.0 == -0.0``;
* an int and a float compare exactly (both become ``fractions.Fraction``);
* ``+inf`` and ``-inf`` equal themselves;
* NaN is null.  A pandas frame cannot tell the two apart, so in this
  project a NaN key behaves as a null key in joins, and NaN and null are
  one class in set operations.  The oracle is "what the native engine
  answers on the equivalent pandas frame", and ``test_join_setop_refs.py``
  holds the references to exactly that.

Output cells are compared exactly.  ``cell`` turns a float into its 8-byte
pattern so that ``-0.0`` and ``0.0`` stay apart (a join's key column must
carry the left frame's own zero), and NaN into ``None``.

Set operations return a ``Counter`` of value classes, not of bit patterns:
which member of a class (``0.0`` or ``-0.0``, NaN or null) represents it in
the output is not defined — pandas keeps the first row, the device keeps
whichever row won the table slot.  ``check_members`` adds what can be said
about bits: every output row is, bit for bit, a row of an input.
"""
import datetime
import math
import struct
from collections import Counter
from fractions import Fraction
from functools import lru_cache
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import pyarrow as pa
import torch

from fugue_amd.dataframe.arrow_dataframe import ArrowDataFrame
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame, StringDeviceColumn
from fugue_amd.schema import Schema

Row = Tuple[Any, ...]
HOWS = ["inner", "left_outer", "right_outer", "full_outer", "semi", "anti"]


# ---------------------------------------------------------------------- #
# value classes and exact cells                                            #
# ---------------------------------------------------------------------- #
def key_class(v: Any) -> Any:
    """What two key values must share to be equal; ``None`` for null."""
    if v is None:
        return None
    if isinstance(v, bool):
        return ("bool", v)
    if isinstance(v, float):
        if math.isnan(v):
            return None
        if math.isinf(v):
            return ("inf", v > 0)
        return Fraction(v)
    if isinstance(v, int):
        return Fraction(v)
    return v


def cell(v: Any) -> Any:
    """One output cell, comparable exactly (floats by bit pattern)."""
    if v is None:
        return None
    if isinstance(v, float):
        if math.isnan(v):
            return None
        return ("f", struct.pack(">d", v))
    return v


def cells(row: Sequence[Any]) -> Row:
    return tuple(cell(v) for v in row)


def row_class(row: Sequence[Any]) -> Row:
    return tuple(key_class(v) for v in row)


# ---------------------------------------------------------------------- #
# joins                                                                    #
# ---------------------------------------------------------------------- #
def join_ref(
    left_rows: Sequence[Row],
    right_rows: Sequence[Row],
    key_idx: Sequence[Tuple[int, int]],
    how: str,
    key_cast: Optional[Sequence[Optional[Callable[[Any], Any]]]] = None,
    n_left: Optional[int] = None,
    n_right: Optional[int] = None,
) -> "Counter[Row]":
    """The multiset of output rows (as ``cells``) of ``left JOIN right``.

    ``key_idx`` holds, per key column, its position in a left row and in a
    right row.  Columns come out in ``get_join_schemas`` order: the left
    row, then the right row without its key columns; semi and anti joins
    give the left row alone.  Key cells come from the left row; a right
    row without a partner (right and full outer) fills them from its own
    keys, through ``key_cast`` where the left column's type differs.
    ``n_left`` / ``n_right`` give a side's column count where it has no
    row to tell it (null padding of the other side's partnerless rows)."""
    assert how in HOWS, how
    lk = [i for i, _ in key_idx]
    rk = [j for _, j in key_idx]
    if n_left is None:
        n_left = len(left_rows[0])
    if n_right is None:
        n_right = len(right_rows[0])
    n_rest = n_right - len(rk)

    def _key(row: Row, idx: List[int]) -> Optional[Row]:
        k = tuple(key_class(row[i]) for i in idx)
        return None if any(x is None for x in k) else k

    def _rest(r: Row) -> Row:
        return tuple(v for j, v in enumerate(r) if j not in rk)

    build: Dict[Row, List[Row]] = {}
    for r in right_rows:
        k = _key(r, rk)
        if k is not None:
            build.setdefault(k, []).append(r)

    out: "Counter[Row]" = Counter()
    matched = set()
    for l in left_rows:
        k = _key(l, lk)
        partners = build.get(k, []) if k is not None else []
        if how in ("semi", "anti"):
            if bool(partners) == (how == "semi"):
                out[cells(l)] += 1
        elif partners:
            matched.add(k)
            for r in partners:
                out[cells(tuple(l) + _rest(r))] += 1
        elif how in ("left_outer", "full_outer"):
            out[cells(tuple(l) + (None,) * n_rest)] += 1
    if how in ("right_outer", "full_outer"):
        for r in right_rows:
            k = _key(r, rk)
            if k is not None and k in matched:
                continue
            left: List[Any] = [None] * n_left
            for n, (i, j) in enumerate(key_idx):
                v = r[j]
                if v is not None and key_cast is not None and key_cast[n] is not None:
                    v = key_cast[n](v)
                left[i] = v
            out[cells(tuple(left) + _rest(r))] += 1
    return out


# ---------------------------------------------------------------------- #
# set operations (value classes; see the module docstring)                 #
# ---------------------------------------------------------------------- #
def distinct_ref(rows: Sequence[Row]) -> "Counter[Row]":
    return Counter({row_class(r): 1 for r in rows})


def union_ref(
    a: Sequence[Row], b: Sequence[Row], distinct: bool = True
) -> "Counter[Row]":
    if distinct:
        return distinct_ref(list(a) + list(b))
    return Counter(row_class(r) for r in list(a) + list(b))


def subtract_ref(
    a: Sequence[Row], b: Sequence[Row], distinct: bool = True
) -> "Counter[Row]":
    """Rows of ``a`` whose class is not in ``b``.  The ALL form keeps every
    such row of ``a`` (the engines' EXCEPT ALL is an anti join, it does not
    subtract counts)."""
    gone = {row_class(r) for r in b}
    kept = [r for r in a if row_class(r) not in gone]
    return distinct_ref(kept) if distinct else Counter(row_class(r) for r in kept)


def intersect_ref(
    a: Sequence[Row], b: Sequence[Row], distinct: bool = True
) -> "Counter[Row]":
    """Rows of ``a`` whose class is in ``b``; the ALL form keeps every such
    row of ``a`` (a semi join)."""
    there = {row_class(r) for r in b}
    kept = [r for r in a if row_class(r) in there]
    return distinct_ref(kept) if distinct else Counter(row_class(r) for r in kept)


def class_counter(rows: Sequence[Row]) -> "Counter[Row]":
    return Counter(row_class(r) for r in rows)


def check_members(out_rows: Sequence[Row], *inputs: Sequence[Row]) -> None:
    """Every output row is bit for bit a row of some input (a set operation
    gathers rows, it computes none)."""
    have = set()
    for rows in inputs:
        have.update(cells(r) for r in rows)
    for r in out_rows:
        assert cells(r) in have, f"row {r!r} is in no input"


# ---------------------------------------------------------------------- #
# frames: one description, three forms                                     #
# ---------------------------------------------------------------------- #
_EPOCH_D = datetime.date(1970, 1, 1)
_EPOCH_T = datetime.datetime(1970, 1, 1)

_TORCH = {
    "bool": torch.bool,
    "byte": torch.int8,
    "short": torch.int16,
    "int": torch.int32,
    "long": torch.int64,
    "float": torch.float32,
    "double": torch.float64,
    "date": torch.int64,
    "datetime": torch.int64,
}
_NP = {
    "bool": np.bool_,
    "byte": np.int8,
    "short": np.int16,
    "int": np.int32,
    "long": np.int64,
    "float": np.float32,
    "double": np.float64,
    "date": np.int64,
    "datetime": np.int64,
}


def _garbage(tp: str) -> Any:
    """What lies under a null slot: the type's minimum, NaN for floats —
    a value that a reduction over the raw data would trip on."""
    if tp == "bool":
        return False
    if tp in ("float", "double"):
        return float("nan")
    return int(np.iinfo(_NP[tp]).min)


def _stored(tp: str, v: Any) -> Any:
    if tp == "date":
        return (v - _EPOCH_D).days
    if tp == "datetime":
        return (v - _EPOCH_T) // datetime.timedelta(microseconds=1)
    return v


class Col:
    """One column: a name, a fugue type name and Python values (``None`` is
    null; a float NaN is a NaN the mask does not cover)."""

    def __init__(self, name: str, tp: str, values: Sequence[Any]):
        self.name, self.tp, self.values = name, tp, list(values)

    @property
    def masked(self) -> bool:
        return any(v is None for v in self.values)

    def device_column(self, device: str) -> DeviceColumn:
        n = len(self.values)
        valid = None
        if self.masked:
            valid = torch.tensor(
                [v is not None for v in self.values], dtype=torch.bool
            ).to(device)
        if self.tp == "str":
            chunks = [
                (b"~null-slot~" if v is None else v.encode("utf-8"))
                for v in self.values
            ]
            offs = np.zeros(n + 1, dtype=np.int64)
            if n > 0:
                offs[1:] = np.cumsum([len(c) for c in chunks])
            raw = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
            return StringDeviceColumn(
                torch.from_numpy(offs).to(device),
                torch.from_numpy(raw).to(device),
                valid,
            )
        g = _garbage(self.tp)
        arr = np.array(
            [g if v is None else _stored(self.tp, v) for v in self.values],
            dtype=_NP[self.tp],
        )
        pa_type = Schema(f"x:{self.tp}").fields[0].type
        return DeviceColumn(torch.from_numpy(arr).to(device), valid, pa_type)

    def arrow(self) -> pa.Array:
        pa_type = Schema(f"x:{self.tp}").fields[0].type
        vals = [
            None if (isinstance(v, float) and math.isnan(v)) else v
            for v in self.values
        ]
        return pa.array(vals, type=pa_type)


class Frame:
    def __init__(self, cols: Sequence[Col]):
        self.cols = list(cols)
        n = {len(c.values) for c in self.cols}
        assert len(n) == 1, n

    @property
    def schema(self) -> Schema:
        return Schema(",".join(f"{c.name}:{c.tp}" for c in self.cols))

    @property
    def names(self) -> List[str]:
        return [c.name for c in self.cols]

    def rows(self) -> List[Row]:
        return list(zip(*[c.values for c in self.cols]))

    def hip(self, device: str) -> HipDataFrame:
        """Built column by column, so that garbage under null slots and a
        NaN outside any mask reach the engine as they are."""
        return HipDataFrame.from_columns(
            {c.name: c.device_column(device) for c in self.cols},
            self.schema,
            device,
        )

    def native(self) -> ArrowDataFrame:
        """The equivalent host frame (NaN and null are both null there)."""
        sch = self.schema
        return ArrowDataFrame(
            pa.Table.from_arrays(
                [c.arrow() for c in self.cols], schema=sch.pa_schema
            )
        )


def frame_rows(df: Any) -> List[Row]:
    """Rows of any engine's result as Python objects."""
    return [tuple(r) for r in df.as_array(type_safe=True)]


# ---------------------------------------------------------------------- #
# key domains                                                              #
# ---------------------------------------------------------------------- #
def _f32(v: float) -> float:
    return float(np.float32(v))


FLOAT64_EDGES = [
    0.0, -0.0, float("inf"), float("-inf"),
    1.0, 1.25, 1.5, 1.75,
    2.0 ** 53, 2.0 ** 53 + 2,
    1e300, -1e300, 2e300, -2e300,
    5e-324,  # the smallest subnormal
    float("nan"),
]
FLOAT32_EDGES = [
    0.0, -0.0, float("inf"), float("-inf"),
    1.0, 1.25, 1.5, 1.75,
    2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 53,
    _f32(3e38), _f32(-3e38), _f32(1.5e38), _f32(-1.5e38),
    _f32(1e-45),  # the smallest float32 subnormal
    _f32(0.1), _f32(0.3),
    float("nan"),
]


def _int_edges(tp: str, host_exact: bool = False) -> List[int]:
    ii = np.iinfo(_NP[tp])
    lo, hi = int(ii.min), int(ii.max)
    if host_exact and tp == "long":
        lo, hi = -(2 ** 53), 2 ** 53
    return [lo, hi, -1, 0, 1, lo + 1, hi - 1]


def domain(
    tp: str, k: int, rng: np.random.Generator, host_exact: bool = False
) -> List[Any]:
    """Up to ``k`` key values of one type, distinct as Python objects, the
    type's edge values first.  ``host_exact``: for an int64 column that
    will carry nulls.  A host (pandas) frame holds such a column as
    float64, so beyond 2**53 the native oracle has no exact answer; the
    extremes are then +-2**53, and the type's own minimum and maximum are
    left to the mask-free cases."""
    if tp == "bool":
        return [False, True]
    if tp in ("byte", "short", "int", "long"):
        ii = np.iinfo(_NP[tp])
        out = _int_edges(tp, host_exact)
        # a narrow band, so that random draws of two sides meet
        lo, hi = max(int(ii.min), -4 * k), min(int(ii.max), 4 * k)
        pool = [int(x) for x in rng.permutation(np.arange(lo, hi + 1))]
    elif tp in ("float", "double"):
        out = list(FLOAT32_EDGES if tp == "float" else FLOAT64_EDGES)
        # quarters: groups that share an integer part
        pool = [float(x) / 4.0 for x in rng.permutation(np.arange(-4 * k, 4 * k))]
    elif tp == "date":
        out = [
            datetime.date(1700, 1, 1), datetime.date(2200, 12, 31),
            datetime.date(1969, 12, 31), _EPOCH_D, datetime.date(1970, 1, 2),
        ]
        pool = [
            _EPOCH_D + datetime.timedelta(days=int(x))
            for x in rng.permutation(np.arange(-4 * k, 4 * k))
        ]
    elif tp == "datetime":
        out = [
            datetime.datetime(1700, 1, 1), datetime.datetime(2200, 12, 31, 23, 59, 59, 999999),
            datetime.datetime(1969, 12, 31, 23, 59, 59, 999999), _EPOCH_T,
            datetime.datetime(1970, 1, 1, 0, 0, 0, 1),
        ]
        pool = [
            _EPOCH_T + datetime.timedelta(microseconds=int(x) * 999_983)
            for x in rng.permutation(np.arange(-4 * k, 4 * k))
        ]
    elif tp == "str":
        out = ["", " ", "a", "A", "ab", "ba", "é", "日本", "a" * 40, "null", "nan"]
        pool = [f"k{int(x):05d}" for x in rng.permutation(8 * k)]
    else:
        raise ValueError(tp)
    seen = {_ident(v) for v in out}
    for v in pool:
        if len(out) >= k:
            break
        if _ident(v) not in seen:
            seen.add(_ident(v))
            out.append(v)
    return out


def _ident(v: Any) -> Any:
    return cell(v) if isinstance(v, float) else v


def draw(
    values: Sequence[Any], n: int, rng: np.random.Generator, unique: bool = False
) -> List[Any]:
    """``n`` key values: every value of ``values`` once (as far as ``n``
    allows), then random repeats, shuffled.  ``unique``: no two rows share
    a key class (NaN may repeat: it matches nothing)."""
    values = list(values)
    if unique:
        seen, uniq = set(), []
        for v in values:
            c = key_class(v)
            if c is None or c not in seen:
                seen.add(c)
                uniq.append(v)
        assert len(uniq) >= n, (len(uniq), n)
        out = uniq[:n]
    else:
        out = values[:n]
        if n > len(out):
            extra = rng.integers(0, len(values), n - len(out))
            out = out + [values[int(i)] for i in extra]
    order = rng.permutation(len(out))
    return [out[int(i)] for i in order]


def with_nulls(vals: List[Any], frac: float, rng: np.random.Generator) -> List[Any]:
    if frac >= 1.0:
        return [None] * len(vals)
    hit = rng.random(len(vals)) < frac
    if len(vals) > 0:
        hit[0] = True
    return [None if h else v for v, h in zip(vals, hit)]


# ---------------------------------------------------------------------- #
# join cases                                                               #
# ---------------------------------------------------------------------- #
class JoinCase:
    """Two frames that share their key column names.  The left frame adds
    ``lv:long`` (the row number) and the right ``rv:double`` (half the row
    number, null on every seventh row when ``null_payload``)."""

    def __init__(
        self,
        name: str,
        left_keys: Sequence[Col],
        right_keys: Sequence[Col],
        hows: Sequence[str] = tuple(HOWS),
        key_cast: Optional[Sequence[Optional[Callable[[Any], Any]]]] = None,
        null_payload: bool = True,
        left_payload: bool = True,
        native_oracle: bool = True,
    ):
        """``left_payload=False``: the left frame is its key columns alone.
        ``native_oracle=False``: the native engine has no exact answer
        (see ``domain``); the plain-Python reference is the only oracle."""
        self.name = name
        self.native_oracle = native_oracle
        self.keys = [c.name for c in left_keys]
        nl, nr = len(left_keys[0].values), len(right_keys[0].values)
        self.left = Frame(
            list(left_keys)
            + ([Col("lv", "long", list(range(nl)))] if left_payload else [])
        )
        rv = [
            None if (null_payload and i % 7 == 3) else i * 0.5 for i in range(nr)
        ]
        self.right = Frame([Col("rv", "double", rv)] + list(right_keys))
        self.hows = list(hows)
        self.key_cast = key_cast
        self._expected: Dict[str, "Counter[Row]"] = {}

    @property
    def route(self) -> Optional[str]:
        """The key route the engine must take, where the key types fix
        it: ``"exact"`` (an int64 key: one integer or float column) or
        ``"hashed"`` (128-bit row hashes: a string or float column in a
        wider key, an integer tuple wider than 63 bits).  ``None`` where
        the packed width depends on the drawn values or the host joins."""
        if self.name in MIXED_CASES[2:]:
            return None
        tps = [c.tp for c in self.left.cols if c.name in self.keys]
        if "str" in tps or (len(tps) > 1 and ("float" in tps or "double" in tps)):
            return "hashed"
        if self.name.startswith("two-long-wide"):
            return "hashed"
        if len(tps) == 1 and tps[0] in ("float", "double"):
            return "exact"
        if len(tps) == 1 and tps[0] not in ("long",):
            # narrow ints, bool and the temporal ranges used here (under
            # 2**55 microseconds) pack into 63 bits with their null code
            return "exact"
        return None

    @property
    def key_idx(self) -> List[Tuple[int, int]]:
        return [
            (self.left.names.index(k), self.right.names.index(k))
            for k in self.keys
        ]

    def expected(self, how: str) -> "Counter[Row]":
        """Computed once per join type and shared by every test."""
        if how not in self._expected:
            self._expected[how] = join_ref(
                self.left.rows(), self.right.rows(), self.key_idx, how,
                self.key_cast, len(self.left.cols), len(self.right.cols),
            )
        return self._expected[how]


KEY_TYPES = [
    "bool", "byte", "short", "int", "long", "float", "double", "date",
    "datetime", "str",
]
NULL_MODES = ["none", "left", "both", "allnull"]
EDGE_ROWS = 257
_ALL_BUT_RIGHT_OUTER = [h for h in HOWS if h not in ("right_outer", "full_outer")]

# the mixed-type cases: the only ones allowed to take the host join
MIXED_CASES = [
    "mixed-int-long", "mixed-long-int",
    "mixed-long-double", "mixed-double-long",
    "mixed-float-double", "mixed-double-float",
]


def _sides(
    tp: str, nl: int, nr: int, seed: int, unique_build: bool = False,
    dom: Optional[int] = None, host_exact: bool = False,
) -> Tuple[List[Any], List[Any]]:
    """Key values of two sides over one domain; a tenth of the domain is
    kept from each side, so both have partnerless rows."""
    rng = np.random.default_rng(seed)
    k = dom if dom is not None else max(nl, nr, 8)
    d = domain(tp, k, rng, host_exact)
    if len(d) > 8:
        cut = max(1, len(d) // 10)
        tail = d[-2 * cut :]
        head = d[: -2 * cut]
        dl, dr = head + tail[:cut], head + tail[cut:]
    else:
        dl, dr = d, d
    if unique_build:
        # every class at most once on the build side: the right share of
        # the domain first, topped up with values the left never has
        pool = dr if tp == "bool" else dr + domain(tp, 2 * nr + 40, rng)
        right = draw(pool, nr, rng, unique=True)
    else:
        right = draw(dr, nr, rng)
    return draw(dl, nl, rng), right


def _nulls(
    mode: str, left: List[Any], right: List[Any], seed: int
) -> Tuple[List[Any], List[Any]]:
    rng = np.random.default_rng(seed + 9)
    if mode == "left":
        return with_nulls(left, 0.2, rng), right
    if mode == "both":
        return with_nulls(left, 0.2, rng), with_nulls(right, 0.2, rng)
    if mode == "allnull":
        return with_nulls(left, 0.2, rng), with_nulls(right, 1.0, rng)
    return left, right


def _single(name: str, tp: str, left: List[Any], right: List[Any], **kw: Any) -> JoinCase:
    return JoinCase(name, [Col("k", tp, left)], [Col("k", tp, right)], **kw)


def _build_join_cases() -> Dict[str, JoinCase]:
    cases: List[JoinCase] = []
    seed = 1000
    # edge values of every key type under every null layout
    for tp in KEY_TYPES:
        for mode in NULL_MODES:
            seed += 1
            l, r = _sides(
                tp, EDGE_ROWS, EDGE_ROWS, seed, dom=64, host_exact=mode != "none"
            )
            l, r = _nulls(mode, l, r, seed)
            cases.append(_single(f"edge-{tp}-{mode}", tp, l, r))
    # more than one block of every join kernel: unique and duplicated build
    for tp in KEY_TYPES:
        seed += 1
        if tp in ("bool", "byte"):
            # too few values for a unique build of this size
            l, r = _sides(tp, 2049, 2, seed, unique_build=True)
        else:
            l, r = _sides(tp, 2049, 2049, seed, unique_build=True)
        cases.append(_single(f"unique-{tp}-2049", tp, l, r))
        seed += 1
        # about two partners per probe row; the narrow types have few
        # values, so their right side stays small instead
        nr = 5000 if tp not in ("bool", "byte") else (3 if tp == "bool" else 300)
        l, r = _sides(tp, 5000, nr, seed, dom=2500)
        cases.append(_single(f"dup-{tp}-5000", tp, l, r))
    # the other row counts, on the three key routes
    for tp in ("long", "double", "str"):
        for n in (1, 255):
            seed += 1
            l, r = _sides(tp, n, n, seed)
            cases.append(_single(f"rows-{tp}-{n}", tp, l, r))
        seed += 1
        l, r = _sides(tp, 50, 257, seed, unique_build=True)
        cases.append(_single(f"swap-{tp}-50x257", tp, l, r))
        seed += 1
        l, r = _sides(tp, 40, 2049, seed, dom=500)
        cases.append(_single(f"swap-dup-{tp}-40x2049", tp, l, r))
        seed += 1
        l, r = _sides(tp, 33, 33, seed)
        cases.append(_single(f"empty-left-{tp}", tp, [], r))
        cases.append(_single(f"empty-right-{tp}", tp, l, []))
        cases.append(_single(f"empty-both-{tp}", tp, [], []))
    # key count
    for mode in ("none", "both"):
        seed += 1
        a1, a2 = _sides("int", EDGE_ROWS, EDGE_ROWS, seed, dom=12)
        b1, b2 = _sides("double", EDGE_ROWS, EDGE_ROWS, seed + 50, dom=24)
        a1, a2 = _nulls(mode, a1, a2, seed)
        b1, b2 = _nulls(mode, b1, b2, seed + 50)
        cases.append(JoinCase(
            f"two-int-double-{mode}",
            [Col("a", "int", a1), Col("b", "double", b1)],
            [Col("a", "int", a2), Col("b", "double", b2)],
        ))
        seed += 1
        a1, a2 = _sides(
            "long", EDGE_ROWS, EDGE_ROWS, seed, dom=12, host_exact=mode != "none"
        )
        b1, b2 = _sides(
            "long", EDGE_ROWS, EDGE_ROWS, seed + 50, dom=12, host_exact=mode != "none"
        )
        a1, a2 = _nulls(mode, a1, a2, seed)
        b1, b2 = _nulls(mode, b1, b2, seed + 50)
        cases.append(JoinCase(
            f"two-long-wide-{mode}",
            [Col("a", "long", a1), Col("b", "long", b1)],
            [Col("b", "long", b2), Col("a", "long", a2)],
        ))
        seed += 1
        a1, a2 = _sides("str", EDGE_ROWS, EDGE_ROWS, seed, dom=10)
        b1, b2 = _sides("short", EDGE_ROWS, EDGE_ROWS, seed + 50, dom=8)
        c1, c2 = _sides("float", EDGE_ROWS, EDGE_ROWS, seed + 90, dom=20)
        a1, a2 = _nulls(mode, a1, a2, seed)
        c1, c2 = _nulls(mode, c1, c2, seed + 90)
        cases.append(JoinCase(
            f"three-str-short-float-{mode}",
            [Col("a", "str", a1), Col("b", "short", b1), Col("c", "float", c1)],
            [Col("a", "str", a2), Col("b", "short", b2), Col("c", "float", c2)],
        ))
    seed += 1
    a1, a2 = _sides("long", 2049, 2049, seed, dom=60)
    b1, b2 = _sides("long", 2049, 2049, seed + 50, dom=60)
    cases.append(JoinCase(
        "two-long-wide-2049",
        [Col("a", "long", a1), Col("b", "long", b1)],
        [Col("a", "long", a2), Col("b", "long", b2)],
    ))
    # mixed sides.  Values are such that the exact answer exists in the
    # left column's type: ints within int32, and |int| <= 2**53 against a
    # double.  A right or full outer join puts the key of a partnerless
    # right row into the LEFT column's type; 1.5 has no int64 form, so
    # those two join types run only where the left type holds every right
    # key (the narrower or integer type on the right).
    seed += 1
    rng = np.random.default_rng(seed)
    small = [-1, 0, 1, 2, 3, 2 ** 31 - 1, -(2 ** 31)] + [
        int(x) for x in rng.integers(-40, 40, 60)
    ]
    il = draw(small, EDGE_ROWS, rng)
    ir = draw(small[:40] + [77, 78], EDGE_ROWS, rng)
    cases.append(JoinCase(
        "mixed-int-long", [Col("k", "int", il)], [Col("k", "long", ir)],
    ))
    cases.append(JoinCase(
        "mixed-long-int", [Col("k", "long", ir)], [Col("k", "int", il)],
    ))
    ints = [1, 2, 3, 0, -1, 2 ** 53, -(2 ** 53), 7, 8] + [
        int(x) for x in rng.integers(-30, 30, 40)
    ]
    dbls = [1.5, 2.0, 2.5, 0.0, -0.0, -1.0, 2.0 ** 53, 7.25, 8.0,
            float("inf"), float("-inf"), float("nan")] + [
        float(x) / 2.0 for x in rng.integers(-60, 60, 40)
    ]
    li = with_nulls(draw(ints, EDGE_ROWS, rng), 0.1, rng)
    rd = with_nulls(draw(dbls, EDGE_ROWS, rng), 0.1, rng)
    cases.append(JoinCase(
        "mixed-long-double", [Col("k", "long", li)], [Col("k", "double", rd)],
        hows=_ALL_BUT_RIGHT_OUTER,
    ))
    cases.append(JoinCase(
        "mixed-double-long", [Col("k", "double", rd)], [Col("k", "long", li)],
        key_cast=[float],
    ))
    f32 = [v for v in FLOAT32_EDGES] + [float(x) / 4.0 for x in rng.integers(-40, 40, 40)]
    f64 = [v for v in FLOAT64_EDGES] + [0.1, 0.3, _f32(0.1), _f32(0.3)] + [
        float(x) / 4.0 for x in rng.integers(-40, 40, 40)
    ]
    lf = draw(f32, EDGE_ROWS, rng)
    rf = draw(f64, EDGE_ROWS, rng)
    cases.append(JoinCase(
        "mixed-float-double", [Col("k", "float", lf)], [Col("k", "double", rf)],
        hows=_ALL_BUT_RIGHT_OUTER,
    ))
    cases.append(JoinCase(
        "mixed-double-float", [Col("k", "double", rf)], [Col("k", "float", lf)],
    ))
    # int64 extremes under a mask: garbage and real values at the type's
    # minimum both reach the engine's range reduction.  Reference only.
    for mode in ("left", "both"):
        seed += 1
        l, r = _sides("long", EDGE_ROWS, EDGE_ROWS, seed, dom=64)
        l, r = _nulls(mode, l, r, seed)
        cases.append(_single(
            f"edge-long-wide-{mode}", "long", l, r, native_oracle=False
        ))
    # a left frame of key columns alone: a right outer join still owes
    # the matched rows the left frame's own zero
    cases.append(_single(
        "keyonly-left-double", "double",
        [-0.0, 1.5, 2.0, 0.0, float("nan")], [0.0, 1.5, 3.0, 1.5],
        left_payload=False,
    ))
    # the issue's own smallest failing joins
    cases.append(_single(
        "issue-fraction-double", "double", [1.0, 1.5, 2.25], [1.5, 1.0, 2.75],
    ))
    cases.append(_single(
        "issue-quarters-double", "double", [0.25, 0.75], [0.5, 0.25],
    ))
    cases.append(_single(
        "issue-fraction-float", "float",
        [_f32(0.1), _f32(0.3)], [_f32(0.3), _f32(0.1), _f32(0.2)],
    ))
    cases.append(_single(
        "issue-huge-double", "double",
        [1e300, 2e300, 2.0 ** 63, 2.0 ** 64, -1e300],
        [2e300, 2.0 ** 64, -2e300, 2.0 ** 63 * 3],
    ))
    cases.append(_single(
        "issue-inf-nan-double", "double",
        [float("inf"), float("-inf"), float("nan"), 0.0],
        [float("-inf"), float("nan"), -0.0, float("inf"), float("inf")],
    ))
    out = {c.name: c for c in cases}
    assert len(out) == len(cases), "duplicate case name"
    return out


@lru_cache(maxsize=None)
def join_cases() -> Dict[str, JoinCase]:
    return _build_join_cases()


def join_case_names(native_only: bool = False) -> List[str]:
    return [
        n for n, c in join_cases().items() if c.native_oracle or not native_only
    ]


# ---------------------------------------------------------------------- #
# set-operation cases                                                      #
# ---------------------------------------------------------------------- #
class SetCase:
    def __init__(self, name: str, a: Frame, b: Frame):
        self.name, self.a, self.b = name, a, b


def _build_set_cases() -> Dict[str, SetCase]:
    cases: List[SetCase] = []
    nan = float("nan")
    cases.append(SetCase(
        "issue-zeros-nan",
        Frame([Col("x", "double", [0.0, -0.0, nan, nan, 1.0])]),
        Frame([Col("x", "double", [-0.0, 1.0])]),
    ))
    cases.append(SetCase(
        "nan-null-one-class",
        Frame([Col("x", "double", [nan, None, 1.0, None, 2.0, -0.0])]),
        Frame([Col("x", "double", [None, 2.0, 3.0])]),
    ))
    cases.append(SetCase(
        "nan-against-null",
        Frame([Col("x", "float", [nan, 1.0, 0.0])]),
        Frame([Col("x", "float", [None, -0.0])]),
    ))
    seed = 5000
    for tp in KEY_TYPES:
        for n in (EDGE_ROWS, 2049):
            if n == 2049 and tp not in ("long", "double", "float", "str"):
                continue
            seed += 1
            l, r = _sides(tp, n, n, seed, dom=max(64, n // 4), host_exact=True)
            l, r = _nulls("both", l, r, seed)
            cases.append(SetCase(
                f"one-{tp}-{n}", Frame([Col("x", tp, l)]), Frame([Col("x", tp, r)])
            ))
    for n in (EDGE_ROWS, 5000):
        seed += 1
        a1, a2 = _sides("double", n, n, seed, dom=24)
        b1, b2 = _sides("int", n, n, seed + 50, dom=max(10, n // 60))
        a1, a2 = _nulls("both", a1, a2, seed)
        cases.append(SetCase(
            f"two-double-int-{n}",
            Frame([Col("x", "double", a1), Col("y", "int", b1)]),
            Frame([Col("x", "double", a2), Col("y", "int", b2)]),
        ))
    seed += 1
    a1, a2 = _sides("float", EDGE_ROWS, EDGE_ROWS, seed, dom=22)
    b1, b2 = _sides("str", EDGE_ROWS, EDGE_ROWS, seed + 50, dom=6)
    c1, c2 = _sides("bool", EDGE_ROWS, EDGE_ROWS, seed + 90)
    a1, a2 = _nulls("both", a1, a2, seed)
    b1, b2 = _nulls("both", b1, b2, seed + 50)
    cases.append(SetCase(
        "three-float-str-bool",
        Frame([Col("x", "float", a1), Col("y", "str", b1), Col("z", "bool", c1)]),
        Frame([Col("x", "float", a2), Col("y", "str", b2), Col("z", "bool", c2)]),
    ))
    seed += 1
    l, r = _sides("double", 33, 33, seed)
    cases.append(SetCase(
        "empty-a", Frame([Col("x", "double", [])]), Frame([Col("x", "double", r)])
    ))
    cases.append(SetCase(
        "empty-b", Frame([Col("x", "double", l)]), Frame([Col("x", "double", [])])
    ))
    out = {c.name: c for c in cases}
    assert len(out) == len(cases), "duplicate case name"
    return out


@lru_cache(maxsize=None)
def set_cases() -> Dict[str, SetCase]:
    return _build_set_cases()


def set_case_names() -> List[str]:
    return list(set_cases().keys())


SET_OPS = [
    ("distinct", True), ("union", True), ("union", False),
    ("subtract", True), ("subtract", False),
    ("intersect", True), ("intersect", False),
]


def set_expected(case: SetCase, op: str, distinct: bool) -> "Counter[Row]":
    a, b = case.a.rows(), case.b.rows()
    if op == "distinct":
        return distinct_ref(a)
    if op == "union":
        return union_ref(a, b, distinct)
    if op == "subtract":
        return subtract_ref(a, b, distinct)
    return intersect_ref(a, b, distinct)


def run_set_op(engine: Any, op: str, distinct: bool, a: Any, b: Any) -> Any:
    if op == "distinct":
        return engine.distinct(a)
    return getattr(engine, op)(a, b, distinct=distinct)


# ---------------------------------------------------------------------- #
# checks shared by the CPU-tensor and the GPU module                       #
# ---------------------------------------------------------------------- #
class Spy:
    """Stands in for a host helper and counts its calls."""

    def __init__(self, fn: Callable[..., Any]):
        self.fn, self.calls = fn, 0

    def __call__(self, *args: Any, **kwargs: Any) -> Any:
        self.calls += 1
        return self.fn(*args, **kwargs)


def spy_on(monkeypatch: Any, *names: str) -> Dict[str, Spy]:
    """Replace helpers of ``fugue_amd.utils.pandas_like`` (the engine looks
    them up there at call time) by counting stand-ins."""
    import fugue_amd.utils.pandas_like as pl

    spies = {}
    for name in names:
        spies[name] = Spy(getattr(pl, name))
        monkeypatch.setattr(pl, name, spies[name])
    return spies


def check_join_case(
    engine: Any, device: str, case: JoinCase, monkeypatch: Any, on_host: bool
) -> None:
    """Every join type of one case: exact row multiset, output schema, and
    whether the host join ran (``on_host``) or must not have."""
    from fugue_amd.dataframe.utils import get_join_schemas

    import fugue_amd.hip.ops as dops

    spy = spy_on(monkeypatch, "pandas_join")["pandas_join"]
    hashes = Spy(dops.hash_rows)
    monkeypatch.setattr(dops, "hash_rows", hashes)
    left, right = case.left.hip(device), case.right.hip(device)
    for how in case.hows:
        before, hashed_before = spy.calls, hashes.calls
        res = engine.join(left, right, how=how, on=case.keys)
        _, want_schema = get_join_schemas(left, right, how=how, on=case.keys)
        assert res.schema == want_schema, (case.name, how)
        got = Counter(cells(r) for r in frame_rows(res))
        want = case.expected(how)
        if got != want:
            extra, missing = got - want, want - got
            raise AssertionError(
                f"{case.name} {how}: {sum(got.values())} rows for "
                f"{sum(want.values())}; unexpected "
                f"{list(extra.items())[:4]}, missing {list(missing.items())[:4]}"
            )
        if case.route is not None:
            assert not on_host
            hashed = hashes.calls > hashed_before
            assert hashed == (case.route == "hashed"), (
                f"{case.name} {how}: route {case.route}, row hashes "
                f"{'computed' if hashed else 'not computed'}"
            )
        ran_host = spy.calls > before
        assert ran_host == on_host, (
            f"{case.name} {how}: host join "
            f"{'ran' if ran_host else 'did not run'}"
        )


def check_set_case(
    engine: Any, device: str, case: SetCase, op: str, distinct: bool,
    monkeypatch: Any,
) -> None:
    """One set operation of one case: classes with their counts, every
    output row bitwise from an input, and the device path (INTERSECT ALL
    is on the host by design)."""
    spies = spy_on(
        monkeypatch, "pandas_except", "pandas_intersect", "drop_duplicates",
        "pandas_union",
    )
    a, b = case.a.hip(device), case.b.hip(device)
    res = run_set_op(engine, op, distinct, a, b)
    assert res.schema == case.a.schema
    rows = frame_rows(res)
    got, want = class_counter(rows), set_expected(case, op, distinct)
    if got != want:
        extra, missing = got - want, want - got
        raise AssertionError(
            f"{case.name} {op} distinct={distinct}: unexpected "
            f"{list(extra.items())[:4]}, missing {list(missing.items())[:4]}"
        )
    # a NaN outside a mask reads back as null: compare members that way
    def _seen(rows_: Sequence[Row]) -> List[Row]:
        return [tuple(None if cell(v) is None else v for v in r) for r in rows_]

    check_members(rows, _seen(case.a.rows()), _seen(case.b.rows()))
    host_calls = sum(s.calls for s in spies.values())
    if (op, distinct) == ("intersect", False):
        assert host_calls > 0
    else:
        assert host_calls == 0, f"{case.name} {op}: host path ran"


SQL_JOIN_SELECT = """
res = SELECT a.k, lv, rv FROM a INNER JOIN b ON a.k = b.k WHERE lv > rv
YIELD DATAFRAME AS result
"""


def sql_cases() -> Dict[str, JoinCase]:
    """The flagship's shape (inner join, one comparison, a projection)
    with a double key: a unique build with no NaN (the fused kernel's
    input), the same with NaN keys, and a duplicated build."""
    out = {}
    l, r = _sides("double", 2049, 2049, 77, unique_build=True)
    l0 = [v if not math.isnan(v) else 1.25 for v in l]
    r0 = [v for v in r if not math.isnan(v)]
    out["sql-double-unique"] = _single(
        "sql-double-unique", "double", l0, r0, null_payload=False
    )
    out["sql-double-unique-nan"] = _single(
        "sql-double-unique-nan", "double", l, r, null_payload=False
    )
    l, r = _sides("double", 5000, 5000, 78, dom=2500)
    out["sql-double-dup"] = _single(
        "sql-double-dup", "double", l, r, null_payload=False
    )
    return out


def sql_expected(case: JoinCase) -> "Counter[Row]":
    """``SELECT k, lv, rv ... WHERE lv > rv`` over the reference join
    (left row = (k, lv), right rest = (rv,))."""
    out: "Counter[Row]" = Counter()
    rows = join_ref(
        case.left.rows(), case.right.rows(), case.key_idx, "inner",
        None, len(case.left.cols), len(case.right.cols),
    )
    for (k, lv, rv), c in rows.items():
        rv_val = struct.unpack(">d", rv[1])[0]
        if lv > rv_val:
            out[(k, lv, rv)] += c
    return out


def check_sql_case(
    make_engine: Callable[[], Any], device: str, case: JoinCase, monkeypatch: Any
) -> Any:
    """The SQL against the reference, fused and with FUGUE_JOIN_FUSED=0;
    returns the first engine (its counters tell whether the fused kernel
    ran)."""
    import fugue_amd.api as fa

    def _run(engine: Any) -> "Counter[Row]":
        res = fa.fugue_sql(
            SQL_JOIN_SELECT, a=case.left.hip(device), b=case.right.hip(device),
            engine=engine, as_fugue=True,
        )
        assert res.schema == "k:double,lv:long,rv:double"
        return Counter(cells(r) for r in frame_rows(res))

    monkeypatch.delenv("FUGUE_JOIN_FUSED", raising=False)
    e1 = make_engine()
    fused = _run(e1)
    monkeypatch.setenv("FUGUE_JOIN_FUSED", "0")
    e0 = make_engine()
    plain = _run(e0)
    monkeypatch.delenv("FUGUE_JOIN_FUSED")
    assert e0.stats.get("join.fused_select") == 0
    want = sql_expected(case)
    assert sum(want.values()) > 0
    assert fused == want, case.name
    assert plain == want, case.name
    return e1
