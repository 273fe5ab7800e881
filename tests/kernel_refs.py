"""Plain numpy / Python-int references shared by the kernel tests
(``test_join_kernels_gpu.py``, ``test_select_kernels_gpu.py``,
``test_groupby_kernels_gpu.py``, ``test_hash_partition_kernels_gpu.py``)
and kept under test themselves by ``test_kernel_refs.py``.  Nothing here
touches the device, the extension or the engine's own evaluators."""
import math
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

INT64_MIN = -(2**63)
INT64_MAX = 2**63 - 1

# ------------------------------------------------------------------ #
# hashing                                                             #
# ------------------------------------------------------------------ #


def mix64(x: np.ndarray) -> np.ndarray:
    """splitmix64 finalizer over int64/uint64 values, as uint64."""
    x = np.ascontiguousarray(x).view(np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return x


def slot_of(keys: np.ndarray, tsize: int) -> np.ndarray:
    """Home slot of every key in a power-of-two table."""
    return (mix64(np.asarray(keys, dtype=np.int64)) & np.uint64(tsize - 1)).astype(
        np.int64
    )


# ------------------------------------------------------------------ #
# joins                                                               #
# ------------------------------------------------------------------ #


def _dense_ids(
    p: np.ndarray,
    b: np.ndarray,
    p2: Optional[np.ndarray],
    b2: Optional[np.ndarray],
) -> Tuple[np.ndarray, np.ndarray]:
    if p2 is None:
        return p, b
    both = np.stack([np.concatenate([p, b]), np.concatenate([p2, b2])], axis=1)
    _, inv = np.unique(both, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1).astype(np.int64)
    return inv[: len(p)], inv[len(p) :]


def match_ranges(
    p: np.ndarray,
    b: np.ndarray,
    p2: Optional[np.ndarray] = None,
    b2: Optional[np.ndarray] = None,
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(order, lo, hi): the build rows matching probe row i are
    ``order[lo[i]:hi[i]]``, in ascending build-row order."""
    pid, bid = _dense_ids(
        np.asarray(p, dtype=np.int64),
        np.asarray(b, dtype=np.int64),
        None if p2 is None else np.asarray(p2, dtype=np.int64),
        None if b2 is None else np.asarray(b2, dtype=np.int64),
    )
    order = np.argsort(bid, kind="stable").astype(np.int64)
    sb = bid[order]
    lo = np.searchsorted(sb, pid, side="left").astype(np.int64)
    hi = np.searchsorted(sb, pid, side="right").astype(np.int64)
    return order, lo, hi


def match_counts(p, b, p2=None, b2=None) -> np.ndarray:
    _, lo, hi = match_ranges(p, b, p2, b2)
    return hi - lo


def out_counts(counts: np.ndarray, mode: int) -> np.ndarray:
    """Output rows per probe row: 0=inner 1=left 2=semi 3=anti."""
    if mode == 0:
        return counts
    if mode == 1:
        return np.maximum(counts, 1)
    if mode == 2:
        return (counts > 0).astype(np.int64)
    return (counts == 0).astype(np.int64)


def join_pairs_ref(
    p, b, mode: int, p2=None, b2=None
) -> Tuple[np.ndarray, np.ndarray]:
    """(probe_idx, build_idx) of the join, probe-major then ascending
    build row.  Semi reports the lowest matching build row; left and anti
    report -1 for unmatched probe rows."""
    order, lo, hi = match_ranges(p, b, p2, b2)
    cnt = hi - lo
    n_p = len(cnt)
    rows = np.arange(n_p, dtype=np.int64)
    if mode == 2 or mode == 3:
        sel = cnt > 0 if mode == 2 else cnt == 0
        pi = rows[sel]
        if mode == 3:
            return pi, np.full(len(pi), -1, dtype=np.int64)
        return pi, order[lo[sel]]
    oc = out_counts(cnt, mode)
    total = int(oc.sum())
    pi = np.repeat(rows, oc)
    start = np.cumsum(oc) - oc
    within = np.arange(total, dtype=np.int64) - np.repeat(start, oc)
    matched = np.repeat(cnt > 0, oc)
    pos = np.repeat(lo, oc) + within
    bi = np.full(total, -1, dtype=np.int64)
    bi[matched] = order[pos[matched]]
    return pi, bi


def sorted_pairs(pi, bi) -> np.ndarray:
    """[m, 2] pairs in lexicographic order (multiset comparison)."""
    pi = np.asarray(pi, dtype=np.int64).reshape(-1)
    bi = np.asarray(bi, dtype=np.int64).reshape(-1)
    o = np.lexsort((bi, pi))
    return np.stack([pi[o], bi[o]], axis=1)


# ------------------------------------------------------------------ #
# postfix expression programs                                         #
# ------------------------------------------------------------------ #

XOP = dict(
    COL=0, LIT_D=1, LIT_I=2, ADD=3, SUB=4, MUL=5, DIV=6,
    LT=7, LE=8, GT=9, GE=10, EQ=11, NE=12, AND=13, OR=14, NOT=15,
    ISNULL=16, NOTNULL=17, NEG=18,
)
TAG_F, TAG_I, TAG_B = 0, 1, 2


class _Val:
    def __init__(self, tag: int, v: np.ndarray, valid: np.ndarray):
        self.tag, self.v, self.valid = tag, v, valid


def run_program(
    ops: Sequence[int],
    aux: Sequence[int],
    imm: Sequence[int],
    cols: List[Tuple[np.ndarray, Optional[np.ndarray]]],
    n: int,
    wide: bool = False,
) -> Tuple[int, np.ndarray, np.ndarray]:
    """Evaluate a postfix program row-wise; returns (tag, values, valid)
    of the top of stack.

    Semantics: arithmetic propagates invalid; comparisons on null give
    false; AND/OR/NOT treat null as false; IS NULL reads the validity
    bit; int (+,-,*) int stays int64 with two's-complement wrap; anything
    with a float operand, and every DIV, is floating point.  ``wide``
    evaluates the floating-point values in ``np.longdouble``."""
    ft = np.longdouble if wide else np.float64
    st: List[_Val] = []
    ones = np.ones(n, dtype=bool)

    def as_f(x: _Val) -> np.ndarray:
        return x.v if x.tag == TAG_F else x.v.astype(ft)

    def truth(x: _Val) -> np.ndarray:
        return x.valid & (x.v != 0)

    with np.errstate(all="ignore"):
        for op, ax in zip(ops, aux):
            if op == XOP["COL"]:
                data, valid = cols[ax]
                vd = ones if valid is None else np.asarray(valid, dtype=bool)
                if data.dtype.kind == "f":
                    st.append(_Val(TAG_F, data.astype(ft), vd))
                elif data.dtype.kind == "b":
                    st.append(_Val(TAG_B, data.astype(np.int64), vd))
                else:
                    st.append(_Val(TAG_I, data.astype(np.int64), vd))
            elif op == XOP["LIT_D"]:
                d = np.array([imm[ax]], dtype=np.int64).view(np.float64)[0]
                st.append(_Val(TAG_F, np.full(n, d, dtype=ft), ones))
            elif op == XOP["LIT_I"]:
                st.append(_Val(TAG_I, np.full(n, imm[ax], dtype=np.int64), ones))
            elif op == XOP["NOT"]:
                a = st.pop()
                st.append(_Val(TAG_B, (~truth(a)).astype(np.int64), ones))
            elif op in (XOP["ISNULL"], XOP["NOTNULL"]):
                a = st.pop()
                r = ~a.valid if op == XOP["ISNULL"] else a.valid
                st.append(_Val(TAG_B, r.astype(np.int64), ones))
            elif op == XOP["NEG"]:
                a = st.pop()
                st.append(_Val(a.tag, -a.v, a.valid))
            elif op in (XOP["AND"], XOP["OR"]):
                b = st.pop()
                a = st.pop()
                r = (
                    truth(a) & truth(b)
                    if op == XOP["AND"]
                    else truth(a) | truth(b)
                )
                st.append(_Val(TAG_B, r.astype(np.int64), ones))
            else:
                b = st.pop()
                a = st.pop()
                both_int = a.tag != TAG_F and b.tag != TAG_F
                valid = a.valid & b.valid
                if XOP["ADD"] <= op <= XOP["DIV"]:
                    if op == XOP["DIV"] or not both_int:
                        x, y = as_f(a), as_f(b)
                        tag = TAG_F
                    else:
                        x, y = a.v, b.v
                        tag = TAG_I
                    if op == XOP["ADD"]:
                        r = x + y
                    elif op == XOP["SUB"]:
                        r = x - y
                    elif op == XOP["MUL"]:
                        r = x * y
                    else:
                        r = x / y
                    st.append(_Val(tag, r, valid))
                else:
                    x, y = (a.v, b.v) if both_int else (as_f(a), as_f(b))
                    r = {
                        XOP["LT"]: np.less, XOP["LE"]: np.less_equal,
                        XOP["GT"]: np.greater, XOP["GE"]: np.greater_equal,
                        XOP["EQ"]: np.equal, XOP["NE"]: np.not_equal,
                    }[op](x, y)
                    st.append(_Val(TAG_B, (r & valid).astype(np.int64), ones))
    assert len(st) == 1, "program must leave exactly one value"
    top = st[0]
    return top.tag, top.v, top.valid


def filter_of(tag: int, v: np.ndarray, valid: np.ndarray) -> np.ndarray:
    """The filter kernel's output for a program result: valid and truthy."""
    return valid & (v != 0)


def program_of(builder: Any) -> Tuple[List[int], List[int], List[int], list]:
    """(ops, aux, imm, cols-as-numpy) of an expression program builder."""
    cols = [
        (
            c.data.cpu().numpy(),
            None if c.valid is None else c.valid.cpu().numpy(),
        )
        for c in builder.cols
    ]
    return list(builder.ops), list(builder.aux), list(builder.imm), cols


# ------------------------------------------------------------------ #
# row hashing (hash_partition.hip)                                    #
# ------------------------------------------------------------------ #

U64 = 2**64 - 1
GOLDEN = 0x9E3779B97F4A7C15
NULL_HASH = GOLDEN  # canonical hash of a null cell, any column type
BYTES_SEED = 0x27D4EB2F165667C5


def mix64_int(x: int) -> int:
    """``mix64`` on one Python int (mod 2^64)."""
    x &= U64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & U64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & U64
    x ^= x >> 33
    return x


def hash_combine_int(h: int, v: int) -> int:
    return mix64_int(h ^ ((v + GOLDEN + (h << 6) + (h >> 2)) & U64))


def hash_combine(h: np.ndarray, v: np.ndarray) -> np.ndarray:
    """Fold the cell hashes ``v`` into the running row hashes ``h``."""
    h = np.asarray(h, dtype=np.uint64)
    v = np.asarray(v, dtype=np.uint64)
    with np.errstate(over="ignore"):
        t = v + np.uint64(GOLDEN) + (h << np.uint64(6)) + (h >> np.uint64(2))
    return mix64(h ^ t)


def hash_bytes(b: bytes) -> int:
    """Hash of one string cell: the length goes into the seed, whole
    8-byte blocks are read little-endian, the 1..7 byte tail is
    accumulated big-endian, one ``mix64`` finishes."""
    n = len(b)
    h = BYTES_SEED ^ n
    full = n - n % 8
    for i in range(0, full, 8):
        h = hash_combine_int(h, int.from_bytes(b[i : i + 8], "little"))
    if full < n:
        h = hash_combine_int(h, int.from_bytes(b[full:], "big"))
    return mix64_int(h)


def seeded_start(seed: int) -> int:
    """Row hash before the first column of a seeded hash family."""
    return mix64_int(seed + 1)


def cell_bits(data: np.ndarray) -> np.ndarray:
    """The raw bits ``hash_rows`` feeds to ``mix64`` for a fixed-width
    column, zero-extended to uint64: int8/bool as one byte, int16 widened
    (sign-extended) to int32 first, 4-byte types as uint32, 8-byte types
    as they are.  Floats hash by bit pattern, not by value."""
    data = np.ascontiguousarray(data)
    if data.dtype == np.bool_:
        data = data.astype(np.uint8)
    if data.dtype == np.int16:
        data = data.astype(np.int32)
    view = {1: np.uint8, 4: np.uint32, 8: np.uint64}[data.dtype.itemsize]
    return data.view(view).astype(np.uint64)


def hash_rows_ref(
    columns: Sequence[Tuple[Any, Optional[np.ndarray]]],
    seed: Optional[int] = None,
) -> np.ndarray:
    """uint64 row hashes over ``columns``: (data, valid-or-None) pairs,
    where data is a fixed-width numpy array or, for a string column, a
    list of ``bytes``.  The first column's cell hash is the row hash
    unless a seed gives a start value; later columns are combined in."""
    n = len(columns[0][0])
    out = None
    if seed is not None:
        out = np.full(n, seeded_start(seed), dtype=np.uint64)
    for data, valid in columns:
        if isinstance(data, np.ndarray) and data.dtype != object:
            v = mix64(cell_bits(data)) if n else np.empty(0, dtype=np.uint64)
        else:
            v = np.array([hash_bytes(bytes(b)) for b in data], dtype=np.uint64)
        if valid is not None:
            v = np.where(np.asarray(valid, dtype=bool), v, np.uint64(NULL_HASH))
        out = v if out is None else hash_combine(out, v)
    return out


def bucket_of_ref(hashes: np.ndarray, num_buckets: int) -> np.ndarray:
    """Bucket of a row hash: the UNSIGNED value modulo the bucket count."""
    h = np.ascontiguousarray(hashes).view(np.uint64)
    return (h % np.uint64(num_buckets)).astype(np.int32)


def part_of(keys: np.ndarray, num_parts: int) -> np.ndarray:
    """Hash partition of a group key: the top log2(P) bits of mix64."""
    bits = num_parts.bit_length() - 1
    assert 1 << bits == num_parts, "power of two"
    h = mix64(np.asarray(keys, dtype=np.int64))
    if bits == 0:
        return np.zeros(len(h), dtype=np.int64)
    return (h >> np.uint64(64 - bits)).astype(np.int64)


# ------------------------------------------------------------------ #
# group-by and keyless reductions (groupby.hip)                       #
# ------------------------------------------------------------------ #

OP_SUM, OP_MIN, OP_MAX, OP_COUNT = 0, 1, 2, 3


def _fsum(v: np.ndarray) -> float:
    """Exact sum rounded once, started from +0.0 as the tables are (so a
    group of only -0.0 sums to +0.0); inf and nan follow IEEE addition."""
    if not np.isfinite(v).all():
        with np.errstate(invalid="ignore"):
            return float(np.sum(v))
    return math.fsum(v.tolist()) + 0.0


def _reduce(v: np.ndarray, op: int) -> float:
    """One aggregate over the valid values ``v`` of a group or column;
    the identity (0, +inf, -inf) where there are none."""
    if op == OP_COUNT:
        return float(len(v))
    if op == OP_SUM:
        return _fsum(v)
    if len(v) == 0:
        return np.inf if op == OP_MIN else -np.inf
    return float(v.min() if op == OP_MIN else v.max())


def groupby_ref(
    keys: np.ndarray,
    vals: np.ndarray,
    valids: Optional[np.ndarray],
    ops: Sequence[int],
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(distinct keys ascending, rows per key, aggregates [A, G]) of
    ``vals`` [A, n] grouped by ``keys``; ``valids`` [A, n] or None masks
    single cells out of their aggregate but never out of the row count."""
    keys = np.asarray(keys, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64).reshape(len(ops), len(keys))
    ukeys, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(inv, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = np.empty((len(ops), len(ukeys)), dtype=np.float64)
    for a, op in enumerate(ops):
        v = vals[a][order]
        ok = None if valids is None else np.asarray(valids[a], dtype=bool)[order]
        for g in range(len(ukeys)):
            seg = v[bounds[g] : bounds[g + 1]]
            if ok is not None:
                seg = seg[ok[bounds[g] : bounds[g + 1]]]
            out[a, g] = _reduce(seg, op)
    return ukeys, counts.astype(np.int64), out


def abs_sums(keys: np.ndarray, v: np.ndarray) -> np.ndarray:
    """Per distinct key (ascending): exact sum of |v|, for the any-order
    summation bound (m - 1) * 2^-53 * sum|v| of a group of m rows."""
    return groupby_ref(keys, np.abs(v)[None, :], None, [OP_SUM])[2][0]


def reduce_cols_ref(
    vals: np.ndarray, valids: Optional[np.ndarray], ops: Sequence[int]
) -> Tuple[np.ndarray, np.ndarray]:
    """(values [A], valid counts [A]) of whole-column SUM/MIN/MAX."""
    vals = np.asarray(vals, dtype=np.float64)
    out = np.empty(len(ops), dtype=np.float64)
    cnt = np.empty(len(ops), dtype=np.int64)
    for a, op in enumerate(ops):
        v = vals[a] if valids is None else vals[a][np.asarray(valids[a], bool)]
        out[a], cnt[a] = _reduce(v, op), len(v)
    return out, cnt


def table_groups(tkeys, gcount, gaggs):
    """A kernel's group table as (keys ascending, counts, aggs [A, G]):
    the occupied slots, which must hold each key once."""
    tkeys = np.asarray(tkeys)
    occ = np.flatnonzero(tkeys != INT64_MIN)
    k = tkeys[occ]
    o = np.argsort(k, kind="stable")
    assert len(np.unique(k)) == len(k), "a key sits in two slots"
    return k[o], np.asarray(gcount)[occ][o], np.asarray(gaggs)[:, occ][:, o]


# ------------------------------------------------------------------ #
# group-by key preparation (groupby.hip)                              #
# ------------------------------------------------------------------ #


def key_stats_ref(
    cols: Sequence[np.ndarray],
    valids: Sequence[Optional[np.ndarray]],
    nsamples: int,
) -> Tuple[List[int], List[int], int, int, int]:
    """(mins, maxs, d, f1, f2): per-column min and max of the stored
    values (null cells included: the kernel reads data only), and over
    the launcher's strided sample (rows ``s * stride``) the number of
    distinct key rows and of those seen exactly once and exactly twice.
    A null cell is its own value, distinct from every stored one."""
    n = len(cols[0])
    mins = [int(c.min()) for c in cols]
    maxs = [int(c.max()) for c in cols]
    stride = max(1, n // nsamples)
    eff = min(nsamples, n // stride)
    rows = np.arange(eff, dtype=np.int64) * stride
    seen: dict = {}
    sampled = [
        [
            None if (v is not None and not v[r]) else int(c[r])
            for r in rows
        ]
        for c, v in zip(cols, valids)
    ]
    for row in zip(*sampled):
        seen[row] = seen.get(row, 0) + 1
    mult = list(seen.values())
    return mins, maxs, len(mult), mult.count(1), mult.count(2)


def code_width(lo: int, hi: int) -> int:
    """Bits of a packed key column whose codes run 0 .. hi - lo + 1: the
    smallest width w >= 1 with hi - lo + 1 < 2^w."""
    top, w = int(hi) - int(lo) + 1, 1
    while top >= (1 << w):
        w += 1
    return w


def pack_shifts(widths: Sequence[int]) -> List[int]:
    """Bit position of each column: the last column sits at bit 0."""
    shifts, s = [], 0
    for w in reversed(list(widths)):
        shifts.append(s)
        s += w
    return shifts[::-1]


def pack_ref(
    cols: Sequence[np.ndarray],
    valids: Sequence[Optional[np.ndarray]],
    mins: Sequence[int],
    widths: Sequence[int],
) -> np.ndarray:
    """Packed int64 group keys: per column code 0 = null, value - min + 1
    otherwise, OR-ed together at ``pack_shifts(widths)``."""
    n = len(cols[0])
    out = [0] * n
    for c, v, lo, sh in zip(cols, valids, mins, pack_shifts(widths)):
        for i in range(n):
            code = 0 if (v is not None and not v[i]) else int(c[i]) - lo + 1
            assert 0 <= code, "min is not the column minimum"
            out[i] |= code << sh
    assert all(0 <= x < 2**63 for x in out), "wider than 63 bits"
    return np.array(out, dtype=np.int64)


def unpack_ref(
    packed: np.ndarray, mins: Sequence[int], widths: Sequence[int]
) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Per column (values int64, valid) out of packed keys; the value of
    a null cell is min - 1 and means nothing."""
    res = []
    p = [int(x) for x in packed]
    for lo, w, sh in zip(mins, widths, pack_shifts(widths)):
        codes = [(x >> sh) & ((1 << w) - 1) for x in p]
        res.append(
            (
                np.array([c - 1 + lo for c in codes], dtype=np.int64),
                np.array([c != 0 for c in codes], dtype=bool),
            )
        )
    return res
