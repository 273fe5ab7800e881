"""Plain numpy references shared by the join and select kernel tests
(``test_join_kernels_gpu.py``, ``test_select_kernels_gpu.py``) and kept
under test themselves by ``test_kernel_refs.py``.  Nothing here touches
the device or the engine's own evaluators."""
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
