"""Plain numpy reference of ``join_unique_select``: a dict join against
unique build keys, one optional comparison, a projection.  Rows come back
sorted, because the kernel writes them in no defined order."""
from typing import Any, List, Optional, Tuple

import numpy as np

PROBE, BUILD, IMM = 0, 1, 2
# comparison codes of the kernel (cmp_apply): 0 == 1 != 2 < 3 <= 4 > 5 >=
OPS = {
    0: lambda a, b: a == b,
    1: lambda a, b: a != b,
    2: lambda a, b: a < b,
    3: lambda a, b: a <= b,
    4: lambda a, b: a > b,
    5: lambda a, b: a >= b,
}


def match_index(p: np.ndarray, b: np.ndarray) -> np.ndarray:
    """build row of every probe row, -1 when its key is absent (the
    dictionary is the sorted build keys, looked up by bisection)"""
    if len(b) == 0:
        return np.full(len(p), -1, dtype=np.int64)
    order = np.argsort(b, kind="stable")
    sb = b[order]
    assert (sb[1:] != sb[:-1]).all(), "build keys must be unique"
    at = np.minimum(np.searchsorted(sb, p), len(sb) - 1)
    return np.where(sb[at] == p, order[at], -1).astype(np.int64)


def _operand(spec: Tuple[int, Any], pi: np.ndarray, bi: np.ndarray):
    kind, value = spec
    if kind == IMM:
        return value
    return value[pi] if kind == PROBE else value[bi]


def _is_float(x: Any) -> bool:
    if isinstance(x, np.ndarray):
        return x.dtype == np.float64
    return isinstance(x, float)


def pred_mask(pred, pi: np.ndarray, bi: np.ndarray) -> np.ndarray:
    """int64 with int64 compares exactly; anything else in float64, IEEE
    (a NaN fails every comparison but !=), as ``cmp_col_kernel``"""
    if pred is None:
        return np.ones(len(pi), dtype=bool)
    op, lhs, rhs = pred
    a, b = _operand(lhs, pi, bi), _operand(rhs, pi, bi)
    if _is_float(a) or _is_float(b):
        a = np.asarray(a).astype(np.float64)
        b = np.asarray(b).astype(np.float64)
    else:
        a = np.asarray(a, dtype=np.int64)
        b = np.asarray(b, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        return np.broadcast_to(OPS[op](a, b), (len(pi),)).astype(bool)


def bits(a: np.ndarray) -> np.ndarray:
    """8-byte cells as int64 bit patterns (NaN payloads compare equal)"""
    return np.ascontiguousarray(a).view(np.int64)


def sorted_rows(cols: List[np.ndarray]) -> np.ndarray:
    """[rows, ncols] int64 bit patterns, rows sorted lexicographically"""
    if len(cols[0]) == 0:
        return np.zeros((0, len(cols)), dtype=np.int64)
    m = np.stack([bits(c) for c in cols], axis=1)
    return m[np.lexsort(m.T[::-1])]


def join_select_ref(
    p: np.ndarray,
    b: np.ndarray,
    pred: Optional[Tuple[int, Tuple[int, Any], Tuple[int, Any]]],
    out_specs: List[Tuple[int, np.ndarray]],
) -> np.ndarray:
    m = match_index(p, b)
    pi = np.flatnonzero(m >= 0)
    bi = m[pi]
    keep = pred_mask(pred, pi, bi)
    pi, bi = pi[keep], bi[keep]
    return sorted_rows(
        [c[pi] if side == PROBE else c[bi] for side, c in out_specs]
    )
