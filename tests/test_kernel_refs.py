"""CPU tests of the references in ``kernel_refs.py`` that the GPU kernel
tests compare against: the join-pair reference against the ops layer's
pandas join, the hash against the ops layer's numpy copy, and the
postfix-program reference on hand-computed rows."""
import numpy as np
import pyarrow as pa
import pytest

torch = pytest.importorskip("torch")

import kernel_refs as kr
from fugue_amd.column.expressions import col, lit
from fugue_amd.hip import expr as hexpr
from fugue_amd.hip import ops as dops
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
from fugue_amd.schema import Schema

I64_MIN, I64_MAX = kr.INT64_MIN, kr.INT64_MAX
MODES = {"inner": 0, "left": 1, "semi": 2, "anti": 3}


def _join_case(seed: int, with_h2: bool):
    rng = np.random.default_rng(seed)
    b = rng.integers(-20, 20, 300).astype(np.int64)
    p = rng.integers(-30, 30, 500).astype(np.int64)
    b[:4] = [I64_MIN, I64_MAX, 0, -1]
    p[:4] = [I64_MIN, I64_MAX, 0, -1]
    if not with_h2:
        return p, b, None, None
    return p, b, rng.integers(0, 3, 500), rng.integers(0, 3, 300)


@pytest.mark.parametrize("with_h2", [False, True])
@pytest.mark.parametrize("how", list(MODES))
def test_join_reference_matches_ops_cpu(how, with_h2):
    p, b, p2, b2 = _join_case(5, with_h2)
    t = torch.from_numpy
    ep, eb = dops._hash_join_indices_cpu(
        t(p), t(b), how,
        None if p2 is None else t(p2), None if b2 is None else t(b2),
    )
    gp, gb = kr.join_pairs_ref(p, b, MODES[how], p2, b2)
    exp = kr.sorted_pairs(ep.numpy(), eb.numpy())
    got = kr.sorted_pairs(gp, gb)
    assert len(exp) > 0
    np.testing.assert_array_equal(got, exp)
    # counts agree with the pair list
    cnt = kr.match_counts(p, b, p2, b2)
    assert int(kr.out_counts(cnt, MODES[how]).sum()) == len(exp)


def test_join_reference_empty_sides():
    e = np.empty(0, dtype=np.int64)
    p = np.array([3, 4, 3], dtype=np.int64)
    for mode in range(4):
        pi, bi = kr.join_pairs_ref(e, p, mode)
        assert len(pi) == 0 and len(bi) == 0
    assert len(kr.join_pairs_ref(p, e, 0)[0]) == 0
    assert len(kr.join_pairs_ref(p, e, 2)[0]) == 0
    for mode in (1, 3):
        pi, bi = kr.join_pairs_ref(p, e, mode)
        np.testing.assert_array_equal(pi, [0, 1, 2])
        np.testing.assert_array_equal(bi, [-1, -1, -1])


def test_mix64_matches_ops_copy_and_known_value():
    x = np.array([0, 1, -1, I64_MIN, I64_MAX, 123456789], dtype=np.int64)
    np.testing.assert_array_equal(
        kr.mix64(x), dops._np_mix64(x.view(np.uint64).copy())
    )
    # fmix64(1), by hand from the two multiply/xor-shift rounds
    v = 1
    for m in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53):
        v ^= v >> 33
        v = (v * m) & (2**64 - 1)
    v ^= v >> 33
    assert int(kr.mix64(np.array([1], dtype=np.int64))[0]) == v
    assert int(kr.mix64(np.array([0], dtype=np.int64))[0]) == 0
    s = kr.slot_of(x, 16)
    assert s.min() >= 0 and s.max() < 16


def _frame():
    c = lambda a, v=None: (torch.from_numpy(np.array(a)),
                           None if v is None else torch.tensor(v))
    cols = {
        "a": DeviceColumn(*c(np.array([1, -2, I64_MIN, 3], dtype=np.int64)), pa.int64()),
        "x": DeviceColumn(
            *c(np.array([0.5, 2.0, np.nan, 4.0]), [True, False, True, True]),
            pa.float64(),
        ),
        "h": DeviceColumn(*c(np.array([1, 0, 2, -3], dtype=np.int16)), pa.int16()),
        "b": DeviceColumn(
            *c(np.array([True, False, True, True]), [True, True, False, True]),
            pa.bool_(),
        ),
    }
    return HipDataFrame.from_columns(
        cols, Schema("a:long,x:double,h:short,b:bool"), "cpu"
    )


def _run(e, wide=False):
    df = _frame()
    b = hexpr._ProgBuilder(df)
    b.emit(e)
    tag, v, valid = kr.run_program(*kr.program_of(b), df.count(), wide=wide)
    assert tag == b.tags[-1], "static tag simulation disagrees"
    return tag, v, valid


def test_program_reference_hand_rows():
    # int arithmetic wraps, stays int, all valid
    tag, v, valid = _run(col("a") * lit(2) + col("h"))
    assert tag == kr.TAG_I and valid.all()
    assert v.tolist() == [3, -4, 2, 3]  # I64_MIN*2 wraps to 0
    tag, v, valid = _run(-col("a") - lit(0))
    assert v.tolist() == [-1, 2, I64_MIN, -3]
    # float arithmetic propagates invalid; division is always float
    tag, v, valid = _run(col("x") * col("h") + lit(1))
    assert tag == kr.TAG_F and valid.tolist() == [True, False, True, True]
    assert v[0] == 1.5 and np.isnan(v[2]) and v[3] == -11.0
    tag, v, valid = _run(col("h") / (col("h") - col("h")))
    assert tag == kr.TAG_F and valid.all()
    assert v[0] == np.inf and np.isnan(v[1]) and v[3] == -np.inf
    # comparisons on null are false for every op, != included
    for e in (col("x") != lit(7.0), col("x") < lit(7.0)):
        tag, v, valid = _run(e)
        assert tag == kr.TAG_B and valid.all()
        assert kr.filter_of(tag, v, valid).tolist()[1] is False
    # NaN: != is true, == and < are false
    assert kr.filter_of(*_run(col("x") != col("x"))).tolist() == [
        False, False, True, False]
    assert kr.filter_of(*_run(col("x") == col("x"))).tolist() == [
        True, False, False, True]
    # NOT / AND / OR treat null as false; IS NULL reads the bit
    assert kr.filter_of(*_run(~col("b"))).tolist() == [False, True, True, False]
    assert kr.filter_of(*_run(col("b") & (col("x") > lit(0)))).tolist() == [
        True, False, False, True]
    assert kr.filter_of(*_run(col("b") | col("x").is_null())).tolist() == [
        True, True, False, True]
    assert kr.filter_of(*_run(col("b").is_null())).tolist() == [
        False, False, True, False]
    assert kr.filter_of(*_run(col("x").not_null())).tolist() == [
        True, False, True, True]
    # bool under arithmetic is an int; float against int compares as float
    tag, v, valid = _run(col("b") + col("b"))
    assert tag == kr.TAG_I and v.tolist() == [2, 0, 2, 2]
    assert valid.tolist() == [True, True, False, True]
    assert kr.filter_of(*_run(col("x") > col("a"))).tolist() == [
        False, False, False, True]
    # wide mode carries more than 53 bits
    tag, v, valid = _run(col("x") / lit(3.0), wide=True)
    assert v.dtype == np.longdouble
    assert v[0] != np.longdouble(np.float64(0.5) / np.float64(3.0))
