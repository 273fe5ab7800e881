"""GPU tests of the row-selection kernel family (``select.hip``) called
through ``get_ext()`` (and through the thin Python callers that pick
the kernel), compared with plain numpy references: ``kernel_refs.py``
for the postfix expression programs, numpy indexing and comparisons for
the rest.  Masks, indices and integers are compared exactly, float
payloads bitwise; only the float results of expression programs carry a
bound, derived below."""
import numpy as np
import pyarrow as pa
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

import kernel_refs as kr
from fugue_amd.column.expressions import col, lit
from fugue_amd.hip import expr as hexpr
from fugue_amd.hip.ext import get_ext
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
from fugue_amd.schema import Schema

I64_MIN, I64_MAX = kr.INT64_MIN, kr.INT64_MAX
DEVICE = "cuda:0"

_PA = {
    np.dtype("int64"): (pa.int64(), "long"),
    np.dtype("int32"): (pa.int32(), "int"),
    np.dtype("int16"): (pa.int16(), "short"),
    np.dtype("int8"): (pa.int8(), "byte"),
    np.dtype("float64"): (pa.float64(), "double"),
    np.dtype("float32"): (pa.float32(), "float"),
    np.dtype("bool"): (pa.bool_(), "bool"),
}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _bits(a: np.ndarray) -> np.ndarray:
    """Same-width unsigned view, for bitwise comparison."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return a.astype(np.uint8)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def _frame(cols: dict) -> HipDataFrame:
    """{name: array | (array, valid)} -> device frame."""
    dcols, fields = {}, []
    for name, spec in cols.items():
        data, valid = spec if isinstance(spec, tuple) else (spec, None)
        tp, sname = _PA[np.asarray(data).dtype]
        dcols[name] = DeviceColumn(
            _dev(data), None if valid is None else _dev(valid), tp
        )
        fields.append(f"{name}:{sname}")
    return HipDataFrame.from_columns(dcols, Schema(",".join(fields)), DEVICE)


# ------------------------------------------------------------------ #
# 1. gather_columns                                                   #
# ------------------------------------------------------------------ #


def _gather_sources(n: int, rng) -> list:
    f = rng.standard_normal(n)
    f[::7] = np.nan
    f[1::7] = -0.0
    f[2::7] = np.inf
    srcs = []
    for j in range(5):
        srcs.append(rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64))
    for j in range(4):
        srcs.append(np.roll(f, j))
    # a NaN with a payload survives only a bitwise copy
    srcs[5] = srcs[5].copy()
    srcs[5].view(np.uint64)[::7] = np.uint64(0x7FF800000000BEEF)
    srcs.append(rng.integers(-(2**31), 2**31, n).astype(np.int32))
    srcs.append(rng.integers(-(2**31), 2**31, n).astype(np.int32))
    srcs.append(np.roll(f, 5).astype(np.float32))
    srcs.append(np.roll(f, 6).astype(np.float32))
    srcs.append(rng.integers(-(2**15), 2**15, n).astype(np.int16))
    srcs.append(rng.integers(-128, 128, n).astype(np.int8))
    srcs.append(rng.random(n) < 0.5)
    order = rng.permutation(len(srcs))  # widths interleaved
    return [srcs[i] for i in order]


@pytest.mark.parametrize("n_idx", [0, 1, 257, 100_003])
def test_gather_columns(n_idx):
    rng = np.random.default_rng(n_idx)
    n = 1000
    srcs = _gather_sources(n, rng)
    assert len(srcs) == 16
    assert sum(s.itemsize == 8 for s in srcs) == 9  # more than half the slots
    idx = rng.integers(0, n, n_idx).astype(np.int64)
    if n_idx >= 4:
        idx[[0, 1, -2, -1]] = [n - 1, 0, 0, n - 1]
    elif n_idx == 1:
        idx[0] = n - 1
    dsrc = [_dev(s) for s in srcs]
    outs = get_ext().gather_columns(_dev(idx), dsrc)
    assert len(outs) == 16
    for s, d, o in zip(srcs, dsrc, outs):
        assert o.dtype == d.dtype and o.shape == (n_idx,)
        np.testing.assert_array_equal(_bits(_host(o)), _bits(s[idx]))
    # a single column
    (o,) = get_ext().gather_columns(_dev(idx), dsrc[3:4])
    np.testing.assert_array_equal(_bits(_host(o)), _bits(srcs[3][idx]))


def test_gather_columns_rejects_strided():
    idx = _dev(np.array([0, 1], dtype=np.int64))
    strided = torch.arange(20, device="cuda")[::2]
    with pytest.raises(RuntimeError):
        get_ext().gather_columns(idx, [strided])
    with pytest.raises(RuntimeError):
        get_ext().gather_columns(idx, [])


def test_gather_rows_twenty_columns():
    """A 20-column frame with three validity masks is 23 flat tensors:
    the frame gathers them in slices of 16 and 7."""
    rng = np.random.default_rng(20)
    n = 3000
    dts = [np.int64, np.float64, np.int32, np.float32, np.int16, np.int8, np.bool_]
    cols = {}
    for j in range(20):
        dt = np.dtype(dts[j % len(dts)])
        if dt.kind == "f":
            data = rng.standard_normal(n).astype(dt)
            data[j::11] = np.nan
        elif dt.kind == "b":
            data = rng.random(n) < 0.5
        else:
            data = rng.integers(-100, 100, n).astype(dt)
        cols[f"c{j}"] = (data, rng.random(n) < 0.8) if j in (2, 9, 17) else data
    df = _frame(cols)
    idx = rng.integers(0, n, 5001).astype(np.int64)
    idx[:2] = [0, n - 1]
    out = df.gather_rows(_dev(idx))
    assert out.schema == df.schema and out.count() == len(idx)
    for name, spec in cols.items():
        data, valid = spec if isinstance(spec, tuple) else (spec, None)
        c = out.col(name)
        np.testing.assert_array_equal(_bits(_host(c.data)), _bits(data[idx]))
        if valid is None:
            assert c.valid is None
        else:
            np.testing.assert_array_equal(_host(c.valid), valid[idx])


# ------------------------------------------------------------------ #
# 2. expr_filter / expr_value against the postfix reference           #
# ------------------------------------------------------------------ #


def _expr_frame(n: int) -> HipDataFrame:
    rng = np.random.default_rng(1000 + n)
    x = rng.uniform(0.5, 2.0, n)
    a = rng.integers(-1000, 1000, n).astype(np.int64)
    amin = a.copy()
    amin[::3] = I64_MIN
    xn = x.copy()
    xn[rng.random(n) < 0.2] = np.nan
    xn[0] = np.nan
    c = rng.integers(-(2**31), 2**31, n).astype(np.int32)
    c[:2] = [2**31 - 1, -(2**31)][: min(n, 2)]
    return _frame(
        dict(
            x=(x, rng.random(n) > 0.1),
            y=rng.uniform(0.5, 2.0, n),
            d=rng.uniform(0.01, 0.1, n),
            g=rng.uniform(0.5, 2.0, n).astype(np.float32),
            a=a,
            q=rng.integers(1, 50, n).astype(np.int64),
            big=rng.integers(2**61, 2**62, n).astype(np.int64),
            amin=amin,
            c=c,
            s=rng.integers(-(2**15), 2**15, n).astype(np.int16),
            t=(rng.integers(-128, 128, n).astype(np.int8), rng.random(n) > 0.2),
            bl=(rng.random(n) < 0.5, rng.random(n) > 0.2),
            z=rng.integers(-1, 2, n).astype(np.int64),
            xn=xn,
        )
    )


def _right_leaning(leaves, op="+"):
    e = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        e = leaf + e if op == "+" else leaf * e
    return e


def _chain(leaves, op="+"):
    e = leaves[0]
    for leaf in leaves[1:]:
        e = e + leaf if op == "+" else e * leaf
    return e


def _xy(k):
    return [col("x") if i % 2 == 0 else col("y") for i in range(k)]


def _lits(k):
    return [lit(1.5 + i) for i in range(k)]


FILTERS = [
    lambda: (col("a") > lit(0)) & (col("x") < lit(1.0)),
    lambda: (col("a") + lit(3)) * lit(2) >= col("a") - lit(1),
    lambda: col("x").is_null() | (col("a") == lit(7)),
    lambda: ~(col("x").not_null()) | (col("x") / lit(2.0) > lit(0.6)),
    # NOT / AND / OR / IS NULL / NOT NULL over null operands
    lambda: ~(col("x") > lit(1.0)),
    lambda: ~col("bl"),
    lambda: col("bl") & (col("t") > lit(0)),
    lambda: col("bl") | col("x").is_null(),
    lambda: col("t").is_null() | col("bl").not_null(),
    lambda: ~(col("t") + lit(1) > lit(0)) & col("x").not_null(),
    # every comparison, over every column tag
    lambda: col("g") <= col("y"),
    lambda: col("c") != col("s"),
    lambda: col("t") < col("c"),
    lambda: col("s") >= lit(3),
    lambda: (col("c") == lit(2**31 - 1)) | (col("c") < lit(-(2**31) + 1)),
    lambda: col("g") * lit(2) > col("s") / lit(10000),
    # binary-op branch: float against int, bool under arithmetic
    lambda: col("y") > col("q"),
    lambda: col("bl") + col("q") > lit(1),
    lambda: col("bl") * col("a") - col("bl") < lit(0),
    # NaN comparands and NaN truthiness
    lambda: col("xn") == col("xn"),
    lambda: col("xn") != col("y"),
    lambda: ~(col("xn") > col("y")),
    lambda: col("xn") & col("bl"),
    lambda: (col("xn") + lit(0.0)) | col("t").is_null(),
    # int64 wrap, -INT64_MIN, division by zero
    lambda: -col("amin") < lit(0),
    lambda: col("big") * col("big") > lit(0),
    lambda: col("big") * lit(3) + col("big") > col("big"),
    lambda: col("a") / col("z") > lit(0),
    lambda: (col("z") / col("z")) != (col("z") / col("z")),
    # the limits: depth 12, 12 immediates, 48 ops
    lambda: _right_leaning(_xy(12)) > lit(14.0),
    lambda: _chain([col("x")] + _lits(11)) > lit(72.7),
    lambda: ~(_chain(_xy(23), "*") > lit(1.0)),
]

# int-tagged programs are compared exactly, float-tagged ones by the bound
VALUES = [
    lambda: (col("q") * lit(3) + lit(7)) - col("q"),
    lambda: col("big") * col("big"),
    lambda: col("big") * lit(3) + col("big"),
    lambda: (-col("amin")) * lit(1),
    lambda: col("c") * col("s") + col("t"),
    lambda: col("bl") + col("bl") * lit(2),
    lambda: col("x") * (lit(1) - col("d")),
    lambda: (col("x") + col("y")) / (col("q") + lit(1)),
    lambda: col("g") * col("y") + col("x"),
    lambda: col("y") - col("d"),
    lambda: col("a") / col("z"),
    lambda: col("q") / lit(7) + col("y") * lit(4.0),
    lambda: _right_leaning(_xy(12)),
    lambda: _chain([col("x")] + _lits(12)),
    lambda: _chain([-col("x")] + _xy(24)[1:], "*"),
]


def _prog(df, e):
    b = hexpr._ProgBuilder(df)
    b.emit(e)
    assert hexpr._fusable(b), "case must fit the interpreter's limits"
    return b


def _n_arith(b) -> int:
    return sum(1 for o in b.ops if kr.XOP["ADD"] <= o <= kr.XOP["DIV"])


@pytest.mark.parametrize("n", [1, 255, 513, 70_001])
def test_expr_filter_vs_reference(n):
    df = _expr_frame(n)
    seen_ops = set()
    limits = dict(depth=0, imm=0, ops=0)
    for i, make in enumerate(FILTERS):
        b = _prog(df, make())
        seen_ops.update(b.ops)
        limits = dict(
            depth=max(limits["depth"], b.max_depth),
            imm=max(limits["imm"], len(b.imm)),
            ops=max(limits["ops"], len(b.ops)),
        )
        tag, v, valid = kr.run_program(*kr.program_of(b), n)
        assert tag == b.tags[-1], f"static tag of filter {i}"
        exp = kr.filter_of(tag, v, valid)
        got = hexpr._run_program(b, df, "filter")
        assert got.dtype == torch.bool
        np.testing.assert_array_equal(_host(got), exp, err_msg=f"filter {i}")
        # the public entry point may pick a dedicated kernel instead
        pub = hexpr.try_fused_filter(make(), df)
        assert pub is not None
        np.testing.assert_array_equal(_host(pub), exp, err_msg=f"filter {i}")
    assert seen_ops == set(kr.XOP.values()), "every opcode is exercised"
    assert limits == dict(depth=12, imm=12, ops=48)


@pytest.mark.parametrize("n", [1, 255, 513, 70_001])
def test_expr_value_vs_reference(n):
    """Int results are exact.  Float results are compared with the same
    program evaluated in ``np.longdouble``: every arithmetic op rounds
    once (relative error at most 2**-53) and a multiply-add may be
    contracted, the operands are positive for ``+`` and far apart for
    ``-`` so no op amplifies the error carried in, hence a program of m
    arithmetic ops is within m * 2**-52 relative."""
    df = _expr_frame(n)
    limits = dict(depth=0, imm=0, ops=0)
    for i, make in enumerate(VALUES):
        b = _prog(df, make())
        limits = dict(
            depth=max(limits["depth"], b.max_depth),
            imm=max(limits["imm"], len(b.imm)),
            ops=max(limits["ops"], len(b.ops)),
        )
        out_int = b.tags[-1] == kr.TAG_I
        assert b.tags[-1] != kr.TAG_B
        prog = kr.program_of(b)
        tag, v, valid = kr.run_program(*prog, n, wide=not out_int)
        assert tag == b.tags[-1], f"static tag of value {i}"
        got, gvalid = hexpr._run_program(b, df, "int" if out_int else "value")
        got, gvalid = _host(got), _host(gvalid)
        np.testing.assert_array_equal(gvalid, valid, err_msg=f"value {i}")
        if out_int:
            assert got.dtype == np.int64
            np.testing.assert_array_equal(got[valid], v[valid], err_msg=f"value {i}")
        else:
            assert got.dtype == np.float64
            m = _n_arith(b)
            ref, g = v[valid], got[valid]
            fin = np.isfinite(ref)
            # inf and NaN (division by zero) must come out as such
            np.testing.assert_array_equal(
                g[~fin], ref[~fin].astype(np.float64), err_msg=f"value {i}"
            )
            err = np.abs(g[fin].astype(np.longdouble) - ref[fin])
            bound = m * np.longdouble(2.0) ** -52 * np.abs(ref[fin])
            nz = ref[fin] != 0
            worst = float((err[nz] / np.abs(ref[fin][nz])).max()) if nz.any() else 0.0
            print(f"value {i}: m={m} worst rel err {worst:.3e}")
            assert (err <= bound).all(), f"value {i}: {worst:.3e} > {m}*2^-52"
        pub = hexpr.try_fused_value(make(), df)
        if pub is not None:
            np.testing.assert_array_equal(
                _bits(_host(pub[0])[valid]), _bits(got[valid]), err_msg=f"value {i}"
            )
            if pub[1] is None:
                assert all(c.valid is None for c in b.cols)
            else:
                np.testing.assert_array_equal(_host(pub[1]), valid)
    assert limits == dict(depth=12, imm=12, ops=48)


def test_expr_division_by_zero_is_valid():
    df = _expr_frame(513)
    b = _prog(df, col("a") / col("z"))
    got, gvalid = hexpr._run_program(b, df, "value")
    got, a, z = _host(got), _host(df.col("a").data), _host(df.col("z").data)
    assert _host(gvalid).all()
    zero = z == 0
    assert zero.any()
    assert np.isinf(got[zero & (a != 0)]).all()
    assert np.isnan(got[zero & (a == 0)]).all()
    np.testing.assert_array_equal(
        np.sign(got[zero & (a != 0)]), np.sign(a[zero & (a != 0)])
    )


def test_expr_past_the_limits_is_not_fused(monkeypatch):
    """One step past the stack depth, the immediate slots or the program
    length: no launch, the caller gets None."""
    df = _expr_frame(255)

    def _no_launch(*_a, **_k):
        raise AssertionError("launched a program past the limits")

    monkeypatch.setattr(hexpr, "_run_program", _no_launch)
    too_deep = _right_leaning(_xy(13))
    too_many_imm = _chain([col("x")] + _lits(13))
    too_long = _chain(_xy(25), "*")
    for e, what in (
        (too_deep, "max_depth"), (too_many_imm, "imm"), (too_long, "ops"),
    ):
        b = hexpr._ProgBuilder(df)
        b.emit(e)
        over = dict(max_depth=b.max_depth, imm=len(b.imm), ops=len(b.ops))
        assert over[what] == dict(max_depth=13, imm=13, ops=49)[what]
        assert hexpr.try_fused_value(e, df) is None
        assert hexpr.try_fused_filter(e > lit(1.0), df) is None
        assert hexpr.try_fused_filter(e, df) is None


# ------------------------------------------------------------------ #
# 3. cmp_imm / cmp_col                                                #
# ------------------------------------------------------------------ #

CMP_OPS = {
    "==": np.equal, "!=": np.not_equal, "<": np.less, "<=": np.less_equal,
    ">": np.greater, ">=": np.greater_equal,
}
_EXPR_OPS = {
    "==": lambda a, b: a == b, "!=": lambda a, b: a != b,
    "<": lambda a, b: a < b, "<=": lambda a, b: a <= b,
    ">": lambda a, b: a > b, ">=": lambda a, b: a >= b,
}
CMP_DTYPES = [np.int64, np.int32, np.int16, np.float64, np.float32]
_FLOAT_EDGES = [np.nan, np.inf, -np.inf, -0.0, 0.0, 0.1]
_INT_LITS = {
    np.int16: [0, 3, 40000, -40000, 32767, -32768],
    np.int32: [0, -4, 2**31, -(2**31), 2**31 - 1],
    np.int64: [0, 5, I64_MIN, I64_MAX, 2**53, 2**53 + 1],
}
_FLOAT_LITS = [0.5, -2.0, 3.0, 0.0, -0.0, 0.1, float("nan"), float("inf"), float("-inf")]


def _cmp_column(dt, n: int, rng, narrow: bool = False) -> np.ndarray:
    dt = np.dtype(dt)
    if dt.kind == "f":
        v = (rng.integers(-6, 7, n) * 0.5).astype(dt)
        edges = np.array(_FLOAT_EDGES).astype(dt)
    else:
        info = np.iinfo(dt)
        v = rng.integers(-6, 7, n).astype(dt)
        edges = [info.min, info.max, 0, -1]
        if dt == np.int64:
            edges = (
                [2**53, -(2**53), 3, -1] if narrow
                else edges + [2**53 + 1, 2**53, -(2**53) - 1]
            )
        edges = np.array(edges, dtype=dt)
    pos = rng.permutation(n)[: len(edges)]
    v[pos] = edges[: len(pos)]
    return v


def _cmp_ref(data, valid, literal, op: str, lit_left: bool) -> np.ndarray:
    """int column with int literal: exact integers; everything else:
    both sides as float64 values.  Null gives false for every op."""
    if data.dtype.kind == "i" and isinstance(literal, int):
        a, b = data.astype(np.int64), np.int64(literal)
    else:
        a, b = data.astype(np.float64), np.float64(literal)
    with np.errstate(invalid="ignore"):
        r = CMP_OPS[op](b, a) if lit_left else CMP_OPS[op](a, b)
    return r if valid is None else r & valid


@pytest.mark.parametrize("n", [1, 1023, 1025, 9001])
def test_cmp_imm(n):
    """Every dtype, op, literal side, with and without validity.

    A mixed int-column / float-literal comparison converts the column to
    float64; that is exact only for |values| <= 2**53, which is the
    kernel's documented contract, so those cases stay inside that range
    (int against int is exact over all of int64 and is tested there)."""
    rng = np.random.default_rng(n)
    ext = get_ext()
    for dt in CMP_DTYPES:
        is_int = np.dtype(dt).kind == "i"
        cases = []
        if is_int:
            cases.append((_cmp_column(dt, n, rng), _INT_LITS[dt]))
            cases.append((_cmp_column(dt, n, rng, narrow=True), _FLOAT_LITS))
        else:
            cases.append((_cmp_column(dt, n, rng), _FLOAT_LITS + [1, 0, -3]))
        for data, lits in cases:
            valid = rng.random(n) < 0.7
            for v in (None, valid):
                df = _frame(dict(a=data if v is None else (data, v)))
                c = df.col("a")
                for literal in lits:
                    imm = (literal, float(literal), True) if isinstance(
                        literal, int) else (0, literal, False)
                    for op in CMP_OPS:
                        tagline = f"{np.dtype(dt)} {op} {literal!r} valid={v is not None}"
                        exp = _cmp_ref(data, v, literal, op, False)
                        got = ext.cmp_imm(
                            c.data, c.valid, *imm, hexpr._CMP_OP_CODE[op]
                        )
                        np.testing.assert_array_equal(_host(got), exp, err_msg=tagline)
                        got = hexpr._try_simple_cmp(
                            _EXPR_OPS[op](col("a"), lit(literal)), df
                        )
                        assert got is not None, tagline
                        np.testing.assert_array_equal(_host(got), exp, err_msg=tagline)
                        # literal on the left: the op must be mirrored
                        exp = _cmp_ref(data, v, literal, op, True)
                        got = hexpr._try_simple_cmp(
                            _EXPR_OPS[op](lit(literal), col("a")), df
                        )
                        assert got is not None, tagline
                        np.testing.assert_array_equal(
                            _host(got), exp, err_msg="mirrored " + tagline
                        )


def test_cmp_imm_float32_is_widened_not_the_literal():
    """A float32 0.1 is not the double 0.1; 2**53 + 1 against 2**53 is
    unequal as integers."""
    df = _frame(dict(f=np.array([0.1, 0.5], dtype=np.float32),
                     i=np.array([2**53 + 1, 2**53], dtype=np.int64)))
    got = hexpr._try_simple_cmp(col("f") == lit(0.1), df)
    assert _host(got).tolist() == [False, False]
    got = hexpr._try_simple_cmp(col("f") > lit(0.1), df)
    assert _host(got).tolist() == [True, True]
    got = hexpr._try_simple_cmp(col("i") == lit(2**53), df)
    assert _host(got).tolist() == [False, True]
    got = hexpr._try_simple_cmp(lit(2**53) < col("i"), df)
    assert _host(got).tolist() == [True, False]


@pytest.mark.parametrize("n", [1, 1023, 1025, 9001])
def test_cmp_col(n):
    rng = np.random.default_rng(7 * n)
    ext = get_ext()
    for dt in CMP_DTYPES:
        a = _cmp_column(dt, n, rng)
        b = np.where(rng.random(n) < 0.5, a, rng.permutation(a)).astype(dt)
        if np.dtype(dt) == np.int64:
            a[0], b[0] = 2**53 + 1, 2**53  # equal as doubles, not as ints
        elif np.dtype(dt).kind == "f" and n > 1:
            a[0], b[0] = -0.0, 0.0
            a[1] = b[1] = np.nan
        va, vb = rng.random(n) < 0.7, rng.random(n) < 0.7
        for xa, xb in ((None, None), (va, None), (None, vb), (va, vb)):
            df = _frame(dict(
                a=a if xa is None else (a, xa), b=b if xb is None else (b, xb)
            ))
            ca, cb = df.col("a"), df.col("b")
            for op in CMP_OPS:
                if np.dtype(dt).kind == "i":
                    r = CMP_OPS[op](a.astype(np.int64), b.astype(np.int64))
                else:
                    with np.errstate(invalid="ignore"):
                        r = CMP_OPS[op](a.astype(np.float64), b.astype(np.float64))
                for x in (xa, xb):
                    if x is not None:
                        r = r & x
                tagline = f"{np.dtype(dt)} {op}"
                got = ext.cmp_col(
                    ca.data, ca.valid, cb.data, cb.valid, hexpr._CMP_OP_CODE[op]
                )
                np.testing.assert_array_equal(_host(got), r, err_msg=tagline)
                got = hexpr._try_simple_cmp(_EXPR_OPS[op](col("a"), col("b")), df)
                assert got is not None
                np.testing.assert_array_equal(_host(got), r, err_msg=tagline)


# ------------------------------------------------------------------ #
# 4. compact_columns_cap / compact_columns                            #
# ------------------------------------------------------------------ #


def _compact_sources(n: int):
    """An int64 and a float64 source whose every value names its row;
    every seventh float is a NaN carrying the row in its payload."""
    i = np.arange(n, dtype=np.int64)
    ints = i * 3 - 1000
    flt = (i * 0.5 + 0.25).astype(np.float64)
    nanrow = i % 7 == 3
    flt.view(np.uint64)[nanrow] = np.uint64(0x7FF8000000000000) | i[nanrow].astype(np.uint64)
    return ints, flt


def _masks(n: int, rng):
    out = {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool)}
    for name, pos in (("first", 0), ("last", n - 1)):
        m = np.zeros(n, dtype=bool)
        if n > 0:
            m[pos] = True
        out[name] = m
    for pct in (1, 50, 99):
        out[f"{pct}%"] = rng.random(n) < pct / 100.0
    return out


def _check_compact(outs, cursor, layout, srcs, mask):
    """``layout[c]`` is None (row index), "i" or "f".  Rows come out in
    any order: sort them by their row index and compare every column
    with its source at the selected rows, bitwise — so all columns of one
    output row come from one input row."""
    rows = np.flatnonzero(mask)
    total = int(cursor)
    assert total == len(rows) == int(mask.sum())
    got = [_host(o)[:total] for o in outs]
    ints, flt = srcs
    key_col = layout.index(None) if None in layout else layout.index("i")
    key = got[key_col] if layout[key_col] is None else (got[key_col] + 1000) // 3
    order = np.argsort(key, kind="stable")
    np.testing.assert_array_equal(key[order], rows)
    for kind, g in zip(layout, got):
        exp = rows if kind is None else (ints[rows] if kind == "i" else flt[rows])
        assert g.dtype == exp.dtype
        np.testing.assert_array_equal(_bits(g[order]), _bits(exp))


def _run_cap(layout, srcs, dsrcs, mask):
    cols = [None if k is None else dsrcs[k] for k in layout]
    outs = get_ext().compact_columns_cap(_dev(mask), cols)
    assert len(outs) == len(layout) + 1
    for o in outs[:-1]:
        assert o.numel() == len(mask)
    _check_compact(outs[:-1], outs[-1].item(), layout, srcs, mask)


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 50_003])
def test_compact_columns_masks(n):
    rng = np.random.default_rng(n)
    srcs = _compact_sources(n)
    dsrcs = dict(i=_dev(srcs[0]), f=_dev(srcs[1]))
    layouts = [
        [None],
        ["f", None, "i"],
        ["i", "f", "f", "i", None, "f", "i", "f"],
        ["i", "f"],
    ]
    for name, mask in _masks(n, rng).items():
        for layout in layouts:
            _run_cap(layout, srcs, dsrcs, mask)
        # exact-size variant: source columns only, sized by the caller
        total = int(mask.sum())
        outs = get_ext().compact_columns(
            _dev(mask), [dsrcs["i"], dsrcs["f"], dsrcs["i"]], total
        )
        for o in outs:
            assert o.numel() == total
        _check_compact(outs, total, ["i", "f", "i"], srcs, mask)


@pytest.mark.parametrize("n", [4097, 50_003])
def test_compact_columns_every_layout(n):
    """ncols 1..8 with the row-index column in every position."""
    rng = np.random.default_rng(n + 1)
    srcs = _compact_sources(n)
    dsrcs = dict(i=_dev(srcs[0]), f=_dev(srcs[1]))
    mask = rng.random(n) < 0.5
    for ncols in range(1, 9):
        for pos in range(ncols):
            layout = ["i" if c % 2 == 0 else "f" for c in range(ncols)]
            layout[pos] = None
            _run_cap(layout, srcs, dsrcs, mask)
        _run_cap(["i"] + ["f"] * (ncols - 1), srcs, dsrcs, mask)


def test_compact_columns_rejects_bad_columns():
    mask = _dev(np.ones(8, dtype=bool))
    four = torch.zeros(8, dtype=torch.int32, device="cuda")
    eight = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        get_ext().compact_columns_cap(mask, [None, four])
    with pytest.raises(RuntimeError):
        get_ext().compact_columns(mask, [four], 8)
    with pytest.raises(RuntimeError):
        get_ext().compact_columns_cap(mask, [eight] * 9)
    with pytest.raises(RuntimeError):
        get_ext().compact_columns_cap(mask, [])


def test_compact_columns_chunk_loop():
    """More chunks than the grid has blocks (8192 x 4096 rows), so every
    block takes a second chunk and the last chunk is ragged."""
    n = 8192 * 4096 + 4099
    rng = np.random.default_rng(33)
    mask = rng.integers(0, 2, n, dtype=np.uint8).view(np.bool_)
    outs = get_ext().compact_columns_cap(_dev(mask), [None])
    total = int(outs[-1].item())
    rows = np.flatnonzero(mask)
    assert total == len(rows)
    got = _host(outs[0].narrow(0, 0, total))
    got.sort()
    np.testing.assert_array_equal(got, rows)


# ------------------------------------------------------------------ #
# 5. eq2_mask                                                         #
# ------------------------------------------------------------------ #


@pytest.mark.parametrize("n", [1, 1025])
def test_eq2_mask(n):
    rng = np.random.default_rng(n)
    l1, l2 = np.int64(-77), np.int64(I64_MAX)
    combo = rng.integers(0, 4, n)
    combo[0] = 3 if n == 1 else combo[0]
    if n > 4:
        combo[:4] = [0, 1, 2, 3]
    h1 = np.where(combo & 1, l1, rng.integers(0, 50, n)).astype(np.int64)
    h2 = np.where(combo & 2, l2, rng.integers(0, 50, n)).astype(np.int64)
    valid = rng.random(n) < 0.6
    if n > 4:
        valid[:4] = True
        valid[4:8] = False
        h1[4:8], h2[4:8] = [l1, l1, 0, 0], [l2, 0, l2, 0]
    eq = (h1 == l1) & (h2 == l2)
    d = [_dev(x) for x in (h1, h2, np.array([l1]), np.array([l2]))]
    for neg in (False, True):
        for v in (None, valid):
            got = get_ext().eq2_mask(*d, None if v is None else _dev(v), neg)
            exp = ~eq if neg else eq
            if v is not None:
                exp = exp & v  # a null row is false in both polarities
            assert got.dtype == torch.bool
            np.testing.assert_array_equal(_host(got), exp)
