"""GPU tests of ``join_unique_select`` (``join.hip``): the unique inner
join fused with one residual comparison and the projection, called through
``get_ext()`` and compared with the numpy dictionary join of
``join_select_refs.py``.  The kernel writes its rows in no defined order,
so results are compared as sorted row sets of 8-byte bit patterns, and the
cursor total with them; everything is exact.

``CHUNK`` is the rows one block takes per pass (``COMPACT_CHUNK``) and a
launch starts at most 8192 blocks, so ``8192 * CHUNK + CHUNK + 77`` probe
rows make block 0 and block 1 take a second grid-stride chunk, the last
one ragged.  Every table comes from ``join_build``, so every chain ends
at -1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

import join_select_refs as jr
import kernel_refs as kr
from fugue_amd.hip import ops as dops
from fugue_amd.hip.ext import get_ext

CHUNK = int(get_ext().COMPACT_CHUNK)
MAX_GRID = 8192
I64_MIN, I64_MAX = kr.INT64_MIN, kr.INT64_MAX
PROBE, BUILD, IMM = jr.PROBE, jr.BUILD, jr.IMM


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _spec_dev(spec):
    kind, value = spec
    return (kind, value if kind == IMM else _dev(value))


def _run(p, b, pred, out_specs, tsize=None):
    """kernel result as (sorted rows, cursor total, raw outputs)"""
    ext = get_ext()
    bk = _dev(b)
    if tsize is None:
        tsize = dops._next_pow2(max(16, len(b) * 2))
    heads, nxt, dup = ext.join_build(bk, tsize)
    assert int(dup.item()) == 0
    dpred = None
    if pred is not None:
        dpred = (pred[0], _spec_dev(pred[1]), _spec_dev(pred[2]))
    outs = ext.join_unique_select(
        _dev(p), bk, heads, nxt, dpred, [(s, _dev(c)) for s, c in out_specs]
    )
    total = int(outs[-1].item())
    cols = [t.narrow(0, 0, total).cpu().numpy() for t in outs[:-1]]
    return jr.sorted_rows(cols), total, outs


def _check(p, b, pred, out_specs, tsize=None):
    want = jr.join_select_ref(p, b, pred, out_specs)
    got, total, outs = _run(p, b, pred, out_specs, tsize)
    assert total == len(want)
    np.testing.assert_array_equal(got, want)
    for (side, c), t in zip(out_specs, outs[:-1]):
        assert t.dtype == torch.from_numpy(c[:0]).dtype
    return total


def _distinct(rng, n, lo=I64_MIN, hi=I64_MAX):
    v = np.unique(rng.integers(lo, hi, 2 * n + 16, dtype=np.int64))
    return rng.permutation(v)[:n]


def _sides(rng, np_, nb, frac):
    """nb unique build keys (negative ones among them) and np_ probe keys
    of which about ``frac`` find a match"""
    pool = _distinct(rng, 2 * nb + 2, -(1 << 40), 1 << 40)
    b, absent = pool[:nb], pool[nb:]
    hit = rng.random(np_) < frac
    p = np.where(
        hit,
        b[rng.integers(0, max(nb, 1), np_)] if nb > 0 else 0,
        absent[rng.integers(0, len(absent), np_)],
    ).astype(np.int64)
    return p, b


SIZES = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1]


@pytest.mark.parametrize("np_", SIZES)
@pytest.mark.parametrize("frac", [1.0, 0.0, 0.5])
def test_probe_sizes_and_match_rates(np_, frac):
    rng = np.random.default_rng(1000 * np_ + int(frac * 10))
    p, b = _sides(rng, np_, 300, frac)
    pv = rng.random(np_)
    bw = rng.integers(-5, 5, len(b)).astype(np.int64)
    total = _check(p, b, None, [(PROBE, p), (PROBE, pv), (BUILD, bw)])
    if frac == 1.0:
        assert total == np_
    if frac == 0.0:
        assert total == 0


@pytest.mark.parametrize("np_", [0, 1, CHUNK + 1])
def test_empty_build(np_):
    rng = np.random.default_rng(np_)
    p = rng.integers(-100, 100, np_).astype(np.int64)
    b = np.zeros(0, dtype=np.int64)
    got, total, outs = _run(
        p, b, (4, (PROBE, p), (IMM, 0)),
        [(PROBE, p), (BUILD, np.zeros(0, dtype=np.float64))],
    )
    assert total == 0 and got.shape == (0, 2)
    assert [t.numel() for t in outs[:-1]] == [0, 0]
    assert outs[1].dtype == torch.float64


def test_second_grid_stride_chunk():
    """more chunks than the launch has blocks; matches are sparse (every
    997th key), some of them in the chunks of the second pass"""
    np_ = MAX_GRID * CHUNK + CHUNK + 77
    p = np.arange(np_, dtype=np.int64) - 12345
    b = np.arange(-12345, np_ - 12345, 997, dtype=np.int64)
    b = np.concatenate([b, np.array([np_ - 12345 - 1, np_ + 5], np.int64)])
    b = np.random.default_rng(5).permutation(np.unique(b))
    bw = (b * 3).astype(np.float64)
    edge = int(p[MAX_GRID * CHUNK])  # first row of the second pass
    assert (b >= edge).sum() >= 3 and p[-1] in b
    # the predicate drops the first chunk's rows, so rows of both passes
    # are kept and dropped
    total = _check(
        p, b, (5, (PROBE, p), (IMM, int(p[CHUNK]))), [(PROBE, p), (BUILD, bw)]
    )
    assert total == int(((b >= p[CHUNK]) & (b <= p[-1])).sum())


def test_long_chains_tsize16():
    """40 build keys in 16 slots: chains several links long"""
    rng = np.random.default_rng(16)
    p, b = _sides(rng, CHUNK + 300, 40, 0.7)
    slots = kr.slot_of(b, 16)
    assert np.bincount(slots, minlength=16).max() >= 3
    bw = rng.random(40)
    _check(p, b, None, [(PROBE, p), (BUILD, bw), (BUILD, b)], tsize=16)
    _check(p, b, (2, (BUILD, bw), (IMM, 0.5)), [(PROBE, p), (BUILD, bw)],
           tsize=16)


def test_extreme_and_negative_keys():
    rng = np.random.default_rng(3)
    special = np.array([I64_MIN, I64_MAX, 0, -1, 1, I64_MIN + 1, I64_MAX - 1],
                       dtype=np.int64)
    b = np.concatenate([special[:5], _distinct(rng, 200, I64_MIN, -1)])
    b = rng.permutation(np.unique(b))
    p = np.concatenate([special, b[:120], _distinct(rng, 150)])
    p = rng.permutation(p)
    _check(p, b, None, [(PROBE, p), (BUILD, b)])
    got, total, _ = _run(p, b, None, [(PROBE, p), (BUILD, b)])
    np.testing.assert_array_equal(got[:, 0], got[:, 1])
    for k in special[:5]:
        assert k in got[:, 0]
    for k in special[5:]:
        assert k not in got[:, 0]


def _pred_fixture():
    """every probe row matches; value columns on both sides"""
    rng = np.random.default_rng(77)
    n, nb = CHUNK + 129, 257
    b = _distinct(rng, nb, -(1 << 30), 1 << 30)
    p = b[rng.integers(0, nb, n)]
    big = (1 << 53) + 1  # 2^53 and 2^53 + 1 are one value in float64
    cols = dict(
        pi=rng.integers(-3, 4, n).astype(np.int64),
        pj=rng.integers(-3, 4, n).astype(np.int64),
        bi=rng.integers(-3, 4, nb).astype(np.int64),
        pbig=(big + rng.integers(-1, 2, n)).astype(np.int64),
        bbig=(big + rng.integers(-1, 2, nb)).astype(np.int64),
        pf=np.round(rng.random(n) * 6 - 3),
        pg=np.round(rng.random(n) * 6 - 3),
        bf=np.round(rng.random(nb) * 6 - 3),
    )
    pn, bn = cols["pf"].copy(), cols["bf"].copy()
    pn[::7] = np.nan
    bn[::5] = np.nan
    cols.update(pnan=pn, bnan=bn)
    return p, b, cols


_PRED_CASES = {
    # int64 with int64, exact
    "ii_probe_probe": ((PROBE, "pi"), (PROBE, "pj")),
    "ii_probe_build": ((PROBE, "pi"), (BUILD, "bi")),
    "ii_build_imm": ((BUILD, "bi"), (IMM, 1)),
    "ii_big_probe_build": ((PROBE, "pbig"), (BUILD, "bbig")),
    "ii_big_build_imm": ((BUILD, "bbig"), (IMM, (1 << 53) + 1)),
    # float64 with float64
    "ff_probe_probe": ((PROBE, "pf"), (PROBE, "pg")),
    "ff_probe_build": ((PROBE, "pf"), (BUILD, "bf")),
    "ff_build_imm": ((BUILD, "bf"), (IMM, 1.0)),
    # mixed, compared in float64
    "if_probe_build": ((PROBE, "pi"), (BUILD, "bf")),
    "fi_probe_probe": ((PROBE, "pf"), (PROBE, "pi")),
    "if_build_imm": ((BUILD, "bi"), (IMM, 0.5)),
    "fi_build_imm": ((BUILD, "bf"), (IMM, 1)),
    "imm_left": ((IMM, 0), (PROBE, "pi")),
    # a NaN on either side
    "nan_left": ((PROBE, "pnan"), (BUILD, "bf")),
    "nan_right": ((PROBE, "pf"), (BUILD, "bnan")),
    "nan_both": ((PROBE, "pnan"), (BUILD, "bnan")),
    "nan_int": ((BUILD, "bnan"), (PROBE, "pi")),
    "nan_imm": ((PROBE, "pf"), (IMM, float("nan"))),
}


@pytest.fixture(scope="module")
def pred_data():
    return _pred_fixture()


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("case", sorted(_PRED_CASES))
def test_predicate_matrix(pred_data, case, op):
    p, b, cols = pred_data
    lhs, rhs = _PRED_CASES[case]

    def _resolve(spec):
        return spec if spec[0] == IMM else (spec[0], cols[spec[1]])

    pred = (op, _resolve(lhs), _resolve(rhs))
    rowid = np.arange(len(p), dtype=np.int64)
    total = _check(p, b, pred, [(PROBE, rowid), (BUILD, b)])
    if case.startswith("nan") and op != 1:
        # IEEE, as cmp_col_kernel: a NaN operand fails all but !=
        m = jr.match_index(p, b)
        a = pred[1][1] if pred[1][0] == IMM else (
            pred[1][1] if pred[1][0] == PROBE else pred[1][1][m])
        c = pred[2][1] if pred[2][0] == IMM else (
            pred[2][1] if pred[2][0] == PROBE else pred[2][1][m])
        nan_rows = np.isnan(np.asarray(a, dtype=np.float64)) | np.isnan(
            np.asarray(c, dtype=np.float64))
        assert total <= int((~np.broadcast_to(nan_rows, (len(p),))).sum())


def test_big_ints_are_not_merged():
    """2^53 and 2^53 + 1 differ as int64 and are equal as float64"""
    b = np.arange(10, dtype=np.int64)
    p = np.arange(10, dtype=np.int64)
    x = np.full(10, 1 << 53, dtype=np.int64)
    y = np.full(10, (1 << 53) + 1, dtype=np.int64)
    rowid = np.arange(10, dtype=np.int64)
    assert _check(p, b, (0, (PROBE, x), (BUILD, y)), [(PROBE, rowid)]) == 0
    assert _check(p, b, (2, (PROBE, x), (BUILD, y)), [(PROBE, rowid)]) == 10
    # mixed goes through float64, where they are one value
    yf = y.astype(np.float64)
    assert _check(p, b, (0, (PROBE, x), (BUILD, yf)), [(PROBE, rowid)]) == 10


@pytest.mark.parametrize("ncols", [1, 4, 8])
def test_projection_widths(ncols):
    rng = np.random.default_rng(ncols)
    p, b = _sides(rng, CHUNK + 500, 700, 0.6)
    pcols = [p, rng.random(len(p)), rng.integers(-9, 9, len(p)).astype(np.int64),
             np.arange(len(p), dtype=np.int64)]
    bcols = [rng.random(len(b)), b, rng.integers(-9, 9, len(b)).astype(np.int64),
             np.arange(len(b)).astype(np.float64)]
    specs = []
    for c in range(ncols):
        specs.append((BUILD, bcols[c // 2]) if c % 2 else (PROBE, pcols[c // 2]))
    if ncols == 1:
        _check(p, b, None, [(BUILD, bcols[0])])
    _check(p, b, None, specs)
    _check(p, b, (4, (PROBE, pcols[1]), (BUILD, bcols[0])), specs)


def test_binding_rejects_bad_arguments():
    ext = get_ext()
    b = _dev(np.arange(8, dtype=np.int64))
    p = _dev(np.arange(8, dtype=np.int64))
    heads, nxt, _ = ext.join_build(b, 16)
    ok = [(PROBE, p)]
    with pytest.raises(RuntimeError):  # nine columns
        ext.join_unique_select(p, b, heads, nxt, None, ok * 9)
    with pytest.raises(RuntimeError):  # no column
        ext.join_unique_select(p, b, heads, nxt, None, [])
    with pytest.raises(RuntimeError):  # 4-byte column
        ext.join_unique_select(p, b, heads, nxt, None, [(PROBE, p.to(torch.int32))])
    with pytest.raises(RuntimeError):  # host tensor
        ext.join_unique_select(p, b, heads, nxt, None, [(PROBE, p.cpu())])
    with pytest.raises(RuntimeError):  # not contiguous
        ext.join_unique_select(p, b, heads, nxt, None,
                               [(PROBE, torch.stack([p, p], 1)[:, 0])])
    with pytest.raises(RuntimeError):  # wrong length for its side
        ext.join_unique_select(p, b, heads, nxt, None, [(BUILD, p[:5].clone())])
    with pytest.raises(RuntimeError):  # int32 keys
        ext.join_unique_select(p.to(torch.int32), b, heads, nxt, None, ok)
    with pytest.raises(RuntimeError):  # table length not a power of two
        ext.join_unique_select(p, b, heads[:12].clone(), nxt, None, ok)
    with pytest.raises(RuntimeError):  # op code
        ext.join_unique_select(p, b, heads, nxt, (6, (PROBE, p), (IMM, 1)), ok)
    with pytest.raises(RuntimeError):  # float32 predicate column
        ext.join_unique_select(
            p, b, heads, nxt, (0, (PROBE, p.to(torch.float32)), (IMM, 1)), ok)
