"""GPU tests of the join kernel family (``join.hip``) and of
``gb_mark_reps``, called through ``get_ext()`` and compared with the
plain numpy references of ``kernel_refs.py``: the multiset of (probe,
build) row pairs with equal keys (and equal second hashes when given).
Cursor-based kernels are compared as sorted pair sets, positional ones
element-wise; everything is exact.

``W`` is the most threads a ``grid_for(n)`` launch starts, so ``W + 77``
rows make a grid-stride loop iterate a second time with a ragged final
wave.  No test builds an unbounded chain: every table comes from
``join_build`` and every walk ends at the chain's -1."""
import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

import kernel_refs as kr
import fugue_amd.api as fa
from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine
from fugue_amd.hip.ext import get_ext

W = 8192 * 256
I64_MIN, I64_MAX = kr.INT64_MIN, kr.INT64_MAX
SPECIAL = [I64_MIN, I64_MAX, 0, -1]


def _dev(a, dtype=np.int64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _host(t):
    return t.cpu().numpy()


def _tsize(nb: int) -> int:
    return dops._next_pow2(max(16, nb * 2))


def _build(b: np.ndarray):
    tsize = _tsize(len(b))
    heads, nxt, dup = get_ext().join_build(_dev(b), tsize)
    return heads, nxt, dup, tsize


def _distinct(rng, n: int, exclude=()) -> np.ndarray:
    """n distinct random int64 values, none of them in ``exclude``."""
    v = np.unique(rng.integers(I64_MIN, I64_MAX, 2 * n + 16, dtype=np.int64))
    v = np.setdiff1d(v, np.asarray(list(exclude), dtype=np.int64))
    return rng.permutation(v)[:n]


# ------------------------------------------------------------------ #
# 1. join_build                                                       #
# ------------------------------------------------------------------ #


def _check_chains(keys: np.ndarray, heads, nxt, tsize: int) -> None:
    """Every row is reached exactly once from its key's home slot and
    every walk ends within n steps."""
    n = len(keys)
    heads, nxt = _host(heads).astype(np.int64), _host(nxt).astype(np.int64)
    assert heads.shape == (tsize,)
    home = kr.slot_of(keys, tsize)
    seen = np.zeros(n, dtype=np.int64)
    slots = np.flatnonzero(heads >= 0)
    cur = heads[slots]
    steps = 0
    while len(cur) > 0:
        steps += 1
        assert steps <= n, "a chain is longer than the build side"
        assert cur.min() >= 0 and cur.max() < n
        np.testing.assert_array_equal(home[cur], slots)
        seen += np.bincount(cur, minlength=n)
        cur = nxt[cur]
        live = cur >= 0
        assert (cur[~live] == -1).all()
        cur, slots = cur[live], slots[live]
    np.testing.assert_array_equal(seen, np.ones(n, dtype=np.int64))


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_join_build_chains(n):
    rng = np.random.default_rng(n)
    keys = _distinct(rng, n, SPECIAL)
    keys[: min(n, 4)] = SPECIAL[: min(n, 4)]
    heads, nxt, dup, tsize = _build(keys)
    _check_chains(keys, heads, nxt, tsize)
    assert int(dup.item()) == 0
    if n >= 2:
        # one duplicated key, far from its twin
        keys2 = keys.copy()
        keys2[n - 1] = keys2[0]
        heads, nxt, dup, tsize = _build(keys2)
        _check_chains(keys2, heads, nxt, tsize)
        assert int(dup.item()) != 0
        # all keys equal: one chain holds every row
        keys3 = np.full(n, 42, dtype=np.int64)
        heads, nxt, dup, tsize = _build(keys3)
        _check_chains(keys3, heads, nxt, tsize)
        assert int(dup.item()) != 0
        assert int((_host(heads) >= 0).sum()) == 1


def test_join_build_dup_inside_shared_chain():
    """A duplicate pair whose chain also holds other keys, and the same
    chain without the duplicate."""
    nb = 40
    tsize = _tsize(nb)
    cand = np.arange(1, 20000, dtype=np.int64)
    slot = kr.slot_of(cand, tsize)
    same = cand[slot == slot[0]][:5]  # five distinct keys, one slot
    assert len(same) == 5
    rest = cand[slot != slot[0]][: nb - 6]
    clean = np.concatenate([same, rest[: nb - 5]])
    heads, nxt, dup = get_ext().join_build(_dev(clean), tsize)
    _check_chains(clean, heads, nxt, tsize)
    assert int(dup.item()) == 0
    dirty = np.concatenate([same[:3], rest, same[3:], same[1:2]])
    assert len(dirty) == nb
    heads, nxt, dup = get_ext().join_build(_dev(dirty), tsize)
    _check_chains(dirty, heads, nxt, tsize)
    assert int(dup.item()) != 0


def test_join_build_empty_and_large():
    heads, nxt, dup = get_ext().join_build(_dev(np.empty(0)), 16)
    np.testing.assert_array_equal(_host(heads), np.full(16, -1))
    assert int(dup.item()) == 0
    n = W + 77  # the build and dup-check loops iterate twice
    keys = np.arange(n, dtype=np.int64) * 7919 - 12345
    heads, nxt, dup, tsize = _build(keys)
    _check_chains(keys, heads, nxt, tsize)
    assert int(dup.item()) == 0


# ------------------------------------------------------------------ #
# 2. join_count / join_emit / join_pairs / join_mark_build            #
# ------------------------------------------------------------------ #


def _dup_case(n_probe: int, seed: int = 11):
    """Build of 3000 rows with key multiplicities 1..5; probe rows half
    present, half absent; the special keys on both sides."""
    rng = np.random.default_rng(seed)
    base = np.concatenate(
        [np.array(SPECIAL, dtype=np.int64), _distinct(rng, 1100, SPECIAL)]
    )
    mult = np.arange(len(base)) % 5 + 1
    b = rng.permutation(np.repeat(base, mult))[:3000]
    absent = _distinct(rng, n_probe, base)
    p = np.where(
        rng.random(n_probe) < 0.5, rng.choice(base, n_probe), absent
    ).astype(np.int64)
    p[:4] = SPECIAL
    return p, b


def _check_pairs(got_p, got_b, p, b, mode, p2=None, b2=None):
    """Sorted pair set against the reference; semi may report any
    matching build row."""
    gp, gb = _host(got_p), _host(got_b)
    ep, eb = kr.join_pairs_ref(p, b, mode, p2, b2)
    assert len(gp) == len(ep) == len(gb)
    if mode == 2:
        o = np.argsort(gp, kind="stable")
        np.testing.assert_array_equal(gp[o], ep)
        assert len(gb) == 0 or (gb.min() >= 0 and gb.max() < len(b))
        np.testing.assert_array_equal(b[gb], p[gp])
        if p2 is not None:
            np.testing.assert_array_equal(b2[gb], p2[gp])
        return
    np.testing.assert_array_equal(kr.sorted_pairs(gp, gb), kr.sorted_pairs(ep, eb))


def _count_emit_pairs(p, b, p2=None, b2=None):
    ext = get_ext()
    heads, nxt, dup, tsize = _build(b)
    dp, db = _dev(p), _dev(b)
    d2 = (None, None) if p2 is None else (_dev(p2), _dev(b2))
    cnt = kr.match_counts(p, b, p2, b2)
    got = ext.join_count(dp, db, d2[0], d2[1], heads, nxt, tsize)
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(_host(got), cnt)
    for mode in range(4):
        oc = kr.out_counts(cnt, mode)
        offsets = np.cumsum(oc) - oc
        total = int(oc.sum())
        op, ob = ext.join_emit(
            dp, db, d2[0], d2[1], heads, nxt, tsize, _dev(offsets), total,
            mode,
        )
        # positional: probe row i owns [offsets[i], offsets[i] + oc[i])
        np.testing.assert_array_equal(
            _host(op), np.repeat(np.arange(len(p), dtype=np.int64), oc)
        )
        _check_pairs(op, ob, p, b, mode, p2, b2)
        pp, pb = ext.join_pairs(dp, db, d2[0], d2[1], heads, nxt, tsize, mode)
        assert pp.numel() == total
        _check_pairs(pp, pb, p, b, mode, p2, b2)
    marked = ext.join_mark_build(
        dp, db, d2[0], d2[1], heads, nxt, tsize, len(b)
    )
    _, lo, hi = kr.match_ranges(b, p, b2, p2)
    np.testing.assert_array_equal(_host(marked), hi > lo)


@pytest.mark.parametrize("n_probe", [4097, 16 * 256 * 3 + 5])
def test_join_count_emit_pairs_mark(n_probe):
    p, b = _dup_case(n_probe)
    _count_emit_pairs(p, b)


def test_join_empty_sides():
    ext = get_ext()
    e = np.empty(0, dtype=np.int64)
    p, b = _dup_case(300)
    # empty probe
    heads, nxt, dup, tsize = _build(b)
    assert ext.join_count(_dev(e), _dev(b), None, None, heads, nxt, tsize).numel() == 0
    for mode in range(4):
        pp, pb = ext.join_pairs(_dev(e), _dev(b), None, None, heads, nxt, tsize, mode)
        assert pp.numel() == 0 and pb.numel() == 0
        op, ob = ext.join_emit(
            _dev(e), _dev(b), None, None, heads, nxt, tsize, _dev(e), 0, mode
        )
        assert op.numel() == 0 and ob.numel() == 0
        pi, bi, cur, _m = ext.join_emit_unique(
            _dev(e), _dev(b), None, None, heads, nxt, mode, True, True, False
        )
        assert bi.numel() == 0 and int(cur.item()) == 0
    marked = ext.join_mark_build(_dev(e), _dev(b), None, None, heads, nxt, tsize, len(b))
    assert not bool(_host(marked).any())
    # empty build: every probe row is unmatched
    heads, nxt, dup, tsize = _build(e)
    cnt = ext.join_count(_dev(p), _dev(e), None, None, heads, nxt, tsize)
    assert not bool(_host(cnt).any())
    for mode in range(4):
        pp, pb = ext.join_pairs(_dev(p), _dev(e), None, None, heads, nxt, tsize, mode)
        _check_pairs(pp, pb, p, e, mode)
        oc = kr.out_counts(np.zeros(len(p), dtype=np.int64), mode)
        op, ob = ext.join_emit(
            _dev(p), _dev(e), None, None, heads, nxt, tsize,
            _dev(np.cumsum(oc) - oc), int(oc.sum()), mode,
        )
        _check_pairs(op, ob, p, e, mode)
    for how, mode in (("inner", 0), ("left", 1), ("semi", 2), ("anti", 3)):
        gp, gb = dops.hash_join_indices(_dev(p), _dev(e), how)
        _check_pairs(gp, gb, p, e, mode)
        gp, gb = dops.hash_join_indices(_dev(e), _dev(b), how)
        assert gp.numel() == 0 and gb.numel() == 0


# ------------------------------------------------------------------ #
# 3. join_emit_unique                                                 #
# ------------------------------------------------------------------ #


def _unique_case(n_probe: int, nb: int = 2000, seed: int = 3):
    rng = np.random.default_rng(seed)
    b = np.concatenate(
        [np.array(SPECIAL[:2], dtype=np.int64), _distinct(rng, nb - 2, SPECIAL)]
    )
    absent = np.concatenate(
        [np.array(SPECIAL[2:], dtype=np.int64), _distinct(rng, 64, list(b) + SPECIAL)]
    )
    p = np.where(
        rng.random(n_probe) < 0.5, rng.choice(b, n_probe), rng.choice(absent, n_probe)
    ).astype(np.int64)
    return p, b


def _positional_ref(p, b, p2=None, b2=None) -> np.ndarray:
    order, lo, hi = kr.match_ranges(p, b, p2, b2)
    assert ((hi - lo) <= 1).all()
    bi = np.full(len(p), -1, dtype=np.int64)
    m = hi > lo
    bi[m] = order[lo[m]]
    return bi


def _check_positional(out_pi, out_bi, out_mask, ref_bi, want_pi, want_mask, neg):
    n = len(ref_bi)
    np.testing.assert_array_equal(_host(out_bi), ref_bi)
    if want_pi:
        np.testing.assert_array_equal(_host(out_pi), np.arange(n))
    else:
        assert out_pi.numel() == 0
    if want_mask:
        assert out_mask.dtype == torch.bool
        exp = ref_bi < 0 if neg else ref_bi >= 0
        np.testing.assert_array_equal(_host(out_mask), exp)
    else:
        assert out_mask.numel() == 0


@pytest.mark.parametrize("n_probe", [1, 3, 1023, 1025, 4099])
def test_join_emit_unique_positional(n_probe):
    p, b = _unique_case(n_probe)
    heads, nxt, dup, tsize = _build(b)
    assert int(dup.item()) == 0
    ref = _positional_ref(p, b)
    if n_probe >= 1023:
        assert (ref >= 0).any() and (ref < 0).any()
    for want_pi in (False, True):
        for want_mask in (False, True):
            for neg in (False, True):
                pi, bi, _cur, mask = get_ext().join_emit_unique(
                    _dev(p), _dev(b), None, None, heads, nxt, 1,
                    want_pi, want_mask, neg,
                )
                _check_positional(pi, bi, mask, ref, want_pi, want_mask, neg)


def _check_cursor_modes(p, b, heads, nxt, p2=None, b2=None):
    d2 = (None, None) if p2 is None else (_dev(p2), _dev(b2))
    for mode in (0, 2, 3):
        pi, bi, cur, _m = get_ext().join_emit_unique(
            _dev(p), _dev(b), d2[0], d2[1], heads, nxt, mode, True, False,
            False,
        )
        ep, eb = kr.join_pairs_ref(p, b, mode, p2, b2)
        total = int(cur.item())
        assert total == len(ep), (mode, total, len(ep))
        # rows past the cursor are unspecified
        np.testing.assert_array_equal(
            kr.sorted_pairs(_host(pi)[:total], _host(bi)[:total]),
            kr.sorted_pairs(ep, eb),
        )


@pytest.mark.parametrize("n_probe", [1, 63, 65, 4099])
def test_join_emit_unique_cursor(n_probe):
    p, b = _unique_case(n_probe)
    heads, nxt, dup, tsize = _build(b)
    _check_cursor_modes(p, b, heads, nxt)


def test_join_emit_unique_cursor_second_grid_pass():
    """W + 77 probe rows: the ballot/shuffle reservation runs in a second
    loop iteration whose last wave is partly past the end."""
    p, b = _unique_case(W + 77)
    heads, nxt, dup, tsize = _build(b)
    _check_cursor_modes(p, b, heads, nxt)


# ------------------------------------------------------------------ #
# 4. second-hash (h2) verification                                    #
# ------------------------------------------------------------------ #


def test_join_h2_shared_h1():
    """Build rows that share h1 with a probe row but differ in h2 never
    match; with three build rows on one h1 and a probe row for each of
    their h2 values, at least two matches sit behind a non-matching row
    of the same h1 in the chain."""
    b = np.array([10, 10, 10, 20, 30, 30, 50], dtype=np.int64)
    b2 = np.array([1, 2, 3, 1, 5, 6, 7], dtype=np.int64)
    p = np.array([10, 10, 10, 10, 20, 20, 30, 40, 50, 50], dtype=np.int64)
    p2 = np.array([1, 2, 3, 9, 1, 2, 6, 1, 7, 8], dtype=np.int64)
    cnt = kr.match_counts(p, b, p2, b2)
    assert cnt.tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 1, 0]
    _count_emit_pairs(p, b, p2, b2)
    # many-to-many on (h1, h2) with plenty of h1-only collisions
    rng = np.random.default_rng(8)
    b = rng.integers(0, 100, 500).astype(np.int64)
    b2 = rng.integers(0, 3, 500).astype(np.int64)
    p = rng.integers(0, 130, 700).astype(np.int64)
    p2 = rng.integers(0, 4, 700).astype(np.int64)
    assert (kr.match_counts(p, b) > kr.match_counts(p, b, p2, b2)).any()
    _count_emit_pairs(p, b, p2, b2)


def test_join_h2_unique_h1():
    """Unique-build kernels with h2: an equal h1 with another h2 is no
    match, positionally and through the cursor."""
    rng = np.random.default_rng(9)
    nb, n_probe = 600, 1025
    b = _distinct(rng, nb)
    b2 = rng.integers(0, 2**40, nb).astype(np.int64)
    pick = rng.integers(0, nb, n_probe)
    p = b[pick].copy()
    p2 = b2[pick].copy()
    wrong = rng.random(n_probe) < 0.4
    p2[wrong] += 1
    absent = rng.random(n_probe) < 0.1
    p[absent] = _distinct(rng, n_probe, b)[absent]
    heads, nxt, dup, tsize = _build(b)
    assert int(dup.item()) == 0
    ref = _positional_ref(p, b, p2, b2)
    assert (ref[wrong] == -1).all() and (ref >= 0).any()
    for neg in (False, True):
        pi, bi, _cur, mask = get_ext().join_emit_unique(
            _dev(p), _dev(b), _dev(p2), _dev(b2), heads, nxt, 1, True, True,
            neg,
        )
        _check_positional(pi, bi, mask, ref, True, True, neg)
    _check_cursor_modes(p, b, heads, nxt, p2, b2)


# ------------------------------------------------------------------ #
# 5. gb_mark_reps                                                     #
# ------------------------------------------------------------------ #


def _h2_of(h1: np.ndarray) -> np.ndarray:
    return (kr.mix64(h1 ^ np.int64(0x5BD1E995)) >> np.uint64(1)).astype(np.int64)


def _mark_reps(h1: np.ndarray, h2: np.ndarray):
    ext = get_ext()
    n = len(h1)
    distinct = len(np.unique(h1))
    tsize = dops._next_pow2(max(16, distinct * 2))
    vals = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    ops = torch.tensor([dops.AGG_COUNT], dtype=torch.int32, device="cuda")
    tkeys, _g, _c = ext.gb_aggregate(_dev(h1), vals, None, ops, tsize, True)
    rep, th2, conflict = ext.gb_mark_reps(_dev(h1), _dev(h2), tkeys, tsize)
    return _host(tkeys), _host(rep), _host(th2), int(conflict.item())


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_gb_mark_reps_clean_and_conflict(n, monkeypatch):
    """Only keys present in the table are fed, and neither hash takes the
    reserved empty-slot value: the kernel's probe loop has no exit for
    an absent key, and GB_EMPTY marks an unset h2."""
    rng = np.random.default_rng(n)
    base = _distinct(rng, max(1, n // 3), [I64_MIN])
    h1 = rng.choice(base, n).astype(np.int64)
    h2 = _h2_of(h1)
    tkeys, rep, th2, conflict = _mark_reps(h1, h2)
    assert conflict == 0
    used = tkeys != dops.GB_EMPTY
    np.testing.assert_array_equal(np.sort(tkeys[used]), np.unique(h1))
    assert (rep[~used] == -1).all()
    assert (th2[~used] == dops.GB_EMPTY).all()
    r = rep[used]
    assert r.min() >= 0 and r.max() < n
    np.testing.assert_array_equal(h1[r], tkeys[used])
    np.testing.assert_array_equal(th2[used], _h2_of(tkeys[used]))
    reps = _host(dops.distinct_reps(_dev(h1), _dev(h2)))
    np.testing.assert_array_equal(np.sort(h1[reps]), np.unique(h1))
    if n < 2:
        return
    # one row keeps its h1 and changes its h2: an h1 collision
    bad = h2.copy()
    twin = np.flatnonzero(h1 == h1[0])
    if len(twin) < 2:
        h1 = h1.copy()
        h1[1] = h1[0]
        bad[1] = bad[0]
    bad[0] ^= 1
    _t, _r, _th, conflict = _mark_reps(h1, bad)
    assert conflict > 0
    with pytest.raises(dops.HashCollisionError):
        dops.distinct_reps(_dev(h1), _dev(bad))
    import pyarrow as pa

    from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
    from fugue_amd.schema import Schema

    df = HipDataFrame.from_columns(
        {
            "k": DeviceColumn(_dev(h1), None, pa.int64()),
            "v": DeviceColumn(
                torch.ones(n, dtype=torch.float64, device="cuda"), None,
                pa.float64(),
            ),
        },
        Schema("k:long,v:double"),
        "cuda:0",
    )
    d1, d2 = _dev(h1), _dev(bad)
    monkeypatch.setattr(
        dops, "hash_rows", lambda cols, seed=None: d1 if seed is None else d2
    )
    with pytest.raises(dops.HashCollisionError):
        dops.groupby_aggregate_hashed(df, ["k"], [("v", dops.AGG_SUM, "s")])


# ------------------------------------------------------------------ #
# 6. join_open_unique                                                 #
# ------------------------------------------------------------------ #


def _oa(p, b, want_pi, want_mask, neg):
    return get_ext().join_open_unique(_dev(p), _dev(b), want_pi, want_mask, neg)


@pytest.mark.parametrize("n_probe", [1, 3, 1023, 1025, 4099])
def test_join_open_unique_positional(n_probe):
    p, b = _unique_case(n_probe)
    # the open-addressed table reserves INT64_MIN: keep it out of the build
    b = b[b != I64_MIN]
    ref = _positional_ref(p, b)
    for want_pi in (False, True):
        for want_mask in (False, True):
            for neg in (False, True):
                pi, bi, mask, flags = _oa(p, b, want_pi, want_mask, neg)
                assert _host(flags).tolist() == [0, 0]
                _check_positional(pi, bi, mask, ref, want_pi, want_mask, neg)


def _wrapping_keys(nb: int) -> np.ndarray:
    """nb distinct keys whose home slots in a 16-slot table are 14 and
    15, so linear probing runs past the table's end."""
    cand = np.arange(1, 4000, dtype=np.int64)
    s = kr.slot_of(cand, 16)
    return np.concatenate([cand[s == 15][: nb - nb // 2], cand[s == 14][: nb // 2]])


@pytest.mark.parametrize("nb", [0, 1, 8])
def test_join_open_unique_small_tables(nb):
    b = _wrapping_keys(nb)
    assert len(b) == nb
    cand = np.arange(4000, 8000, dtype=np.int64)
    s = kr.slot_of(cand, 16)
    absent = np.concatenate([cand[s == 15][:3], cand[s == 14][:3], cand[s == 3][:3]])
    p = np.concatenate([b, absent, b[::-1], np.array([0, -1, I64_MAX])]).astype(np.int64)
    ref = _positional_ref(p, b)
    for neg in (False, True):
        pi, bi, mask, flags = _oa(p, b, True, True, neg)
        assert _host(flags).tolist() == [0, 0]
        _check_positional(pi, bi, mask, ref, True, True, neg)
    pi, bi, mask, flags = _oa(np.empty(0, dtype=np.int64), b, True, True, False)
    assert bi.numel() == 0 and pi.numel() == 0 and mask.numel() == 0


def test_join_open_unique_flags():
    p = np.array([1, 2, 3], dtype=np.int64)
    _pi, _bi, _m, flags = _oa(p, np.array([5, 6, 5, 7], dtype=np.int64), False, False, False)
    f = _host(flags)
    assert f[0] != 0 and f[1] == 0
    _pi, _bi, _m, flags = _oa(p, np.array([5, I64_MIN, 7], dtype=np.int64), False, False, False)
    f = _host(flags)
    assert f[0] == 0 and f[1] != 0


@pytest.mark.parametrize("nb", [0, 3, 2000])
def test_join_open_unique_sentinel_probe_key(nb):
    """INT64_MIN only on the probe side is an ordinary absent key: no
    flag, no match.  (The table marks empty slots with that value; a
    probe for it must not take an empty slot for a hit.)"""
    rng = np.random.default_rng(nb)
    b = _distinct(rng, nb, [I64_MIN])
    p = np.concatenate([b[: nb // 2], _distinct(rng, 40, list(b))])
    p = np.concatenate([[I64_MIN], p, [I64_MIN] * 5]).astype(np.int64)
    p[len(p) // 2] = I64_MIN
    ref = _positional_ref(p, b)
    assert (ref[p == I64_MIN] == -1).all()
    for neg in (False, True):
        pi, bi, mask, flags = _oa(p, b, True, True, neg)
        assert _host(flags).tolist() == [0, 0]
        _check_positional(pi, bi, mask, ref, True, True, neg)


# ------------------------------------------------------------------ #
# 7. engine level                                                     #
# ------------------------------------------------------------------ #


@pytest.mark.parametrize("how", ["inner", "left_outer", "semi", "anti"])
def test_open_addressed_join_sentinel_left_only(how, monkeypatch):
    """fa.join through the open-addressed path with INT64_MIN in the left
    frame only: the build side raises no flag, so the result comes from
    the open-addressed probe itself."""
    monkeypatch.setenv("FUGUE_JOIN_OA", "1")
    engine = HipExecutionEngine()
    rng = np.random.default_rng(41)
    n = 5000
    k = rng.integers(0, 3000, n).astype(np.int64)
    k[rng.random(n) < 0.02] = I64_MIN
    k[0] = k[n - 1] = I64_MIN
    left = pd.DataFrame(dict(k=k, v=rng.random(n)))
    right = pd.DataFrame(dict(k=np.arange(0, 4000, 2, dtype=np.int64), w=rng.random(2000)))
    got = (
        fa.join(left, right, how=how, engine=engine, as_fugue=True)
        .as_pandas().sort_values(["k", "v"]).reset_index(drop=True)
    )
    if how == "inner":
        exp = left.merge(right, on="k", how="inner")
    elif how == "left_outer":
        exp = left.merge(right, on="k", how="left")
    elif how == "semi":
        exp = left[left.k.isin(right.k)]
    else:
        exp = left[~left.k.isin(right.k)]
    exp = exp.sort_values(["k", "v"]).reset_index(drop=True)
    assert len(exp) > 0
    pd.testing.assert_frame_equal(got, exp, check_dtype=False)
