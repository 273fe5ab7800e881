"""Dense group-by replay: dense group ids prepared once per key tensor,
tile-coalesced value scatter and the LDS-add aggregate on replayed calls.

Every case aggregates the SAME key tensor four times with fresh values
(negatives included); calls three and four are replays.  Reference:
``scatter_add_`` in fp64 plus ``bincount`` over the keys' dense codes.
Keys and counts must match exactly, sums within ``rtol=1e-12`` (atomic
order varies)."""
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import pyarrow as pa  # noqa: E402

from fugue_amd.hip import ops as dops  # noqa: E402
from fugue_amd.hip.ext import get_ext  # noqa: E402
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame  # noqa: E402
from fugue_amd.schema import Schema  # noqa: E402


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _agg(kcol, vals, expected_groups):
    df = HipDataFrame.from_columns(
        {"k": kcol, "v": DeviceColumn(vals, None, pa.float64())},
        Schema("k:long,v:double"), "cuda",
    )
    return dops.groupby_aggregate(
        df, ["k"], [("v", dops.AGG_SUM, "s")],
        expected_groups=expected_groups,
    )


def _entry(keys):
    ents = [
        e for k, e in dops._LAYOUT_MEMO.items()
        if k[0] == keys.data_ptr() and k[1] == keys.numel()
        and e.ref() is not None
    ]
    assert len(ents) == 1, "expected exactly one layout entry for the keys"
    return ents[0]


def _run_case(keys, expected_groups, seed, expect_dense):
    """Four aggregations over ``keys``; checks each against the reference
    and that calls three and four took (or did not take) the dense path.
    Returns the layout entry."""
    dops._LAYOUT_MEMO.clear()
    dops._LAYOUT_SEEN.clear()
    n = keys.numel()
    g = _gen(seed)
    kcol = DeviceColumn(keys, None, pa.int64())
    uniq, inv = torch.unique(keys, return_inverse=True)
    ref_count = torch.bincount(inv, minlength=uniq.numel())
    ent = None
    for call in range(1, 5):
        vals = torch.rand(n, dtype=torch.float64, device="cuda",
                          generator=g) * 4.0 - 1.0
        out_keys, out_aggs, out_count, _ = _agg(kcol, vals, expected_groups)
        ref = torch.zeros(uniq.numel(), dtype=torch.float64, device="cuda")
        ref.scatter_add_(0, inv, vals)
        perm = torch.argsort(out_keys)
        assert torch.equal(out_keys.index_select(0, perm), uniq), call
        assert torch.equal(out_count.index_select(0, perm), ref_count), call
        assert torch.allclose(
            out_aggs["s"].index_select(0, perm), ref, rtol=1e-12
        ), call
        if call >= 2:
            ent = _entry(keys)
            assert isinstance(ent, dops._DenseLayout) == expect_dense
            hits = ent.hits if expect_dense else 0
            assert hits == (max(0, call - 2) if expect_dense else 0), call
    return ent


def test_dense_replay_base_shape():
    keys = torch.randint(0, 200_000, (300_001,), dtype=torch.int64,
                         device="cuda", generator=_gen(11))
    ent = _run_case(keys, 200_000, 12, True)
    # dense entries drop the cached spill keys
    assert not hasattr(ent, "pkeys")


def test_dense_replay_sparse():
    """300 distinct keys over 1024 partitions: most partitions are empty
    and every aggregate chunk spans many partitions."""
    pool = torch.randint(0, 1 << 40, (300,), dtype=torch.int64,
                         device="cuda", generator=_gen(21))
    idx = torch.randint(0, 300, (50_000,), device="cuda", generator=_gen(22))
    _run_case(pool.index_select(0, idx), 200_000, 23, True)


def test_dense_replay_heavy_hitter():
    """one key holds half of the rows.  n is kept small because the
    reference itself (``scatter_add_``: fp64 global atomics, all of the
    hot key's rows on one address) slows quadratically with the hot
    key's row count — 33 s at n = 300_001, where the aggregation under
    test takes 0.2 ms."""
    n = 50_001
    keys = torch.randint(0, 200_000, (n,), dtype=torch.int64, device="cuda",
                         generator=_gen(31))
    hot = torch.rand(n, device="cuda", generator=_gen(32)) < 0.5
    keys = torch.where(hot, torch.full_like(keys, 777), keys)
    _run_case(keys, 200_000, 33, True)


def test_dense_replay_wide_keys():
    """negative keys and keys >= 2^31: the int64 spill path (narrow == 0)"""
    r = torch.randint(0, 200_000, (300_001,), dtype=torch.int64,
                      device="cuda", generator=_gen(41))
    keys = (r - 100_000) * 3_000_000_019
    assert int(keys.min()) < 0 and int(keys.max()) >= (1 << 31)
    _run_case(keys, 200_000, 42, True)


def test_dense_replay_declined():
    """3M distinct keys over 1024 partitions (~2900 each) overflow the
    id-assignment table: the dense layout is declined and the plain
    replay stays exact.

    ``expected_groups`` is 1_100_000, not smaller: the group-by's global
    hash table holds ``next_pow2(2 * expected_groups)`` slots and its
    insert probes until it finds a free slot, so an estimate whose table
    cannot hold the 3M groups never terminates on any path.  1_100_000
    still selects 1024 partitions and still underestimates the
    cardinality almost threefold."""
    n = 4_000_000
    perm = torch.randperm(n, device="cuda", generator=_gen(51))
    keys = (perm % 3_000_000).to(torch.int64)
    ent = _run_case(keys, 1_100_000, 52, False)
    assert isinstance(ent, dops._PlainLayout) and ent.pkeys is not None


def test_dense_replay_new_key_tensor():
    keys = torch.randint(0, 200_000, (300_001,), dtype=torch.int64,
                         device="cuda", generator=_gen(61))
    ent = _run_case(keys, 200_000, 62, True)
    keys2 = keys.clone()  # equal contents, new address (keys still alive)
    assert keys2.data_ptr() != keys.data_ptr()
    vals = torch.rand(keys.numel(), dtype=torch.float64, device="cuda",
                      generator=_gen(63)) - 0.5
    out_keys, out_aggs, out_count, _ = _agg(
        DeviceColumn(keys2, None, pa.int64()), vals, 200_000
    )
    assert ent.hits == 2  # the old layout was not replayed
    assert out_keys is not ent.out_keys
    uniq, inv = torch.unique(keys2, return_inverse=True)
    ref = torch.zeros(uniq.numel(), dtype=torch.float64, device="cuda")
    ref.scatter_add_(0, inv, vals)
    perm = torch.argsort(out_keys)
    assert torch.equal(out_keys.index_select(0, perm), uniq)
    assert torch.equal(out_count.index_select(0, perm),
                       torch.bincount(inv, minlength=uniq.numel()))
    assert torch.allclose(out_aggs["s"].index_select(0, perm), ref,
                          rtol=1e-12)


def test_dense_replay_gate_off(monkeypatch):
    monkeypatch.setenv("FUGUE_GB_REPLAY_DENSE", "0")
    keys = torch.randint(0, 200_000, (300_001,), dtype=torch.int64,
                         device="cuda", generator=_gen(71))
    ent = _run_case(keys, 200_000, 72, False)
    assert isinstance(ent, dops._PlainLayout) and ent.pkeys is not None
    assert not hasattr(ent, "gid")


@pytest.mark.parametrize("tile", [512, 8192])
def test_scatter_tile_arbitrary_permutation(tile):
    """a pure permutation through the tile scatter is bit-exact; n leaves
    a final partial tile"""
    ext = get_ext()
    n = 20_001
    pos = torch.randperm(n, device="cuda", generator=_gen(81)).to(torch.int32)
    vals = torch.randn(n, dtype=torch.float64, device="cuda",
                       generator=_gen(82))
    rank, dst = ext.scatter_tile_prepare(pos, tile)
    out = ext.scatter_tile(vals, rank, dst, tile)
    ref = torch.empty_like(vals)
    ref[pos.long()] = vals
    assert torch.equal(out, ref)


@pytest.mark.parametrize("chunk,slots", [(1024, 2048), (16384, 4096)])
def test_dense_aggregate_hand_built(chunk, slots):
    """hand-built ids: empty partitions, a chunk smaller than a partition,
    and chunks whose ids run past the LDS table (global-add branch)"""
    ext = get_ext()
    sizes = [0, 5000, 100, 0, 3000, 7001, 1, 2500]
    distinct = [0, 1500, 3, 0, 900, 2000, 1, 700]
    offsets = torch.tensor([0] + sizes, device="cuda").cumsum(0)
    group_base = torch.tensor([0] + distinct, device="cuda").cumsum(0)
    n, n_groups = sum(sizes), sum(distinct)
    g = _gen(91)
    parts = []
    for p, (sz, d) in enumerate(zip(sizes, distinct)):
        if sz:
            parts.append(
                torch.randint(0, d, (sz,), device="cuda", generator=g)
                + int(group_base[p])
            )
    gid = torch.cat(parts).to(torch.int32)
    vals = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    out = ext.gb_dense_aggregate(gid, vals, offsets, group_base, n_groups,
                                 chunk, slots)
    ref = torch.zeros(n_groups, dtype=torch.float64, device="cuda")
    ref.scatter_add_(0, gid.long(), vals)
    assert torch.allclose(out, ref, rtol=1e-12)
