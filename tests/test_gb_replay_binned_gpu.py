"""Binned dense group-by replay: the replayed values are laid out by bins
of M consecutive hash partitions (``FUGUE_GB_REPLAY_BIN_PARTS``), so the
tile scatter's runs are M times longer, and the aggregate walks chunks of
one bin with the bin's first id as its table base.

End-to-end cases aggregate the SAME key tensor four times with fresh
values; calls three and four are replays.  Each asserts that the memo
entry is a ``_DenseLayout`` with the expected ``bin_parts`` and that its
``hits`` advance on calls three and four, so a silent fallback cannot
pass.  Reference: ``scatter_add_`` in fp64 plus ``bincount`` over the
keys' dense codes; keys and counts exact, sums within ``rtol=1e-12``
(atomic order varies).  The direct kernel cases compare on the CPU."""
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


def _reference(keys):
    """(uniq, inv, counts) of the key tensor: computed once per case and
    shared by every knob setting run over it."""
    uniq, inv = torch.unique(keys, return_inverse=True)
    return uniq, inv, torch.bincount(inv, minlength=uniq.numel())


def _run_case(monkeypatch, keys, ref, expected_groups, seed, knob,
              expect_parts):
    """Four aggregations over ``keys`` with the bin knob at ``knob``;
    checks each against the reference, the entry's ``bin_parts`` and that
    calls three and four were replays.  Returns (entry, out_keys,
    out_count) of the last call."""
    monkeypatch.setenv("FUGUE_GB_REPLAY_BIN_PARTS", str(knob))
    monkeypatch.setenv("FUGUE_GB_BIN_SLOTS", "8192")
    dops._LAYOUT_MEMO.clear()
    dops._LAYOUT_SEEN.clear()
    uniq, inv, ref_count = ref
    n = keys.numel()
    g = _gen(seed)
    kcol = DeviceColumn(keys, None, pa.int64())
    ent = out_keys = out_count = None
    for call in range(1, 5):
        vals = torch.rand(n, dtype=torch.float64, device="cuda",
                          generator=g) * 4.0 - 1.0
        out_keys, out_aggs, out_count, _ = _agg(kcol, vals, expected_groups)
        want = torch.zeros(uniq.numel(), dtype=torch.float64, device="cuda")
        want.scatter_add_(0, inv, vals)
        perm = torch.argsort(out_keys)
        assert torch.equal(out_keys.index_select(0, perm), uniq), call
        assert torch.equal(out_count.index_select(0, perm), ref_count), call
        assert torch.allclose(
            out_aggs["s"].index_select(0, perm), want, rtol=1e-12
        ), call
        if call >= 2:
            ent = _entry(keys)
            assert isinstance(ent, dops._DenseLayout), call
            assert ent.bin_parts == expect_parts, call
            assert ent.hits == call - 2, call
    return ent, out_keys, out_count


def test_binned_replay_end_to_end(monkeypatch):
    keys = torch.randint(0, 200_000, (300_001,), dtype=torch.int64,
                         device="cuda", generator=_gen(11))
    ref = _reference(keys)
    got = {}
    for knob in (1, 4, 8):
        ent, out_keys, out_count = _run_case(
            monkeypatch, keys, ref, 200_000, 12, knob, knob
        )
        got[knob] = (out_keys, out_count)
        if knob > 1:
            nbins = 1024 // knob
            assert ent.bin_offsets.numel() == nbins + 1
            assert ent.bin_group_base.numel() == nbins + 1
            assert ent.bin_chunk_base.numel() == nbins + 1
            assert torch.equal(ent.bin_offsets, ent.offsets[::knob])
            assert torch.equal(ent.bin_group_base, ent.group_base[::knob])
            assert int(ent.bin_chunk_base[-1]) == ent.bin_chunks
    # same groups, counts and output order whatever the value layout
    assert torch.equal(got[1][0], got[8][0])
    assert torch.equal(got[1][1], got[8][1])


def test_binned_replay_bin_width_reduced(monkeypatch):
    """1.95M distinct keys over 1024 partitions, about 1900 each (the
    fullest holds 2039, under the id-assignment limit of 2048).  Eight
    partitions hold about 15200 ids, four about 7600 (7874 at most): with
    an 8192-slot table the width drops from the knob's 8 to 4.

    ``expected_groups`` is 1_100_000 for the reason the declined dense
    test gives: the global table of the first-sight path must hold every
    group, and 1_100_000 still selects 1024 partitions."""
    n = 2_500_000
    perm = torch.randperm(n, device="cuda", generator=_gen(21))
    keys = (perm % 1_950_000).to(torch.int64)
    ref = _reference(keys)
    _run_case(monkeypatch, keys, ref, 1_100_000, 22, 8, 4)
    _run_case(monkeypatch, keys, ref, 1_100_000, 23, 1, 1)


def test_binned_replay_sparse(monkeypatch):
    """300 distinct keys over 128 bins: most bins are empty"""
    pool = torch.randint(0, 1 << 40, (300,), dtype=torch.int64,
                         device="cuda", generator=_gen(31))
    idx = torch.randint(0, 300, (50_000,), device="cuda", generator=_gen(32))
    keys = pool.index_select(0, idx)
    _run_case(monkeypatch, keys, _reference(keys), 200_000, 33, 8, 8)


def test_binned_replay_heavy_hitter(monkeypatch):
    """one key holds half of the rows; n stays small for the reason the
    dense heavy-hitter test gives (the torch reference slows down)"""
    n = 50_001
    keys = torch.randint(0, 200_000, (n,), dtype=torch.int64, device="cuda",
                         generator=_gen(41))
    hot = torch.rand(n, device="cuda", generator=_gen(42)) < 0.5
    keys = torch.where(hot, torch.full_like(keys, 777), keys)
    _run_case(monkeypatch, keys, _reference(keys), 200_000, 43, 8, 8)


def test_binned_replay_smaller_than_a_tile(monkeypatch):
    """n below one scatter tile (and below the partitioned path's usual
    sizes): one partial tile feeds every bin"""
    keys = torch.randint(0, 150_000, (5_000,), dtype=torch.int64,
                         device="cuda", generator=_gen(51))
    _run_case(monkeypatch, keys, _reference(keys), 200_000, 52, 8, 8)


def _hand_layout(n, part_sizes, m, seed):
    """offsets/bin_offsets of hand-built partitions, a random permutation
    as recorded positions and ids that identify the recorded position"""
    assert sum(part_sizes) == n
    offsets = torch.tensor([0] + part_sizes, dtype=torch.int64).cumsum(0)
    bin_offsets = offsets[::m].contiguous()
    pos = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    gid_old = torch.arange(n, dtype=torch.int32) * 7 + 3
    return offsets, bin_offsets, pos.to(torch.int32), gid_old


def _check_layout(pos, gid_old, bin_offsets, tile, rank, dst, gid_new):
    n = pos.numel()
    pos, rank, dst = pos.long(), rank.long() & 0xFFFF, dst.long()
    nbins = bin_offsets.numel() - 1
    assert torch.equal(torch.sort(dst).values, torch.arange(n))
    bin_of_dst = torch.bucketize(dst, bin_offsets, right=True) - 1
    next_free = bin_offsets[:-1].clone()  # runs of a bin are in tile order
    for t0 in range(0, n, tile):
        cnt = min(tile, n - t0)
        d = dst[t0:t0 + cnt]
        b = bin_of_dst[t0:t0 + cnt]
        # ranks are a permutation of the tile; the row ranked r goes to d[r]
        r = rank[t0:t0 + cnt]
        assert torch.equal(torch.sort(r).values, torch.arange(cnt))
        row_dst = d[r]
        old = pos[t0:t0 + cnt]
        # a row stays in the bin of its recorded position: bins in order
        assert torch.equal(
            torch.bucketize(row_dst, bin_offsets, right=True),
            torch.bucketize(old, bin_offsets, right=True),
        )
        assert torch.equal(gid_new[row_dst], gid_old[old])
        # ranks follow the recorded position
        assert torch.equal(torch.argsort(old), torch.argsort(r))
        assert bool((b[1:] >= b[:-1]).all())
        for bb in range(nbins):
            run = d[b == bb]
            if run.numel() == 0:
                continue
            # one ascending contiguous run, adjacent to the previous tile's
            assert torch.equal(
                run, torch.arange(run.numel()) + int(next_free[bb])
            )
            next_free[bb] += run.numel()
    assert torch.equal(next_free, bin_offsets[1:])


def test_binned_layout_property():
    """tile 512, 16 partitions in bins of 4, three tiles and 17 rows"""
    ext = get_ext()
    tile, m = 512, 4
    n = 3 * tile + 17
    sizes = [0, 130, 7, 260, 1, 0, 0, 0, 300, 55, 0, 200, 90, 410, 100, 0]
    offsets, bin_offsets, pos, gid_old = _hand_layout(n, sizes, m, 61)
    rank, dst, gid_new = ext.scatter_tile_prepare_binned(
        pos.cuda(), gid_old.cuda(), bin_offsets.cuda(), tile
    )
    _check_layout(pos, gid_old, bin_offsets, tile, rank.cpu(), dst.cpu(),
                  gid_new.cpu())
    # the scatter places values by the same layout
    vals = torch.randn(n, dtype=torch.float64,
                       generator=torch.Generator().manual_seed(62))
    out = ext.scatter_tile(vals.cuda(), rank, dst, tile).cpu()
    row_dst = torch.empty(n, dtype=torch.long)
    for t0 in range(0, n, tile):
        cnt = min(tile, n - t0)
        row_dst[t0:t0 + cnt] = dst.cpu().long()[t0:t0 + cnt][
            rank.cpu().long()[t0:t0 + cnt] & 0xFFFF]
    want = torch.empty_like(vals)
    want[row_dst] = vals
    assert torch.equal(out, want)


def test_binned_layout_smaller_than_a_tile():
    ext = get_ext()
    tile, m, n = 512, 2, 100
    sizes = [10, 0, 40, 5, 0, 0, 25, 20]
    offsets, bin_offsets, pos, gid_old = _hand_layout(n, sizes, m, 71)
    rank, dst, gid_new = ext.scatter_tile_prepare_binned(
        pos.cuda(), gid_old.cuda(), bin_offsets.cuda(), tile
    )
    _check_layout(pos, gid_old, bin_offsets, tile, rank.cpu(), dst.cpu(),
                  gid_new.cpu())


@pytest.mark.parametrize(
    "slots,chunk", [(2048, 1024), (4096, 16384), (8192, 4096), (8192, 65536)]
)
def test_binned_aggregate_hand_built(slots, chunk):
    """hand-built ids: an empty bin, a bin shorter than one chunk, a bin of
    exactly three chunks, a bin with a final partial chunk, a bin exactly
    as wide as the table and one wider than it, whose ids past the table
    take the global-add branch and must still be exact"""
    ext = get_ext()
    rows = [0, chunk // 2 + 3, 3 * chunk, 2 * chunk + 77, chunk + 1, 0,
            2 * chunk + 5]
    width = [0, 300, 1000, 17, slots, 0, slots + 500]
    bin_offsets = torch.tensor([0] + rows, dtype=torch.int64).cumsum(0)
    bin_group_base = torch.tensor([0] + width, dtype=torch.int64).cumsum(0)
    chunks = [(r + chunk - 1) // chunk for r in rows]
    bin_chunk_base = torch.tensor([0] + chunks, dtype=torch.int64).cumsum(0)
    n, n_groups = sum(rows), sum(width)
    g = torch.Generator().manual_seed(81)
    gid = torch.cat([
        torch.randint(0, w, (r,), generator=g) + int(bin_group_base[b])
        for b, (r, w) in enumerate(zip(rows, width)) if r
    ]).to(torch.int32)
    vals = torch.randn(n, dtype=torch.float64, generator=g)
    out = ext.gb_dense_aggregate_binned(
        gid.cuda(), vals.cuda(), bin_offsets.cuda(), bin_group_base.cuda(),
        bin_chunk_base.cuda(), sum(chunks), n_groups, chunk, slots,
    )
    want = torch.zeros(n_groups, dtype=torch.float64)
    want.index_add_(0, gid.long(), vals)
    assert torch.allclose(out.cpu(), want, rtol=1e-12)


def test_binned_bindings_empty():
    """n = 0 through the new bindings: empty results"""
    ext = get_ext()
    i32 = dict(dtype=torch.int32, device="cuda")
    zeros = torch.zeros(5, dtype=torch.int64, device="cuda")
    rank, dst, gid_new = ext.scatter_tile_prepare_binned(
        torch.empty(0, **i32), torch.empty(0, **i32), zeros, 512
    )
    assert rank.numel() == 0 and dst.numel() == 0 and gid_new.numel() == 0
    assert rank.dtype == torch.int16 and dst.dtype == torch.int32
    assert gid_new.dtype == torch.int32
    vals = torch.empty(0, dtype=torch.float64, device="cuda")
    out = ext.gb_dense_aggregate_binned(
        gid_new, vals, zeros, zeros, zeros, 0, 0, 1024, 8192
    )
    assert out.numel() == 0 and out.dtype == torch.float64
    out = ext.gb_replay_binned(
        vals, gid_new, rank, dst, zeros, zeros, zeros, 0, 0, 1024, 8192, 512
    )
    assert out.numel() == 0 and out.dtype == torch.float64
