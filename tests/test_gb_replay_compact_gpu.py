"""Compact binned dense replay (``FUGUE_GB_REPLAY_COMPACT``): the binned
value layout without the per-row destination and with 16-bit ids relative
to the bin.  The 10 B/row binned kernels are the reference for the layout:
what is a pure permutation (ranks, placed values, ids) must be bit-equal to
them; sums are checked against a float64 CPU reference within
``rtol=1e-12`` (atomic order varies), counts and keys exactly.

Tile 512 throughout (and one case at the default tile, 8192, the only
one whose LDS passes 64 KB), so three tiles are 1.5K rows.  ``tile_start`` is
``[tiles, B + 1]``: the exclusive row prefix of the (tile, bin) counts and,
last, the tile's placed rows.

The end-to-end cases run at tile 2048 with the default 8 partitions per bin
(128 bins, the most the host rule ``nbins <= tile // 16`` admits there) and
at tile 512 with 32 partitions per bin (32 bins, again the most); tile 512
with 8 partitions per bin has 128 bins and is the fallback case."""
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

TILE = 512


def _u16(t):
    return t.cpu().long() & 0xFFFF


def _hand_ids(pos_bins, widths, seed):
    """bin_group_base of the given id widths and, by recorded position, an
    id inside the bin of that position (first and last id of a bin
    included)"""
    g = torch.Generator().manual_seed(seed)
    bgb = torch.tensor([0] + widths, dtype=torch.int64).cumsum(0)
    w = torch.tensor(widths, dtype=torch.int64)[pos_bins]
    off = (torch.rand(pos_bins.numel(), generator=g, dtype=torch.float64)
           * w).long().clamp_(max=w - 1) if pos_bins.numel() else w
    if pos_bins.numel() > 1:
        off[0] = 0
        off[-1] = w[-1] - 1
    return bgb, (bgb[pos_bins] + off).to(torch.int32)


def _check_against_binned(pos, gid_old, bin_offsets, bgb, tile=TILE,
                          threads=(0, 512)):
    """The compact preparation and scatter against the binned pair on the
    same input; returns the compact outputs (on the GPU)."""
    ext = get_ext()
    n = pos.numel()
    nbins = bin_offsets.numel() - 1
    ntiles = (n + tile - 1) // tile
    dpos, dgid, dbo = pos.cuda(), gid_old.cuda(), bin_offsets.cuda()
    rank0, dst0, gid0 = ext.scatter_tile_prepare_binned(dpos, dgid, dbo, tile)
    rank, rel, tstart, tdelta = ext.scatter_tile_prepare_compact(
        dpos, dgid, dbo, bgb.cuda(), tile
    )
    assert rank.dtype == torch.int16 and rel.dtype == torch.int16
    assert tstart.dtype == torch.int16 and tdelta.dtype == torch.int32
    assert tuple(tstart.shape) == (ntiles, nbins + 1)
    assert tuple(tdelta.shape) == (ntiles, nbins)
    assert torch.equal(rank, rank0)
    # keep_gid: the same four tensors and the binned gid
    kept = ext.scatter_tile_prepare_compact(dpos, dgid, dbo, bgb.cuda(), tile,
                                            True)
    assert len(kept) == 5 and kept[4].dtype == torch.int32
    for i, want in ((0, rank), (2, tstart), (3, tdelta)):
        assert torch.equal(kept[i], want)
    dst0c, gid0c = dst0.cpu().long(), gid0.cpu().long()
    ts, tdl = _u16(tstart), tdelta.cpu().long()
    placed = dst0c >= 0
    # tile_delta[t][b] + r rebuilds the binned dst of every sorted row
    rebuilt = torch.full((n,), -1, dtype=torch.long)
    for t in range(ntiles):
        t0 = t * tile
        cnt = min(tile, n - t0)
        r = torch.arange(cnt)
        assert ts[t, 0] == 0 and bool((ts[t, 1:] >= ts[t, :-1]).all())
        b = torch.bucketize(r, ts[t, :nbins].contiguous(), right=True) - 1
        d = tdl[t, b] + r
        ok = (r < ts[t, nbins]) & (d >= 0) & (d < n)
        rebuilt[t0:t0 + cnt] = torch.where(ok, d, torch.full_like(d, -1))
    assert torch.equal(rebuilt, dst0c)
    # ids: rel == gid_new - bin_group_base[bin], wherever a row was placed
    d = dst0c[placed]
    assert torch.equal(kept[4].cpu().long()[d], gid0c[d])
    # (a destination no row was placed at is left unwritten)
    assert torch.equal(kept[1].cpu()[d], rel.cpu()[d])
    bin_of_d = torch.bucketize(d, bin_offsets, right=True) - 1
    assert torch.equal(_u16(rel)[d], gid0c[d] - bgb[bin_of_d])
    # values: bit-equal to the binned scatter at every placed destination
    vals = torch.randn(n, dtype=torch.float64,
                       generator=torch.Generator().manual_seed(n + nbins))
    want = ext.scatter_tile(vals.cuda(), rank0, dst0, tile)
    for th in threads:
        out = ext.scatter_tile_compact(vals.cuda(), rank, tstart, tdelta,
                                       tile, th)
        if bool(placed.all()):
            assert torch.equal(out, want), th
        else:
            assert torch.equal(out.cpu()[d], want.cpu()[d]), th
    return rank, rel, tstart, tdelta


@pytest.mark.parametrize("nbins", [1, 2, 7])
def test_compact_layout_equivalence(nbins):
    """two tiles and a partial third, a random permutation, random bin
    boundaries"""
    n = 2 * TILE + 37
    g = torch.Generator().manual_seed(100 + nbins)
    cuts = torch.sort(torch.randint(0, n + 1, (nbins - 1,), generator=g))
    bin_offsets = torch.cat([torch.tensor([0]), cuts.values,
                             torch.tensor([n])]).to(torch.int64)
    pos = torch.randperm(n, generator=g)
    pos_bins = torch.bucketize(torch.arange(n), bin_offsets, right=True) - 1
    bgb, gid_old = _hand_ids(pos_bins, [300 + 211 * b for b in range(nbins)],
                             200 + nbins)
    _check_against_binned(pos.to(torch.int32), gid_old, bin_offsets, bgb,
                          threads=(0, 512, 1024))


def test_compact_layout_equivalence_tile_8192():
    """the default tile: the value tile and the table rows need more than
    64 KB of LDS and a lane walks eight ranks (two tiles and a partial
    third, 128 bins of uneven size, some empty)"""
    tile, nbins = 8192, 128
    n = 2 * tile + 37
    g = torch.Generator().manual_seed(150)
    cuts = torch.sort(torch.randint(0, n + 1, (nbins - 1,), generator=g))
    bin_offsets = torch.cat([torch.tensor([0]), cuts.values,
                             torch.tensor([n])]).to(torch.int64)
    pos = torch.randperm(n, generator=g)
    pos_bins = torch.bucketize(torch.arange(n), bin_offsets, right=True) - 1
    bgb, gid_old = _hand_ids(pos_bins, [1 + 61 * b for b in range(nbins)],
                             151)
    _check_against_binned(pos.to(torch.int32), gid_old, bin_offsets, bgb,
                          tile=tile, threads=(0, 512, 1024))


def test_compact_empty_bins_and_one_bin_tiles():
    """three full tiles over six bins: bins 0, 2 and 5 (start, middle,
    end) are empty, bin 1 is filled by tile 0 alone, tile 1 falls into bin
    3 alone, tile 2 holds the rest of bin 3 and all of bin 4"""
    n = 3 * TILE
    sizes = [0, 512, 0, 700, 324, 0]
    bin_offsets = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
    g = torch.Generator().manual_seed(301)
    p1 = torch.randperm(512, generator=g)
    p3 = torch.randperm(700, generator=g) + 512
    p4 = torch.randperm(324, generator=g) + 1212
    t2 = torch.cat([p3[512:], p4])
    pos = torch.cat([p1, p3[:512], t2[torch.randperm(512, generator=g)]])
    assert torch.equal(torch.sort(pos).values, torch.arange(n))
    pos_bins = torch.bucketize(torch.arange(n), bin_offsets, right=True) - 1
    bgb, gid_old = _hand_ids(pos_bins, [5, 4000, 0, 65536, 17, 9], 302)
    _, _, tstart, _ = _check_against_binned(
        pos.to(torch.int32), gid_old, bin_offsets, bgb
    )
    ts = _u16(tstart)
    assert ts[0].tolist() == [0, 0, 512, 512, 512, 512, 512]
    assert ts[1].tolist() == [0, 0, 0, 0, 512, 512, 512]
    assert ts[2].tolist() == [0, 0, 0, 0, 188, 512, 512]


@pytest.mark.parametrize("n", [100, 1])
def test_compact_smaller_than_a_tile(n):
    sizes = [n // 3, 0, n - n // 3]
    bin_offsets = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
    pos = torch.randperm(n, generator=torch.Generator().manual_seed(400 + n))
    pos_bins = torch.bucketize(torch.arange(n), bin_offsets, right=True) - 1
    bgb, gid_old = _hand_ids(pos_bins, [40, 3, 50], 401)
    rank, rel, tstart, tdelta = _check_against_binned(
        pos.to(torch.int32), gid_old, bin_offsets, bgb
    )
    # and through the aggregate and the one-call step
    ext = get_ext()
    chunk = 256
    chunks = [(s + chunk - 1) // chunk for s in sizes]
    bcb = torch.tensor([0] + chunks, dtype=torch.int64).cumsum(0)
    vals = torch.rand(n, dtype=torch.float64,
                      generator=torch.Generator().manual_seed(402)) + 0.5
    want = torch.zeros(int(bgb[-1]), dtype=torch.float64)
    want.index_add_(0, gid_old.long()[pos], vals)
    out = ext.gb_replay_compact(
        vals.cuda(), rel, rank, tstart, tdelta, bin_offsets.cuda(),
        bgb.cuda(), bcb.cuda(), sum(chunks), int(bgb[-1]), chunk, 2048, TILE,
    )
    assert torch.allclose(out.cpu(), want, rtol=1e-12)
    assert torch.equal(out.cpu() != 0, want != 0)


def test_compact_bindings_empty():
    """n = 0 through the new bindings: empty results, no launch"""
    ext = get_ext()
    i32 = dict(dtype=torch.int32, device="cuda")
    zeros = torch.zeros(5, dtype=torch.int64, device="cuda")
    rank, rel, tstart, tdelta = ext.scatter_tile_prepare_compact(
        torch.empty(0, **i32), torch.empty(0, **i32), zeros, zeros, TILE
    )
    assert rank.numel() == 0 and rank.dtype == torch.int16
    assert rel.numel() == 0 and rel.dtype == torch.int16
    assert tuple(tstart.shape) == (0, 5) and tstart.dtype == torch.int16
    assert tuple(tdelta.shape) == (0, 4) and tdelta.dtype == torch.int32
    vals = torch.empty(0, dtype=torch.float64, device="cuda")
    out = ext.scatter_tile_compact(vals, rank, tstart, tdelta, TILE)
    assert out.numel() == 0 and out.dtype == torch.float64
    out = ext.gb_dense_aggregate_compact(
        rel, vals, zeros, zeros, zeros, 0, 0, 1024, 8192
    )
    assert out.numel() == 0 and out.dtype == torch.float64
    out = ext.gb_replay_compact(
        vals, rel, rank, tstart, tdelta, zeros, zeros, zeros, 0, 0, 1024,
        8192, TILE,
    )
    assert out.numel() == 0 and out.dtype == torch.float64


def test_compact_non_permutation_dropped():
    """a few positions >= n: those rows are dropped exactly as the binned
    pair drops them, and nothing is written outside [0, n)"""
    ext = get_ext()
    n, margin, poison = 2 * TILE + 37, 1024, -7.25
    g = torch.Generator().manual_seed(501)
    sizes = [400, 0, 500, n - 900]
    bin_offsets = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
    pos = torch.randperm(n, generator=g)
    bad = torch.tensor([3, 511, 512, 700, n - 1])
    pos[bad] = torch.tensor([n, n + 5, 2**31 - 1, n + 4096, 2**30])
    pos_bins = torch.bucketize(torch.arange(n), bin_offsets, right=True) - 1
    bgb, gid_old = _hand_ids(pos_bins, [100, 1, 8192, 3000], 502)
    rank, rel, tstart, tdelta = _check_against_binned(
        pos.to(torch.int32), gid_old, bin_offsets, bgb
    )
    # placed rows per tile: the tile's rows less its bad positions
    assert _u16(tstart)[:, -1].tolist() == [TILE - 2, TILE - 2, 37 - 1]
    _, dst0, _ = ext.scatter_tile_prepare_binned(
        pos.to(torch.int32).cuda(), gid_old.cuda(), bin_offsets.cuda(), TILE
    )
    vals = torch.randn(n, dtype=torch.float64, generator=g)
    for th in (512, 1024):
        buf = torch.full((n + 2 * margin,), poison, dtype=torch.float64,
                         device="cuda")
        ref = buf.clone()
        ext.scatter_tile_compact(vals.cuda(), rank, tstart, tdelta, TILE, th,
                                 buf[margin:margin + n])
        # the binned pair on the same poisoned ground
        d = dst0.cpu().long()
        placed = d >= 0
        assert int(placed.sum()) == n - bad.numel()
        row_vals = torch.empty(n, dtype=torch.float64)
        for t0 in range(0, n, TILE):
            cnt = min(TILE, n - t0)
            row_vals[t0:t0 + cnt][_u16(rank)[t0:t0 + cnt]] = \
                vals[t0:t0 + cnt]
        ref = ref.cpu()
        ref[margin + d[placed]] = row_vals[placed]
        assert torch.equal(buf.cpu(), ref), th


def _aggregate_case(slots, chunk):
    """the hand-built bins of test_binned_aggregate_hand_built: an empty
    bin, one shorter than a chunk, one of exactly three chunks (and one of
    exactly one), a final partial chunk, a bin exactly as wide as the table
    and one wider, whose ids past the table take the global-add branch"""
    rows = [0, chunk // 2 + 3, 3 * chunk, 2 * chunk + 77, chunk, 0,
            2 * chunk + 5]
    width = [0, 300, 1000, 17, slots, 0, slots + 500]
    bin_offsets = torch.tensor([0] + rows, dtype=torch.int64).cumsum(0)
    bgb = torch.tensor([0] + width, dtype=torch.int64).cumsum(0)
    chunks = [(r + chunk - 1) // chunk for r in rows]
    bcb = torch.tensor([0] + chunks, dtype=torch.int64).cumsum(0)
    g = torch.Generator().manual_seed(81)
    rel = []
    for r, w in zip(rows, width):
        if r:
            x = torch.randint(0, w, (r,), generator=g)
            x[0], x[-1] = 0, w - 1  # first and last id of the bin
            if w >= slots:
                x[1] = slots - 1  # last slot of the table
            rel.append(x)
    rel = torch.cat(rel)
    bins = torch.repeat_interleave(torch.arange(len(rows)),
                                   torch.tensor(rows))
    gid = (rel + bgb[bins]).to(torch.int32)
    vals = torch.rand(sum(rows), dtype=torch.float64, generator=g) + 0.5
    return (bin_offsets, bgb, bcb, sum(chunks), sum(width), gid,
            rel.to(torch.int16), vals)


@pytest.mark.parametrize(
    "slots,chunk", [(2048, 1024), (4096, 16384), (8192, 4096), (8192, 65536)]
)
def test_compact_aggregate_hand_built(slots, chunk):
    ext = get_ext()
    bo, bgb, bcb, total, n_groups, gid, rel, vals = _aggregate_case(
        slots, chunk
    )
    assert int(_u16(rel).max()) == slots + 500 - 1
    args = (bo.cuda(), bgb.cuda(), bcb.cuda(), total, n_groups, chunk, slots)
    out = ext.gb_dense_aggregate_compact(rel.cuda(), vals.cuda(), *args)
    old = ext.gb_dense_aggregate_binned(gid.cuda(), vals.cuda(), *args)
    want = torch.zeros(n_groups, dtype=torch.float64)
    want.index_add_(0, gid.long(), vals)
    assert torch.allclose(out.cpu(), want, rtol=1e-12)
    assert torch.allclose(out, old, rtol=1e-12)
    # values are >= 0.5: a group is touched exactly when its sum is not 0
    assert torch.equal(out.cpu() != 0, want != 0)
    assert int((out != 0).sum()) == int((old != 0).sum())


# ---- end to end through ops.groupby_aggregate ----


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


def _run_end_to_end(monkeypatch, keys, tile, parts, compact, seed):
    """first sight, the recording call and two replays with fresh values;
    every call against the CPU reference.  Returns (entry, out_keys,
    out_count) of the last call."""
    monkeypatch.setenv("FUGUE_GB_REPLAY_TILE", str(tile))
    monkeypatch.setenv("FUGUE_GB_REPLAY_BIN_PARTS", str(parts))
    monkeypatch.setenv("FUGUE_GB_BIN_SLOTS", "8192")
    monkeypatch.setenv("FUGUE_GB_REPLAY_COMPACT", str(compact))
    dops._LAYOUT_MEMO.clear()
    dops._LAYOUT_SEEN.clear()
    uniq, inv = torch.unique(keys.cpu(), return_inverse=True)
    ref_count = torch.bincount(inv, minlength=uniq.numel())
    g = torch.Generator(device="cuda").manual_seed(seed)
    kcol = DeviceColumn(keys, None, pa.int64())
    ent = out_keys = out_count = None
    for call in range(1, 5):
        vals = torch.rand(keys.numel(), dtype=torch.float64, device="cuda",
                          generator=g) * 4.0 - 1.0
        out_keys, out_aggs, out_count, _ = _agg(kcol, vals, 200_000)
        want = torch.zeros(uniq.numel(), dtype=torch.float64)
        want.index_add_(0, inv, vals.cpu())
        perm = torch.argsort(out_keys.cpu())
        assert torch.equal(out_keys.cpu()[perm], uniq), call
        assert torch.equal(out_count.cpu()[perm], ref_count), call
        assert torch.allclose(out_aggs["s"].cpu()[perm], want,
                              rtol=1e-12), call
        if call >= 2:
            ent = _entry(keys)
            assert isinstance(ent, dops._DenseLayout), call
            assert ent.bin_parts == parts and ent.tile == tile, call
            assert ent.hits == call - 2, call
    return ent, out_keys, out_count


def _keys_3k(n, seed):
    pool = torch.randint(0, 1 << 40, (3000,), dtype=torch.int64,
                         device="cuda",
                         generator=torch.Generator("cuda").manual_seed(seed))
    idx = torch.randint(0, 3000, (n,), device="cuda",
                        generator=torch.Generator("cuda").manual_seed(seed + 1))
    return pool.index_select(0, idx)


@pytest.mark.parametrize(
    "tile,parts,expect_compact",
    [(2048, 8, True), (512, 32, True), (512, 8, False)],
)
def test_compact_replay_end_to_end(monkeypatch, tile, parts, expect_compact):
    """20K rows, 3K groups, 1024 partitions.  The last case has 128 bins
    at tile 512, more than tile // 16: the knob at 1 falls back to the
    10 B/row binned layout."""
    keys = _keys_3k(20_011, 601)
    got = {}
    for compact in (0, 1, 2):
        ent, out_keys, out_count = _run_end_to_end(
            monkeypatch, keys, tile, parts, compact, 610 + compact
        )
        got[compact] = (out_keys, out_count)
        if compact == 2 and expect_compact:
            assert ent.dst is None and ent.rel is None
            assert ent.tile_start is not None and ent.tile_delta is not None
            assert ent.gid.element_size() == 4
            assert ent.gid.numel() == keys.numel()
        elif compact and expect_compact:
            assert ent.dst is None and ent.gid is None
            assert ent.rel.element_size() == 2
            assert ent.rel.numel() == keys.numel()
            nbins = 1024 // parts
            ntiles = (keys.numel() + tile - 1) // tile
            assert tuple(ent.tile_start.shape) == (ntiles, nbins + 1)
            assert tuple(ent.tile_delta.shape) == (ntiles, nbins)
        else:
            assert ent.rel is None and ent.tile_start is None
            assert ent.dst is not None and ent.dst.numel() == keys.numel()
            assert ent.gid.element_size() == 4
    # same keys and counts in the same output order
    for compact in (1, 2):
        assert torch.equal(got[0][0], got[compact][0])
        assert torch.equal(got[0][1], got[compact][1])


def test_compact_replay_heavy_hitter(monkeypatch):
    """one key holds half of the rows: every wave adds into one LDS slot"""
    keys = _keys_3k(20_011, 701)
    hot = torch.rand(keys.numel(), device="cuda",
                     generator=torch.Generator("cuda").manual_seed(702)) < 0.5
    keys = torch.where(hot, torch.full_like(keys, 777), keys)
    ent, _, _ = _run_end_to_end(monkeypatch, keys, 512, 32, 1, 703)
    assert ent.dst is None and ent.rel.element_size() == 2
