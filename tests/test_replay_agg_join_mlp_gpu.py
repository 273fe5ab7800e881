"""GPU tests of the two kernels that keep more loads in flight:
``gb_dense_aggregate_compact`` (contiguous block ranges, the LDS table
carried from chunk to chunk of a bin, a register-pipelined row loop) and
``join_unique_select`` (fewer probe rows per block for small probes).  Both
are called through the extension bindings.

Aggregate: hand-built ``rel`` / values / bin arrays.  Values are small
integers held in fp64, so every sum is exact in any order and the result
must EQUAL ``numpy.bincount`` on the CPU.  Join: sorted row sets against
``join_select_refs.py``, exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

import join_select_refs as jr
from fugue_amd.hip import ops as dops
from fugue_amd.hip.ext import get_ext

MAX_GRID = 8192  # most blocks of any launch (device_common.h)
SENTINEL = -7.0
TAIL = 64


def _layout(rows, widths, chunk, seed):
    """bin arrays of the compact layout for bins of ``rows`` rows and
    ``widths`` ids, and per row an id relative to its bin (the first and
    the last id of every bin among them) and a small integer value"""
    rng = np.random.default_rng(seed)
    bo = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    bgb = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    chunks = [(r + chunk - 1) // chunk for r in rows]
    bcb = np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64)
    rel = []
    for r, w in zip(rows, widths):
        x = rng.integers(0, w, r)
        if r:
            x[0], x[-1] = w - 1, 0
        rel.append(x)
    rel = np.concatenate(rel).astype(np.int64)
    vals = rng.integers(-9, 10, len(rel)).astype(np.float64)
    return bo, bgb, bcb, int(sum(chunks)), rel, vals


def _check_aggregate(rows, widths, chunk, slots, seed=0, n_groups=None,
                     bgb=None):
    """run the kernel into a zeroed buffer with a sentinel tail and compare
    with numpy.bincount, exactly; ids at or past n_groups are dropped"""
    bo, bgb0, bcb, total, rel, vals = _layout(rows, widths, chunk, seed)
    if bgb is None:
        bgb = bgb0
    bgb = np.asarray(bgb, dtype=np.int64)
    if n_groups is None:
        n_groups = int(bgb[-1])
    bins = np.repeat(np.arange(len(rows)), rows)
    gid = bgb[bins] + rel
    keep = gid < n_groups
    want = np.bincount(gid[keep], weights=vals[keep], minlength=n_groups)
    assert rel.max(initial=0) < 65536
    buf = torch.full((n_groups + TAIL,), SENTINEL, dtype=torch.float64,
                     device="cuda")
    buf[:n_groups] = 0
    rel16 = torch.from_numpy(rel.astype(np.uint16).view(np.int16)).cuda()
    out = get_ext().gb_dense_aggregate_compact(
        rel16, torch.from_numpy(vals).cuda(), torch.from_numpy(bo).cuda(),
        torch.from_numpy(bgb).cuda(), torch.from_numpy(bcb).cuda(), total,
        n_groups, chunk, slots, out=buf,
    )
    assert out.data_ptr() == buf.data_ptr() and out.numel() == n_groups
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[:n_groups], want)
    np.testing.assert_array_equal(got[n_groups:], np.full(TAIL, SENTINEL))
    # the binding that allocates its own result answers the same
    own = get_ext().gb_dense_aggregate_compact(
        rel16, torch.from_numpy(vals).cuda(), torch.from_numpy(bo).cuda(),
        torch.from_numpy(bgb).cuda(), torch.from_numpy(bcb).cuda(), total,
        n_groups, chunk, slots,
    )
    np.testing.assert_array_equal(own.cpu().numpy(), want)
    return total


SLOTS = [2048, 4096, 8192]


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("rows", [[1000, 0, 1537], [1001, 3, 1537]])
def test_empty_bin_bin_change_and_ragged_ends(rows, slots):
    """an empty bin, a bin change inside one block's range, heads and tails
    that are no multiple of four rows (the second shape also starts bins
    at rows that are not)"""
    total = _check_aggregate(rows, [700, 5, 1900], 256, slots, seed=1)
    assert total == sum((r + 255) // 256 for r in rows)


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize(
    "rows,chunk",
    [([200], 256), ([256], 256), ([5], 256), ([1], 65536), ([7, 1, 2], 4),
     ([900, 1], 256)],
)
def test_fewer_chunks_than_blocks(rows, chunk, slots):
    """total_chunks below any grid, and total_chunks == 1; a bin of five
    rows and bins of one row"""
    _check_aggregate(rows, [33] * len(rows), chunk, slots, seed=2)


@pytest.mark.parametrize("chunk", [256, 4096])
def test_bin_wider_than_the_table(chunk):
    """a bin three times as wide as the 2048-slot table between two narrow
    ones: its ids past the table add straight to the result, and the table
    carried over from the bin before must not take them"""
    _check_aggregate([3000, 9000, 2000], [2048, 3 * 2048, 100], chunk, 2048,
                     seed=3)


def test_range_from_mid_bin_to_mid_bin():
    """two bins of about 10K chunks of 256 rows, more chunks than twice the
    largest grid.  The chunk counts are chosen so that for every grid from
    2 up to the largest the first chunk of bin 1 is the first chunk of no
    block (checked here for the even split, the first `rem` blocks one
    chunk longer): the block that owns it also owns the last chunk of bin
    0, so its range starts inside bin 0 and ends inside bin 1"""
    c0, c1 = 10037, 9998
    rows = [c0 * 256 - 100, c1 * 256 - 13]
    t = c0 + c1
    g = np.arange(2, MAX_GRID + 1)
    q, rem = t // g, t % g
    assert (q >= 2).all()
    # block bx starts at chunk bx * q + min(bx, rem)
    starts_a_block = ((c0 % (q + 1) == 0) & (c0 // (q + 1) <= rem)) | (
        ((c0 - rem) % q == 0) & ((c0 - rem) // q >= rem)
    )
    assert not starts_a_block.any()
    for slots in (2048, 8192):
        _check_aggregate(rows, [1500, 2048], 256, slots, seed=4)


@pytest.mark.parametrize("slots", SLOTS)
def test_ids_past_n_groups_are_dropped(slots):
    """bin_group_base placed so that base + rel reaches and passes
    n_groups, through the table (rel < slots) and through the global add
    (rel >= slots): those rows are dropped and nothing is written past the
    end"""
    rows, widths = [1200, 2100, 900], [500, slots + 300, 400]
    n_groups = 500 + slots + 100  # inside the global-add part of bin 1
    _check_aggregate(rows, widths, 256, slots, seed=5, n_groups=n_groups)
    # the last bin wholly past the end, the middle one cut inside the table
    _check_aggregate(rows, widths, 256, slots, seed=6, n_groups=500 + 77)
    # a base past the end of a result of 10 groups
    _check_aggregate([300, 300], [10, 10], 256, slots, seed=7, n_groups=10,
                     bgb=[0, 5, 15])


# ---- join_unique_select ----

PROBE, BUILD = jr.PROBE, jr.BUILD
BLOCK_ROWS = [0, 1024, 2048, int(get_ext().COMPACT_CHUNK)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("with_pred", [False, True])
@pytest.mark.parametrize("frac", [0.5, 1.0])
@pytest.mark.parametrize("np_", [1, 255, 1025, 4097, 20000])
def test_join_probe_sizes_every_block_size(np_, frac, with_pred):
    """probe sizes on both sides of every rows-per-block the launcher can
    choose, each through the launcher's own choice (0) and through every
    instantiation forced; half or all of the keys present; with and
    without `s > w`, one operand holding a NaN"""
    rng = np.random.default_rng(7 * np_ + int(10 * frac) + with_pred)
    nb = 3000
    pool = rng.permutation(np.arange(-nb, nb, dtype=np.int64) * 7919)
    b, absent = pool[:nb], pool[nb:]
    hit = rng.random(np_) < frac
    p = np.where(hit, b[rng.integers(0, nb, np_)],
                 absent[rng.integers(0, nb, np_)]).astype(np.int64)
    s = rng.random(np_)
    w = rng.random(nb)
    pred = None
    if with_pred:
        s[np_ // 2] = np.nan
        pred = (4, (PROBE, s), (BUILD, w))
    specs = [(PROBE, p), (PROBE, s), (BUILD, w)]
    want = jr.join_select_ref(p, b, pred, specs)
    if frac == 1.0 and not with_pred:
        assert len(want) == np_
    ext = get_ext()
    bk = _dev(b)
    heads, nxt, dup = ext.join_build(bk, dops._next_pow2(2 * nb))
    assert int(dup.item()) == 0
    dpred = None
    if with_pred:
        dpred = (4, (PROBE, _dev(s)), (BUILD, _dev(w)))
    dspecs = [(side, _dev(c)) for side, c in specs]
    for block_rows in BLOCK_ROWS:
        outs = ext.join_unique_select(_dev(p), bk, heads, nxt, dpred, dspecs,
                                      block_rows=block_rows)
        total = int(outs[-1].item())
        assert total == len(want), block_rows
        got = jr.sorted_rows(
            [t.narrow(0, 0, total).cpu().numpy() for t in outs[:-1]]
        )
        np.testing.assert_array_equal(got, want, err_msg=str(block_rows))


def test_join_block_rows_is_checked():
    ext = get_ext()
    k = torch.arange(8, dtype=torch.int64, device="cuda")
    heads, nxt, _ = ext.join_build(k, 16)
    with pytest.raises(RuntimeError):
        ext.join_unique_select(k, k, heads, nxt, None, [(0, k)],
                               block_rows=512)
