"""Device relational primitives: row hashing, radix partition, group-by
aggregation, hash join, sort.

These wrap the hand-written CDNA4 kernels (``csrc/*.hip``) plus
rocPRIM-backed torch primitives (sort/cumsum/unique — the "library GEMM"
equivalents).  Reference call sites being replaced are listed in
SURVEY.md §2.3.
"""
from typing import Any, Dict, List, Optional, Sequence, Tuple

import os
import weakref
from dataclasses import dataclass

import numpy as np
import pyarrow as pa
import torch

from fugue_amd.exceptions import FugueBug
from fugue_amd.hip.ext import get_ext
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame, StringDeviceColumn
from fugue_amd.schema import Schema

GB_EMPTY = -0x8000000000000000  # GB_EMPTY of csrc/relational.h, as int64
# copies of two csrc/relational.h limits, for hosts without the extension;
# the extension exports its own values under the same names, and
# tests/test_groupby_kernels_gpu.py holds the copies to them
PACK_MAX_COLS = 8
GB_LDS_MAX_AGGS = 4

AGG_SUM = 0
AGG_MIN = 1
AGG_MAX = 2
AGG_COUNT = 3


def _next_pow2(n: int) -> int:
    p = 1
    while p < n:
        p <<= 1
    return p


def _is_cpu(t: torch.Tensor) -> bool:
    return t.device.type == "cpu"


# ------------------------------------------------------------------ #
# CPU equivalents (numpy uint64) of the kernel hash — used when frames
# are CPU-resident (gloo multi-process tests; no GPU in CI).  The GPU
# path always runs the HIP kernels; on a GPU host the extension is
# REQUIRED (get_ext raises loudly if it failed to build).
# ------------------------------------------------------------------ #
def _np_mix64(x: "np.ndarray") -> "np.ndarray":
    with np.errstate(over="ignore"):
        x = x.astype(np.uint64, copy=True)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
        return x


def _np_hash_combine(h: "np.ndarray", v: "np.ndarray") -> "np.ndarray":
    with np.errstate(over="ignore"):
        return _np_mix64(
            h
            ^ (
                v
                + np.uint64(0x9E3779B97F4A7C15)
                + (h << np.uint64(6))
                + (h >> np.uint64(2))
            )
        )


def _hash_rows_cpu(
    cols: Sequence[DeviceColumn], seed: Optional[int] = None
) -> torch.Tensor:
    out: Optional[np.ndarray] = None
    null_h = np.uint64(0x9E3779B97F4A7C15)
    if seed is not None:
        n = len(cols[0])
        out = _np_mix64(np.full(n, np.uint64(seed) + np.uint64(1)))
    for c in cols:
        if isinstance(c, StringDeviceColumn):
            import pandas as pd

            strings = c.to_arrow().to_pandas()
            # null cells get null_h below; their placeholder must not hold
            # a NUL (pandas' object hashing stops at it, and a "\0..."
            # placeholder changed the hash of "" in the same column).
            # Known limit of this host twin: for the same reason strings
            # that differ only after an embedded NUL ("ab", "ab\0") share
            # one hash here, while the kernel tells them apart (STATUS.md)
            v = pd.util.hash_array(
                strings.fillna("").to_numpy(dtype=object)
            ).astype(np.uint64)
            v = _np_mix64(v)
            if c.valid is not None:
                v = np.where(c.valid.numpy(), v, null_h)
        else:
            raw = c.data.numpy()
            if raw.dtype == np.bool_:
                raw = raw.astype(np.uint8)
            elif raw.dtype == np.int16:
                # hash_rows widens int16 to int32 (sign-extending) before
                # the kernel hashes the 32 raw bits
                raw = raw.astype(np.int32)
            bits = raw.view(_unsigned_view_dtype(raw.dtype)).astype(np.uint64)
            v = _np_mix64(bits)
            if c.valid is not None:
                v = np.where(c.valid.numpy(), v, null_h)
        out = v if out is None else _np_hash_combine(out, v)
    return torch.from_numpy(out.view(np.int64).copy())


def _unsigned_view_dtype(dt: "np.dtype"):
    m = {
        np.dtype("int64"): np.uint64,
        np.dtype("float64"): np.uint64,
        np.dtype("int32"): np.uint32,
        np.dtype("float32"): np.uint32,
        np.dtype("int16"): np.uint16,
        np.dtype("int8"): np.uint8,
        np.dtype("uint8"): np.uint8,
    }
    return m[np.dtype(dt)]


def hash_rows(
    cols: Sequence[DeviceColumn], seed: Optional[int] = None
) -> torch.Tensor:
    """Row-wise 64-bit hash over multiple columns (strings included);
    int64 tensor holding uint64 bits.  ``seed`` derives an independent
    hash family (used for 128-bit verification of string keys)."""
    if _is_cpu(cols[0].data):
        return _hash_rows_cpu(cols, seed=seed)
    ext = get_ext()
    n = len(cols[0])
    device = cols[0].data.device
    out = torch.empty(n, dtype=torch.int64, device=device)
    first = seed is None
    if seed is not None:
        ext.hash_seed(out, seed)
    for c in cols:
        if isinstance(c, StringDeviceColumn):
            ext.hash_string_column(c.offsets, c.bytes, c.valid, out, first)
        else:
            data = c.data
            if data.dtype == torch.int16:
                data = data.to(torch.int32)
            ext.hash_column(data, c.valid, out, first)
        first = False
    return out


def partition_by_hash(
    df: HipDataFrame, hashes: torch.Tensor, num_buckets: int
) -> Tuple[HipDataFrame, torch.Tensor]:
    """Reorder rows bucket-contiguously; returns (frame, counts[num_buckets]).

    MI355X equivalent of Dask's ``hash_repartition``
    (``fugue_dask/_utils.py:44``).
    """
    if _is_cpu(hashes):
        h = hashes.numpy().view(np.uint64)
        buckets_np = (h % np.uint64(num_buckets)).astype(np.int64)
        counts_np = np.bincount(buckets_np, minlength=num_buckets)
        perm_np = np.argsort(buckets_np, kind="stable")
        return (
            df.gather_rows(torch.from_numpy(perm_np)),
            torch.from_numpy(counts_np.astype(np.int64)),
        )
    ext = get_ext()
    buckets = ext.bucket_of(hashes, num_buckets)
    counts = ext.bucket_histogram(buckets, num_buckets)
    offsets = torch.zeros(num_buckets, dtype=torch.int64, device=hashes.device)
    torch.cumsum(counts[:-1], 0, out=offsets[1:])
    perm = ext.bucket_scatter(buckets, offsets.clone())
    return df.gather_rows(perm), counts


def partition_by_bucket_ids(
    df: HipDataFrame, bucket_ids: torch.Tensor, num_buckets: int
) -> Tuple[HipDataFrame, torch.Tensor]:
    """Reorder rows into bucket-contiguous order given explicit bucket ids
    (rand / even repartition)."""
    if _is_cpu(bucket_ids):
        b = bucket_ids.numpy().astype(np.int64)
        counts_np = np.bincount(b, minlength=num_buckets)
        perm_np = np.argsort(b, kind="stable")
        return (
            df.gather_rows(torch.from_numpy(perm_np)),
            torch.from_numpy(counts_np.astype(np.int64)),
        )
    ext = get_ext()
    b32 = bucket_ids.to(torch.int32)
    counts = ext.bucket_histogram(b32, num_buckets)
    offsets = torch.zeros(
        num_buckets, dtype=torch.int64, device=bucket_ids.device
    )
    torch.cumsum(counts[:-1], 0, out=offsets[1:])
    perm = ext.bucket_scatter(b32, offsets.clone())
    return df.gather_rows(perm), counts


def rand_buckets(n: int, num_buckets: int, seed: Optional[int], device) -> torch.Tensor:
    gen = torch.Generator(device=device)
    if seed is not None:
        gen.manual_seed(seed)
    return torch.randint(
        0, num_buckets, (n,), dtype=torch.int64, device=device, generator=gen
    )




# ---------------------------------------------------------------- #
# fused group-key statistics (own kernels, single host readback)    #
# ---------------------------------------------------------------- #

_KEY_STATS_MEMO: "Dict[Tuple[int, ...], Tuple[Any, Any]]" = {}
_KEY_STATS_MEMO_CAP = 128

# join build-table reuse: the chained table (heads, next) of a build-key
# tensor and its duplicate flag depend on nothing but the keys, and a
# persistent dimension table is the same tensor on every call (iterating
# driver, plan cache).  Keyed like _KEY_STATS_MEMO — (address, length,
# dtype) plus a weakref to the key tensor that must still be alive — so a
# repeated build side skips join_build, join_dup_check, the heads fill
# and the flag readback.  heads is 4 B x tsize (2 to 4 slots per build
# row) and next 4 B per row: 12 to 20 B per build row.  At most
# _JOIN_BUILD_MEMO_CAP entries, first-in first-out; a table above
# _JOIN_BUILD_MEMO_MAX_BYTES (256 MB, about 13M to 22M build rows) is
# built per call and never kept.  FUGUE_JOIN_BUILD_MEMO=0 disables it.
_JOIN_BUILD_MEMO: "Dict[Tuple[Any, ...], Tuple[Any, Any]]" = {}
_JOIN_BUILD_MEMO_CAP = 4
_JOIN_BUILD_MEMO_MAX_BYTES = 256 << 20

# shuffle-layout reuse (Spark shuffle-reuse analog): for a repeated key
# tensor, the partition layout is recorded once and fresh values replay
# through it.  A plain entry caches the spill keys + per-row positions
# (pkeys 4-8 B + pos 4 B per row).  A dense entry (single SUM over a
# null-free fp64 column, FUGUE_GB_REPLAY_DENSE=1) caches per row the
# dense group id (4 B) and the tile scatter's rank + destination
# (2 B + 4 B) = 10 B/row, plus keys and counts per GROUP; pkeys and pos
# are dropped.  When the values are laid out by bins of partitions
# (FUGUE_GB_REPLAY_BIN_PARTS) the compact form (FUGUE_GB_REPLAY_COMPACT)
# keeps the rank and a 16-bit id relative to the bin (2 B + 2 B) = 4
# B/row plus a [tiles, bins] destination table (6 B per tile and bin,
# under 12 MB at 125M rows); with the knob off, or more than tile/16
# bins, the binned layout keeps the 10 B/row.  Two entries ~0.5GB each
# at 125M rows (~1.25GB each when not compact) — bound the cache
# tightly.
_LAYOUT_MEMO: "Dict[Tuple[Any, ...], Any]" = {}
_LAYOUT_MEMO_CAP = 2
# key tensors seen once (candidates): recording uses the slower simple
# scatter, so it only happens on the SECOND sight of the same keys —
# one-shot group-bys never pay the record cost
_LAYOUT_SEEN: "Dict[Tuple[Any, ...], Any]" = {}
_LAYOUT_SEEN_CAP = 16

def _key_stats_device(
    datas: "List[torch.Tensor]",
    valids: "List[Optional[torch.Tensor]]",
    with_minmax: bool,
) -> Tuple[Optional[List[int]], Optional[List[int]], int]:
    """(mins, maxs, estimated_distinct) for device key columns via ONE
    launch set + ONE host readback (``gb_key_stats``), memoized by the
    column tensors' identities (frames are immutable, so an identical
    tensor tuple ⇒ identical stats; repeated plans skip the kernels AND
    the device sync entirely).  Replaces per-column min/max reductions
    + torch.unique Chao sampling (profiles/NOTES.md r02)."""
    n = int(datas[0].numel())
    # key on (address, length, dtype): re-created VIEWS of the same
    # storage (fresh tensor objects each plan run) still hit.  Safe
    # because a hit requires the memoized tensors to still be ALIVE —
    # two live tensors at one address with one length alias the same
    # bytes (frames treat column tensors as immutable).
    key = tuple(
        (t.data_ptr(), t.numel(), str(t.dtype)) for t in datas
    ) + (n, with_minmax)
    hit = _KEY_STATS_MEMO.get(key)
    if hit is not None:
        refs, value = hit
        if all(r() is not None for r in refs):
            return value
        del _KEY_STATS_MEMO[key]
    ext = get_ext()
    nsamples = min(65536, n)
    st = ext.gb_key_stats(datas, valids, nsamples, 131072, with_minmax)
    st = st.cpu().tolist()  # the single host readback
    k = len(datas)
    BIAS = 1 << 63
    U64 = (1 << 64) - 1

    def _dec(x: int) -> int:
        raw = (x & U64) ^ BIAS  # undo the order-preserving bias
        return raw - (1 << 64) if raw >= BIAS else raw

    mins = maxs = None
    if with_minmax:
        mins = [_dec(v) for v in st[: 2 * k : 2]]
        maxs = [_dec(v) for v in st[1 : 2 * k : 2]]
    d, f1, f2 = st[2 * k], st[2 * k + 1], st[2 * k + 2]
    if n > nsamples:
        est = d + (f1 * f1) // max(2 * f2, 1)
        est = max(d, min(n, est))
    else:
        est = max(1, d)
    value = (mins, maxs, est)
    if len(_KEY_STATS_MEMO) >= _KEY_STATS_MEMO_CAP:
        _KEY_STATS_MEMO.pop(next(iter(_KEY_STATS_MEMO)))
    _KEY_STATS_MEMO[key] = (tuple(weakref.ref(t) for t in datas), value)
    return value


def _layout_second_sight(lkey: tuple, packed: "torch.Tensor") -> bool:
    """True when this key tensor was already aggregated once (same
    address, still alive) — the signal that recording its layout will
    pay off."""
    hit = _LAYOUT_SEEN.get(lkey)
    if hit is not None and hit() is not None:
        return True
    if len(_LAYOUT_SEEN) >= _LAYOUT_SEEN_CAP:
        _LAYOUT_SEEN.pop(next(iter(_LAYOUT_SEEN)))
    _LAYOUT_SEEN[lkey] = weakref.ref(packed)
    return False


@dataclass
class _PlainLayout:
    """Recorded layout replayed through ``gb_aggregate_replay``."""

    ref: Any  # weakref to the packed key tensor the layout was made from
    pkeys: "torch.Tensor"  # spill keys (int32 when the keys fit 31 bits)
    pos: "torch.Tensor"  # spill position of every row


@dataclass
class _DenseLayout:
    """Recorded layout replayed through ``gb_replay_dense``: the value
    scatter is either tile-coalesced (``tile`` > 0: ``rank`` and ``dst``
    from ``scatter_tile_prepare``) or by recorded position (``tile`` ==
    0: ``pos``).  With ``bin_parts`` > 1 the values are laid out by bins
    of that many consecutive hash partitions instead (``rank``, ``dst``
    and ``gid`` from ``scatter_tile_prepare_binned``; ``gid`` is then in
    binned order) and the bin arrays drive the aggregate.  A compact
    binned entry (``tile_start`` is not None, from
    ``scatter_tile_prepare_compact``) holds the per-tile tables instead of
    ``dst``, and either the 16-bit ``rel`` (``gid`` is None) or, with
    ``FUGUE_GB_REPLAY_COMPACT=2``, the int32 ``gid`` (``rel`` is None)."""

    ref: Any
    gid: Optional["torch.Tensor"]
    offsets: "torch.Tensor"
    group_base: "torch.Tensor"
    n_groups: int
    out_keys: "torch.Tensor"
    out_count: "torch.Tensor"
    rank: Optional["torch.Tensor"]
    dst: Optional["torch.Tensor"]
    pos: Optional["torch.Tensor"]
    tile: int
    hits: int = 0  # replayed steps served by this entry
    bin_parts: int = 1  # partitions per bin (1: the partition layout)
    bin_offsets: Optional["torch.Tensor"] = None  # [B+1] offsets[::M]
    bin_group_base: Optional["torch.Tensor"] = None  # [B+1] group_base[::M]
    bin_chunk_base: Optional["torch.Tensor"] = None  # [B+1] chunk prefix
    bin_chunks: int = 0  # total aggregate chunks over all bins
    bin_chunk: int = 0  # rows per aggregate chunk bin_chunk_base is for
    bin_slots: int = 0  # table slots the bin width was chosen for
    rel: Optional["torch.Tensor"] = None  # [n] uint16 id - bin_group_base
    tile_start: Optional["torch.Tensor"] = None  # [tiles, B+1] uint16
    tile_delta: Optional["torch.Tensor"] = None  # [tiles, B] int32


def _layout_get(lkey: tuple) -> Any:
    """The memoized layout for this key while its key tensor is alive."""
    ent = _LAYOUT_MEMO.get(lkey)
    return ent if ent is not None and ent.ref() is not None else None


def _layout_put(lkey: tuple, ent: Any) -> None:
    if len(_LAYOUT_MEMO) >= _LAYOUT_MEMO_CAP:
        _LAYOUT_MEMO.pop(next(iter(_LAYOUT_MEMO)))
    _LAYOUT_MEMO[lkey] = ent


def _choose_bin_parts(
    group_base: List[int], num_parts: int, max_parts: int, slots: int
) -> int:
    """Partitions per bin: the largest power of two that is at most
    ``max_parts``, divides ``num_parts`` and keeps every bin's group ids
    within ``slots`` (``group_base`` is the host copy, [P+1])."""
    m = 1
    while (
        m * 2 <= max_parts
        and num_parts % (m * 2) == 0
        and max(
            group_base[b + m * 2] - group_base[b]
            for b in range(0, num_parts, m * 2)
        ) <= slots
    ):
        m *= 2
    return m


def _prepare_dense_layout(
    ext: Any, packed: "torch.Tensor", pkeys: "torch.Tensor",
    pos: "torch.Tensor", num_parts: int, tile: int,
    bin_parts: int = 1, bin_slots: int = 8192, bin_chunk: int = 65536,
    compact: int = 0,
) -> Optional[_DenseLayout]:
    """One-time preparation of the dense replay layout from the recorded
    partitioned keys (int64) and per-row spill positions; None when it is
    declined (a partition's distinct keys overflow the id-assignment
    table, or G >= 2^31) and the plain replay entry must be kept.  One
    host readback, once per key tensor.  ``bin_parts`` is the most
    partitions a bin of the value layout may hold (1: keep the partition
    layout); the width used is the widest whose bins fit ``bin_slots``.
    ``compact`` asks for the compact form of a binned layout, taken when
    its per-tile table is at most 1/8 of the ``dst`` bytes it replaces
    (``nbins <= tile // 16``): 1 with 16-bit ids, 2 with the int32 ids
    and the binned aggregate."""
    offsets, distinct = ext.gb_dense_count(pkeys=pkeys, num_parts=num_parts)
    group_base = torch.zeros(
        num_parts + 1, dtype=torch.int64, device=pkeys.device
    )
    torch.cumsum(distinct, 0, out=group_base[1:])
    binned = tile > 0 and bin_parts > 1
    if binned:
        # the same single readback also carries what the bin width and
        # the chunk count are chosen from
        host = torch.cat(
            [distinct.max().reshape(1), group_base, offsets]
        ).tolist()
        dmax, gb_host = host[0], host[1 : num_parts + 2]
        off_host = host[num_parts + 2 :]
        n_groups = gb_host[-1]
    else:
        dmax, n_groups = torch.stack(
            [distinct.max(), group_base[-1]]
        ).tolist()
    if dmax > int(ext.dense_assign_max()) or n_groups >= (1 << 31):
        return None
    gid, out_keys, out_count = ext.gb_dense_assign(
        pkeys=pkeys, offsets=offsets, group_base=group_base,
        n_groups=n_groups,
    )
    m = 1
    if binned:
        m = _choose_bin_parts(gb_host, num_parts, bin_parts, bin_slots)
    if m > 1:
        bin_offsets = offsets[::m].contiguous()
        bin_rows = [
            off_host[b + m] - off_host[b] for b in range(0, num_parts, m)
        ]
        chunks = torch.tensor(
            [(r + bin_chunk - 1) // bin_chunk for r in bin_rows],
            dtype=torch.int64,
        )
        bin_chunk_base = torch.zeros(chunks.numel() + 1, dtype=torch.int64)
        torch.cumsum(chunks, 0, out=bin_chunk_base[1:])
        bin_group_base = group_base[::m].contiguous()
        dst = rel = tile_start = tile_delta = None
        if compact and num_parts // m <= tile // 16:
            out = ext.scatter_tile_prepare_compact(
                pos=pos, gid=gid, bin_offsets=bin_offsets,
                bin_group_base=bin_group_base, tile=tile,
                keep_gid=compact == 2,
            )
            rank, rel, tile_start, tile_delta = out[:4]
            gid = None
            if compact == 2:
                gid, rel = out[4], None
        else:
            rank, dst, gid = ext.scatter_tile_prepare_binned(
                pos=pos, gid=gid, bin_offsets=bin_offsets, tile=tile
            )
        return _DenseLayout(
            ref=weakref.ref(packed), gid=gid, offsets=offsets,
            group_base=group_base, n_groups=int(n_groups),
            out_keys=out_keys, out_count=out_count, rank=rank, dst=dst,
            pos=None, tile=tile, bin_parts=m, bin_offsets=bin_offsets,
            bin_group_base=bin_group_base,
            bin_chunk_base=bin_chunk_base.to(pkeys.device),
            bin_chunks=int(bin_chunk_base[-1]), bin_chunk=bin_chunk,
            bin_slots=bin_slots, rel=rel, tile_start=tile_start,
            tile_delta=tile_delta,
        )
    rank = dst = None
    if tile > 0:
        rank, dst = ext.scatter_tile_prepare(pos, tile)
    return _DenseLayout(
        ref=weakref.ref(packed), gid=gid, offsets=offsets,
        group_base=group_base, n_groups=int(n_groups), out_keys=out_keys,
        out_count=out_count, rank=rank, dst=dst,
        pos=None if tile > 0 else pos, tile=tile,
    )


@dataclass(frozen=True)
class _GbKnobs:
    """The FUGUE_GB_* tuning knobs of the partitioned group-by, read from
    the environment once per ``groupby_aggregate`` call (A/B scripts and
    tests change them between calls in one process)."""

    staged_max: int = 1_200_000  # FUGUE_GB_STAGED_MAX
    parts: int = 1024  # FUGUE_GB_PARTS: 512, 1024 or 2048
    scatter_chunk: int = 0  # FUGUE_GB_SCATTER_CHUNK (0: kernel default)
    agg_chunk: int = 0  # FUGUE_GB_AGG_CHUNK (0: kernel default)
    narrow: bool = True  # FUGUE_GB_NARROW
    staged_min_rows: int = 48_000_000  # FUGUE_GB_STAGED_MIN_ROWS
    layout_reuse: bool = True  # FUGUE_GB_LAYOUT_REUSE
    replay_dense: bool = True  # FUGUE_GB_REPLAY_DENSE
    # FUGUE_GB_REPLAY_TILE: rows per tile of the replay value scatter, a
    # power of two in [512, 8192], or 0 to replay values by recorded
    # position (the pre-tile scatter, kept for A/B).  The layout is
    # recorded with a reservation chunk equal to the tile, so the rows of
    # one (tile, partition) leave as one contiguous run.
    replay_tile: int = 8192
    # FUGUE_GB_DENSE_SLOTS: LDS table slots of the dense replay
    # aggregate (2048, 4096 or 8192; 8 B per slot)
    dense_slots: int = 4096
    # FUGUE_GB_REPLAY_BIN_PARTS: most consecutive hash partitions merged
    # into one bin of the replayed value layout (a power of two; 1 keeps
    # the partition layout).  A (tile, bin) scatter run is that many
    # times longer than a (tile, partition) run.  The width used is the
    # widest whose bins' group ids fit the binned aggregate's table.
    replay_bin_parts: int = 8
    # FUGUE_GB_BIN_SLOTS / FUGUE_GB_BIN_CHUNK: LDS table slots (2048,
    # 4096 or 8192) and rows per chunk of the binned dense aggregate
    bin_slots: int = 8192
    bin_chunk: int = 65536
    # FUGUE_GB_REPLAY_COMPACT: a binned layout with at most tile/16 bins
    # keeps no per-row destination and 16-bit ids (0: the 10 B/row
    # binned layout, kept for A/B; 2: no destination but the int32 ids
    # and the binned aggregate, 8 B/row, kept for A/B)
    replay_compact: int = 1

    @classmethod
    def from_env(cls) -> "_GbKnobs":
        env = os.environ.get
        parts = int(env("FUGUE_GB_PARTS", "1024"))
        tile = int(env("FUGUE_GB_REPLAY_TILE", "8192"))
        if tile != 0 and (tile < 512 or tile > 8192 or tile & (tile - 1)):
            raise ValueError(
                f"FUGUE_GB_REPLAY_TILE={tile}: expected 0 or a power of two "
                "in [512, 8192]"
            )
        slots = int(env("FUGUE_GB_DENSE_SLOTS", "4096"))
        bin_parts = int(env("FUGUE_GB_REPLAY_BIN_PARTS", "8"))
        if bin_parts < 1 or bin_parts & (bin_parts - 1):
            raise ValueError(
                f"FUGUE_GB_REPLAY_BIN_PARTS={bin_parts}: expected a power "
                "of two >= 1"
            )
        bin_slots = int(env("FUGUE_GB_BIN_SLOTS", "8192"))
        bin_chunk = int(env("FUGUE_GB_BIN_CHUNK", "65536"))
        compact = int(env("FUGUE_GB_REPLAY_COMPACT", "1"))
        return cls(
            staged_max=int(env("FUGUE_GB_STAGED_MAX", "1200000")),
            parts=parts if parts in (512, 1024, 2048) else 512,
            scatter_chunk=int(env("FUGUE_GB_SCATTER_CHUNK", "0")),
            agg_chunk=int(env("FUGUE_GB_AGG_CHUNK", "0")),
            narrow=bool(int(env("FUGUE_GB_NARROW", "1"))),
            staged_min_rows=int(env("FUGUE_GB_STAGED_MIN_ROWS", "48000000")),
            layout_reuse=env("FUGUE_GB_LAYOUT_REUSE", "1") != "0",
            replay_dense=env("FUGUE_GB_REPLAY_DENSE", "1") != "0",
            replay_tile=tile,
            dense_slots=slots if slots in (2048, 4096, 8192) else 4096,
            replay_bin_parts=bin_parts,
            bin_slots=bin_slots if bin_slots in (2048, 4096, 8192) else 8192,
            bin_chunk=bin_chunk if bin_chunk >= 256 else 65536,
            replay_compact=(
                compact if compact in (0, 1, 2) else 1
            ),
        )


@dataclass(frozen=True)
class _GbPlan:
    """How one high-cardinality group-by runs (``_plan_partitioned``)."""

    num_parts: int
    tsize: int  # global group table slots
    narrow: int  # int32 spill keys: 1 yes, 0 no, -1 speculative
    force_simple: bool  # simple scatter instead of the LDS-staged one
    reuse: bool  # record / replay the partition layout
    dense_ok: bool  # a recorded layout may be the dense kind
    tile: int  # replay scatter tile (0: by position)
    sc_chunk: int
    ag_chunk: int


def _table_size(expected_groups: int) -> int:
    return _next_pow2(max(16, int(expected_groups * 2)))


def _plan_partitioned(
    n: int,
    expected_groups: int,
    n_aggs: int,
    fp64_sum: bool,
    key_bits: Optional[int],
    key_range: Optional[Tuple[int, int]],
    knobs: _GbKnobs,
) -> _GbPlan:
    """Plan the 2-phase partitioned aggregation (hash-partition rows so
    each partition's groups fit the per-workgroup LDS table) of ``n``
    rows with ``n_aggs`` SUM/COUNT aggregates over null-free inputs.
    ``fp64_sum``: the single aggregate is a SUM of an fp64 column.
    ``key_bits``: packed key width when the keys were packed (pack meta);
    ``key_range``: measured (lo, hi) of unpacked keys when known."""
    # single-agg path with moderate cardinality uses the LDS
    # write-staged scatter (512 parts, 4096-slot phase-3 table)
    if n_aggs <= 1 and expected_groups <= knobs.staged_max:
        # staged-variant partition count: 512 (8-deep staging,
        # 4096-slot phase-3), 1024 (4-deep, 2048-slot) or 2048
        # (2-deep, 1024-slot) — smaller tables run phase 3 at
        # higher occupancy; A/B via FUGUE_GB_PARTS
        num_parts = knobs.parts
    else:
        num_parts = min(4096, _next_pow2(max(16, expected_groups // 512)))
    # int32 intermediate keys shrink the partitioned spill 16B->12B
    # per row (and its MALL footprint) when the packed key range is
    # known (pack meta) or measured to fit 31 bits
    narrow = 0
    if knobs.narrow:
        if key_bits is not None:
            narrow = 1 if key_bits <= 31 else 0
        elif key_range is not None:
            narrow = 1 if key_range[0] >= 0 and key_range[1] < (1 << 31) else 0
        else:
            narrow = -1  # speculative: overflow flag checked after the run
    # the LDS write-staged scatter pays off only on big spills; at
    # q3-like sizes the simple per-chunk-reservation variant is
    # faster (same-box A/B, profiles/NOTES.md r02)
    force_simple = n < knobs.staged_min_rows
    reuse = (
        knobs.layout_reuse
        and n_aggs == 1
        and n < (1 << 31)
        and num_parts in (512, 1024, 2048)
    )
    # dense replay (FUGUE_GB_REPLAY_DENSE, default on): the zero-copy
    # condition of the aggregate input plus the op
    dense_ok = reuse and knobs.replay_dense and n_aggs == 1 and fp64_sum
    return _GbPlan(
        num_parts=num_parts,
        tsize=_table_size(expected_groups),
        narrow=narrow,
        force_simple=force_simple,
        reuse=reuse,
        dense_ok=dense_ok,
        tile=knobs.replay_tile if dense_ok else 0,
        sc_chunk=knobs.scatter_chunk,
        ag_chunk=knobs.agg_chunk,
    )


def _run_partitioned(
    ext: Any, packed: "torch.Tensor", vals: "torch.Tensor",
    ops: "torch.Tensor", plan: _GbPlan, *, record: bool = False,
) -> Tuple["torch.Tensor", ...]:
    """Run the planned aggregation: (tkeys, gaggs, gcount, pkeys, pos).
    ``record`` keeps the wide spill keys and every row's spill position
    (simple scatter, reservation chunk = replay tile) for a layout entry;
    otherwise pkeys/pos are scratch."""

    def run(narrow: int) -> List["torch.Tensor"]:
        return ext.gb_aggregate_partitioned(
            keys=packed, vals=vals, ops=ops, num_parts=plan.num_parts,
            tsize=plan.tsize, scatter_chunk=plan.sc_chunk,
            agg_chunk=plan.ag_chunk, narrow=narrow, record_layout=record,
            force_simple=plan.force_simple and not record,
            record_chunk=plan.tile if record else 0,
        )

    tkeys, gaggs, gcount, ovf, pkeys, pos = run(0 if record else plan.narrow)
    if not record and plan.narrow == -1 and int(ovf.item()) != 0:
        # a key fell outside [0, 2^31): redo exactly, wide keys
        tkeys, gaggs, gcount, ovf, pkeys, pos = run(0)
    return tkeys, gaggs, gcount, pkeys, pos


def _compact_groups(
    ext: Any, tkeys: "torch.Tensor", gcount: "torch.Tensor",
    gaggs: "torch.Tensor", aggs: List[Tuple[str, int, str]],
    extra: Optional["torch.Tensor"] = None,
) -> Tuple["torch.Tensor", Dict[str, "torch.Tensor"], "torch.Tensor", Any]:
    """Occupied slots of a group table as (keys, {out_name: values},
    counts, extra) in table order; ``extra`` is an optional per-slot
    int64 column compacted alongside.  Deterministic own-kernel
    compaction (replaces nonzero + per-column index_select); ONE host
    read for the total."""
    if len(aggs) > 6:  # beyond the kernel's by-value pointer pack
        occupied = (tkeys != GB_EMPTY).nonzero(as_tuple=True)[0]
        return (
            tkeys.index_select(0, occupied),
            {
                oname: gaggs[i].index_select(0, occupied)
                for i, (_, _, oname) in enumerate(aggs)
            },
            gcount.index_select(0, occupied),
            None if extra is None else extra.index_select(0, occupied),
        )
    ck, cc, ca, ce, bases = ext.gb_compact(tkeys, gcount, gaggs, extra)
    total = int(bases[-1].item())
    return (
        ck.narrow(0, 0, total),
        {
            oname: ca[i].narrow(0, 0, total)
            for i, (_, _, oname) in enumerate(aggs)
        },
        cc.narrow(0, 0, total),
        None if extra is None else ce.narrow(0, 0, total),
    )


def _code_width(lo: int, hi: int) -> int:
    """Bits of one packed key column: codes run 0 (NULL) .. hi - lo + 1.
    Exact in Python ints (a float log2 rounds 2**k + 1 down to k bits once
    k passes 53, and has no value beyond 64 bits)."""
    return max(1, (int(hi) - int(lo) + 1).bit_length())


def _device_packable(key_cols: "Sequence[DeviceColumn]") -> bool:
    # integer dtypes only: the kernels load raw values by width, while
    # float keys go through the torch path's value-cast to int64; the
    # kernels take at most PACK_MAX_COLS columns per launch
    return len(key_cols) <= PACK_MAX_COLS and all(
        (not isinstance(c, StringDeviceColumn))
        and c.data.is_cuda
        and c.data.dtype in (torch.int64, torch.int32, torch.int16)
        and c.data.is_contiguous()
        for c in key_cols
    )


def pack_keys(
    key_cols: Sequence[DeviceColumn],
    mins: Optional[List[int]] = None,
    widths: Optional[List[int]] = None,
) -> Tuple[torch.Tensor, Optional[Dict[str, Any]]]:
    """Pack 1+ integer-like key columns into a single exact int64 key.

    Nulls get their own code (0); valid values are offset by 1.  Returns
    (keys, meta) where meta describes how to unpack; meta None means the
    single input column was used as-is (no nulls, int64).
    """
    if (
        len(key_cols) == 1
        and not isinstance(key_cols[0], StringDeviceColumn)
        and key_cols[0].data.dtype == torch.int64
        and key_cols[0].valid is None
        and mins is None
    ):
        return key_cols[0].data, None
    n = len(key_cols[0])
    for c in key_cols:
        if isinstance(c, StringDeviceColumn):
            raise NotImplementedError("string group keys not yet on device")
    # device fused path: one min/max pass + one pack pass (own kernels,
    # single host readback; memoized per tensor identity)
    if n > 0 and _device_packable(key_cols):
        kd = [c.data for c in key_cols]
        kv = [c.valid for c in key_cols]
        est = None
        if mins is None:
            comp_mins, comp_maxs, est = _key_stats_device(kd, kv, True)
            comp_widths = [
                _code_width(lo, hi) for lo, hi in zip(comp_mins, comp_maxs)
            ]
        else:
            comp_mins = list(mins)
            comp_widths = list(widths)
        total_bits = sum(comp_widths)
        if total_bits <= 63:
            shifts: List[int] = []
            shift = 0
            for w in reversed(comp_widths):
                shifts.append(shift)
                shift += w
            shifts.reverse()
            packed = get_ext().pack_columns(kd, kv, comp_mins, shifts)
            return packed, dict(
                mode="pack",
                mins=comp_mins,
                widths=comp_widths,
                nulls=[c.valid is not None for c in key_cols],
                device_pack=True,
                est=est,
            )
        # >63 bits: fall through to the torch dense re-encode below
    datas = []
    comp_mins = []
    comp_widths = []
    for i, c in enumerate(key_cols):
        d = c.data.to(torch.int64)
        if mins is None and c.data.is_floating_point() and d.numel() > 0:
            # the value cast is exact for integral floats only (both zeros
            # are 0); anything else would merge with its truncation, so
            # the caller takes its exact host path.  Single-rank only:
            # with rank-consistent ``mins`` (distributed partial merge) a
            # rank must not leave the collective plan on its own data, so
            # non-integral float keys are still truncated there (STATUS.md)
            exact = (d.to(c.data.dtype) == c.data) & (c.data.abs() < 2.0**62)
            if c.valid is not None:
                exact = exact | ~c.valid
            if not bool(exact.all().item()):
                raise NotImplementedError("non-integral float group keys")
        if mins is None:
            lo = int(d.min().item()) if d.numel() > 0 else 0
            hi = int(d.max().item()) if d.numel() > 0 else 0
        else:
            lo, hi = mins[i], mins[i] + (1 << widths[i]) - 2
        code = d - lo + 1  # 0 reserved for NULL
        if c.valid is not None:
            code = torch.where(c.valid, code, torch.zeros_like(code))
        datas.append(code)
        comp_mins.append(lo)
        if widths is None:
            w = _code_width(lo, hi)
            comp_widths.append(w)
        else:
            comp_widths.append(widths[i])
    total_bits = sum(comp_widths)
    if total_bits <= 63:
        packed = torch.zeros_like(datas[0])
        shift = 0
        for d, w in zip(reversed(datas), reversed(comp_widths)):
            packed = packed | (d << shift)
            shift += w
        return packed, dict(
            mode="pack",
            mins=comp_mins,
            widths=comp_widths,
            nulls=[c.valid is not None for c in key_cols],
        )
    # fallback: dense re-encode via torch.unique on stacked keys
    stacked = torch.stack(datas, dim=1)
    uniq, inverse = torch.unique(stacked, dim=0, return_inverse=True)
    return inverse.to(torch.int64), dict(
        mode="unique", uniq=uniq, mins=comp_mins
    )


def unpack_keys(
    packed: torch.Tensor,
    meta: Optional[Dict[str, Any]],
    key_cols: Sequence[DeviceColumn],
) -> List[DeviceColumn]:
    """Recover key columns (with nulls) from packed group keys."""
    if meta is None:
        return [DeviceColumn(packed, None, key_cols[0].pa_type)]
    res: List[DeviceColumn] = []
    if meta["mode"] == "pack":
        nulls = meta.get("nulls")
        shift = sum(meta["widths"])
        if packed.is_cuda and all(
            c.data.element_size() in (2, 4, 8) for c in key_cols
        ):
            ext = get_ext()
            for i, (c, lo, w) in enumerate(
                zip(key_cols, meta["mins"], meta["widths"])
            ):
                shift -= w
                has_nulls = nulls[i] if nulls is not None else True
                data, valid = ext.unpack_column(
                    packed, shift, w, lo, c.data.element_size(), has_nulls
                )
                res.append(
                    DeviceColumn(
                        data, valid if has_nulls else None, c.pa_type
                    )
                )
            return res
        for i, (c, lo, w) in enumerate(
            zip(key_cols, meta["mins"], meta["widths"])
        ):
            shift -= w
            code = (packed >> shift) & ((1 << w) - 1)
            data = (code - 1 + lo).to(c.data.dtype)
            if nulls is not None and not nulls[i]:
                res.append(DeviceColumn(data, None, c.pa_type))
                continue
            valid = code != 0
            res.append(
                DeviceColumn(
                    data, None if bool(valid.all().item()) else valid, c.pa_type
                )
            )
        return res
    uniq = meta["uniq"]
    for i, c in enumerate(key_cols):
        code = uniq[packed, i]
        valid = code != 0
        data = (code - 1 + meta["mins"][i]).to(c.data.dtype)
        res.append(
            DeviceColumn(
                data, None if bool(valid.all().item()) else valid, c.pa_type
            )
        )
    return res


def _agg_input(c, n: int) -> "torch.Tensor":
    """fp64 aggregation input for a column; string columns are only legal
    for COUNT (validity-only), so their data contribution is zeros."""
    if getattr(c, "is_string", False):
        return torch.zeros(
            n, dtype=torch.float64,
            device=c.offsets.device,
        )
    return c.data.to(torch.float64)


def _agg_inputs(
    df: HipDataFrame, aggs: List[Tuple[str, int, str]], n: int, device: Any
) -> Tuple["torch.Tensor", Optional["torch.Tensor"], "torch.Tensor", bool]:
    """Kernel inputs for ``aggs``: (vals [A, n] fp64, valids [A, n] or
    None, ops [A] int32, zero_copy).  ``zero_copy``: the single aggregate
    reads a null-free fp64 column in place.  No aggregates at all run as
    one COUNT."""
    if len(aggs) == 0:
        return (
            torch.zeros((1, n), dtype=torch.float64, device=device),
            None,
            torch.tensor([AGG_COUNT], dtype=torch.int32, device=device),
            False,
        )
    ops = torch.tensor(
        [op for _, op, _ in aggs], dtype=torch.int32, device=device
    )
    if len(aggs) == 1:
        c = df.col(aggs[0][0])
        if c.data.dtype == torch.float64 and c.valid is None:
            return c.data.unsqueeze(0), None, ops, True
    vals = torch.empty((len(aggs), n), dtype=torch.float64, device=device)
    valids: Optional[torch.Tensor] = None
    if any(df.col(c).valid is not None for c, _, _ in aggs):
        valids = torch.ones((len(aggs), n), dtype=torch.bool, device=device)
    for i, (cname, _, _) in enumerate(aggs):
        c = df.col(cname)
        vals[i] = _agg_input(c, n)
        if valids is not None and c.valid is not None:
            valids[i] = c.valid
    return vals, valids, ops, False


def _groupby_with_empty_key(
    df: HipDataFrame,
    keys: List[str],
    aggs: List[Tuple[str, int, str]],
    packed: "torch.Tensor",
    expected_groups: int,
) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor, None]:
    """``groupby_aggregate`` over a raw int64 key column that holds
    GB_EMPTY: the rows of that key are one group, reduced by the keyless
    kernel and appended to the hash aggregation of all other rows (which
    then meets the kernels' contract).  Off the hot path: it gathers both
    row sets."""
    device = packed.device
    is_empty_key = packed == GB_EMPTY
    rows = is_empty_key.nonzero(as_tuple=True)[0]
    rest = (~is_empty_key).nonzero(as_tuple=True)[0]
    vals, _ = global_aggregate(df.gather_rows(rows), aggs)
    if rest.numel() > 0:
        out_keys, out_aggs, out_count, _ = groupby_aggregate(
            df.gather_rows(rest), keys, aggs, expected_groups=expected_groups
        )
    else:
        out_keys = torch.empty(0, dtype=torch.int64, device=device)
        out_count = torch.empty(0, dtype=torch.int64, device=device)
        out_aggs = {
            oname: torch.empty(0, dtype=torch.float64, device=device)
            for _, _, oname in aggs
        }
    one = lambda v, dt: torch.tensor([v], dtype=dt, device=device)  # noqa: E731
    return (
        torch.cat([out_keys, one(GB_EMPTY, torch.int64)]),
        {
            oname: torch.cat([out_aggs[oname], one(vals[oname], torch.float64)])
            for _, _, oname in aggs
        },
        torch.cat([out_count, one(int(rows.numel()), torch.int64)]),
        None,
    )


def groupby_aggregate(
    df: HipDataFrame,
    keys: List[str],
    aggs: List[Tuple[str, int, str]],  # (input col, op, output name)
    expected_groups: Optional[int] = None,
    pack_mins: Optional[List[int]] = None,
    pack_widths: Optional[List[int]] = None,
) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor, Optional[Dict[str, Any]]]:
    """Hash group-by: returns (group_keys_packed, {out_name: fp64 values},
    group_row_counts, pack_meta).

    Reference comparator: the groupby-aggregate SQL path
    (``fugue/execution/execution_engine.py:889`` + qpd/duckdb/dask-sql).
    """
    n = df.count()
    device = df.col(keys[0]).data.device if keys else torch.device(df.device)
    key_cols = [df.col(k) for k in keys]
    packed, meta = pack_keys(key_cols, mins=pack_mins, widths=pack_widths)
    vals, valids, ops, zero_copy = _agg_inputs(df, aggs, n, device)
    if _is_cpu(packed):
        return _groupby_aggregate_cpu(packed, aggs, df, meta)
    ext = get_ext()
    key_range = None
    key_stats = None
    if meta is None and n > 0:
        # raw int64 keys are the only ones that can equal GB_EMPTY (packed
        # and re-encoded keys are >= 0); the kernels' contract excludes it
        # (csrc/relational.h), and the minimum of the memoized key stats
        # is the presence test.  Without ``expected_groups`` (every engine
        # call) this is the readback the sizing needs anyway; a caller
        # that passes ``expected_groups`` now pays one stats launch set
        # and host sync per key tensor (memoized).  ``key_range`` stays
        # unset for such callers on purpose: they keep the speculative
        # int32 narrowing, which tests/test_gb_staged_gpu.py reaches
        # exactly this way
        key_stats = _key_stats_device([packed], [None], True)
        if key_stats[0][0] == GB_EMPTY:
            return _groupby_with_empty_key(
                df, keys, aggs, packed, expected_groups or key_stats[2]
            )
    if expected_groups is None:
        # sample-based distinct-count estimate (Chao83: D ≈ d + f1²/(2·f2),
        # robust when the sample is mostly singletons — a linear scale-up
        # would estimate ~n for any high-ish cardinality).  Own kernel +
        # single host readback; for meta-None keys the same readback
        # carries min/max so the int32-narrowing decision needs no
        # speculative overflow check.
        if key_stats is not None:
            key_lo, key_hi, expected_groups = key_stats
            key_range = (key_lo[0], key_hi[0])
        elif n > 0:
            expected_groups = (meta or {}).get("est")
            if expected_groups is None:
                _, _, expected_groups = _key_stats_device(
                    [packed], [None], False
                )
        else:
            expected_groups = 1
    sum_count_only = all(op in (AGG_SUM, AGG_COUNT) for _, op, _ in aggs)
    # the partitioned path aggregates in a per-partition LDS table that
    # holds at most GB_LDS_MAX_AGGS aggregates; wider calls go to the HBM
    # table, like every other shape that path does not take
    partitioned = (
        expected_groups > 100_000
        and valids is None
        and sum_count_only
        and vals.shape[0] <= GB_LDS_MAX_AGGS
    )
    if not partitioned:
        use_lds = expected_groups <= 100_000 and sum_count_only
        tkeys, gaggs, gcount = ext.gb_aggregate(
            keys=packed, vals=vals, valids=valids, ops=ops,
            tsize=_table_size(expected_groups), use_lds=use_lds,
        )
    else:
        # high cardinality: 2-phase partitioned aggregation
        knobs = _GbKnobs.from_env()
        plan = _plan_partitioned(
            n, expected_groups, len(aggs),
            zero_copy and aggs[0][1] == AGG_SUM,
            None if meta is None else sum(meta["widths"]),
            key_range, knobs,
        )
        # the dense gate and the scatter tile are part of the memo key so
        # an in-process A/B keeps one entry per side
        # the bin knobs shape the dense layout (tile scatter only)
        bins = (1, 0, 0, 0)
        if plan.dense_ok and plan.tile > 0 and knobs.replay_bin_parts > 1:
            bins = (knobs.replay_bin_parts, knobs.bin_slots, knobs.bin_chunk,
                    knobs.replay_compact)
        lkey = (
            packed.data_ptr(), n, plan.num_parts, plan.tsize, plan.narrow,
            plan.dense_ok, plan.tile,
        ) + bins
        ent = _layout_get(lkey) if plan.reuse else None
        if isinstance(ent, _DenseLayout):
            # dense replay: groups, counts, output order and every row's
            # group were fixed when the layout was recorded; the step is
            # the value scatter + one LDS add per row.  The SAME cached
            # out_keys/out_count tensors are returned every call on
            # purpose: columns are immutable, and a stable key tensor
            # lets the identity-memoized key stats of a downstream join
            # hit instead of re-running.
            if ent.tile_start is not None:
                out_sum = ext.gb_replay_compact(
                    vals=vals,
                    rel=ent.rel if ent.rel is not None else ent.gid,
                    rank=ent.rank,
                    tile_start=ent.tile_start, tile_delta=ent.tile_delta,
                    bin_offsets=ent.bin_offsets,
                    bin_group_base=ent.bin_group_base,
                    bin_chunk_base=ent.bin_chunk_base,
                    total_chunks=ent.bin_chunks, n_groups=ent.n_groups,
                    chunk=ent.bin_chunk, slots=ent.bin_slots, tile=ent.tile,
                )
            elif ent.bin_parts > 1:
                out_sum = ext.gb_replay_binned(
                    vals=vals, gid=ent.gid, rank=ent.rank, dst=ent.dst,
                    bin_offsets=ent.bin_offsets,
                    bin_group_base=ent.bin_group_base,
                    bin_chunk_base=ent.bin_chunk_base,
                    total_chunks=ent.bin_chunks, n_groups=ent.n_groups,
                    chunk=ent.bin_chunk, slots=ent.bin_slots, tile=ent.tile,
                )
            else:
                out_sum = ext.gb_replay_dense(
                    vals=vals, gid=ent.gid, offsets=ent.offsets,
                    group_base=ent.group_base, n_groups=ent.n_groups,
                    chunk=plan.ag_chunk, slots=knobs.dense_slots,
                    tile=ent.tile, rank=ent.rank, dst=ent.dst, pos=ent.pos,
                )
            ent.hits += 1
            return ent.out_keys, {aggs[0][2]: out_sum}, ent.out_count, meta
        if ent is not None:
            # replay: fresh values through the recorded layout — phase 1
            # (hist) and the key scatter are skipped entirely
            tkeys, gaggs, gcount = ext.gb_aggregate_replay(
                pkeys=ent.pkeys, pos=ent.pos, vals=vals, ops=ops,
                num_parts=plan.num_parts, tsize=plan.tsize,
                agg_chunk=plan.ag_chunk,
            )
        elif plan.reuse and _layout_second_sight(lkey, packed):
            # second sight of these keys: record the layout (recording
            # uses the slower simple scatter; only repeat keys justify it)
            tkeys, gaggs, gcount, pkeys, pos = _run_partitioned(
                ext, packed, vals, ops, plan, record=True
            )
            new_ent = None
            if plan.dense_ok:
                new_ent = _prepare_dense_layout(
                    ext, packed, pkeys, pos, plan.num_parts, plan.tile,
                    *bins
                )
            if new_ent is None:
                if plan.narrow == 1:
                    pkeys = pkeys.to(torch.int32)
                new_ent = _PlainLayout(weakref.ref(packed), pkeys, pos)
            _layout_put(lkey, new_ent)
        else:
            tkeys, gaggs, gcount, _, _ = _run_partitioned(
                ext, packed, vals, ops, plan
            )
    if len(aggs) == 0:
        gaggs = torch.empty((0, 0), dtype=torch.float64, device=device)
    out_keys, out_aggs, out_count, _ = _compact_groups(
        ext, tkeys, gcount, gaggs, aggs
    )
    return out_keys, out_aggs, out_count, meta


def _groupby_aggregate_cpu(
    packed: torch.Tensor,
    aggs: List[Tuple[str, int, str]],
    df: HipDataFrame,
    meta: Optional[Dict[str, Any]],
) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor, Optional[Dict[str, Any]]]:
    import pandas as pd

    data: Dict[str, Any] = {"__key": packed.numpy()}
    n_rows = packed.numel()
    for cname, op, oname in aggs:
        c = df.col(cname)
        v = _agg_input(c, int(n_rows)).numpy()
        if c.valid is not None:
            v = np.where(c.valid.numpy(), v, np.nan)
        data[oname] = v
    pdf = pd.DataFrame(data)
    g = pdf.groupby("__key", sort=False)
    out_count = g.size()
    out_keys = torch.from_numpy(out_count.index.to_numpy().astype(np.int64))
    count_t = torch.from_numpy(out_count.to_numpy().astype(np.int64))
    out_aggs: Dict[str, torch.Tensor] = {}
    for cname, op, oname in aggs:
        if op == AGG_SUM:
            s = g[oname].sum(min_count=0)
        elif op == AGG_MIN:
            s = g[oname].min()
        elif op == AGG_MAX:
            s = g[oname].max()
        elif op == AGG_COUNT:
            s = g[oname].count().astype("float64")
        else:
            raise FugueBug(f"op {op}")
        out_aggs[oname] = torch.from_numpy(s.to_numpy().astype("float64"))
    return out_keys, out_aggs, count_t, meta


def _hash_join_indices_cpu(
    probe_keys: torch.Tensor,
    build_keys: torch.Tensor,
    how: str,
    probe_h2: Optional[torch.Tensor] = None,
    build_h2: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    import pandas as pd

    p = pd.DataFrame({"k": probe_keys.numpy()})
    b = pd.DataFrame({"k": build_keys.numpy()})
    if probe_h2 is not None:
        p["k2"] = probe_h2.numpy()
        b["k2"] = build_h2.numpy()
    on = list(p.columns)
    p["pi"] = np.arange(len(p), dtype=np.int64)
    b["bi"] = np.arange(len(b), dtype=np.int64)
    if how == "inner":
        m = p.merge(b, on=on, how="inner")
        return (
            torch.from_numpy(m["pi"].to_numpy()),
            torch.from_numpy(m["bi"].to_numpy()),
        )
    if how == "left":
        m = p.merge(b, on=on, how="left")
        bi = m["bi"].fillna(-1).astype("int64")
        return (
            torch.from_numpy(m["pi"].to_numpy()),
            torch.from_numpy(bi.to_numpy()),
        )
    if how == "semi":
        m = p.merge(b.drop_duplicates(on), on=on, how="inner")
        return (
            torch.from_numpy(m["pi"].to_numpy()),
            torch.from_numpy(m["bi"].to_numpy()),
        )
    if how == "anti":
        m = p.merge(b.drop_duplicates(on), on=on, how="left")
        m = m[m["bi"].isna()]
        return (
            torch.from_numpy(m["pi"].to_numpy()),
            torch.from_numpy(np.full(len(m), -1, dtype=np.int64)),
        )
    raise FugueBug(f"unsupported join mode {how}")


class HashCollisionError(RuntimeError):
    """h1 collision between distinct keys detected (exact fallback path
    is taken by the caller)."""


_H2_SEED = 0x5851F42D4C957F2D


def global_aggregate(
    df: HipDataFrame,
    aggs: List[Tuple[str, int, str]],  # (input col, op, output name)
) -> Tuple[Dict[str, float], Dict[str, int]]:
    """Keyless whole-column reductions: returns ({name: value},
    {name: non-null count}).  SUM wave-reduction runs on the f64 matrix
    core (``v_mfma_f64_16x16x4_f64`` — see ``reduce_cols_kernel``)."""
    n = df.count()
    out_vals: Dict[str, float] = {}
    out_counts: Dict[str, int] = {}
    if len(aggs) == 0:
        return out_vals, out_counts
    c0 = df.col(aggs[0][0])
    if _is_cpu(c0.data if not getattr(c0, "is_string", False) else c0.offsets):
        import pandas as pd

        for cname, op, oname in aggs:
            c = df.col(cname)
            v = _agg_input(c, n).numpy().astype("float64")
            if c.valid is not None:
                v = np.where(c.valid.numpy(), v, np.nan)
            sr = pd.Series(v)
            cnt = int(sr.notna().sum())
            if op == AGG_SUM:
                val = float(sr.sum()) if cnt > 0 else 0.0
            elif op == AGG_MIN:
                val = float(sr.min()) if cnt > 0 else float("inf")
            elif op == AGG_MAX:
                val = float(sr.max()) if cnt > 0 else float("-inf")
            else:  # AGG_COUNT
                val = float(cnt)
            out_vals[oname] = val
            out_counts[oname] = cnt
        return out_vals, out_counts
    ext = get_ext()
    device = torch.device(df.device)
    n_aggs = len(aggs)
    vals = torch.empty((n_aggs, max(n, 1)), dtype=torch.float64, device=device)
    valids: Optional[torch.Tensor] = None
    if any(df.col(c).valid is not None for c, _, _ in aggs):
        valids = torch.ones((n_aggs, max(n, 1)), dtype=torch.bool, device=device)
    kernel_ops = []
    for i, (cname, op, _) in enumerate(aggs):
        c = df.col(cname)
        vals[i, :n] = _agg_input(c, n)
        if valids is not None:
            if c.valid is not None:
                valids[i, :n] = c.valid
            if n < vals.shape[1]:
                valids[i, n:] = False
        kernel_ops.append(AGG_SUM if op == AGG_COUNT else op)
    if n == 0 and valids is None:
        valids = torch.zeros((n_aggs, 1), dtype=torch.bool, device=device)
    ops_t = torch.tensor(kernel_ops, dtype=torch.int32, device=device)
    out, cnt = ext.reduce_columns(vals[:, :max(n, 1)], valids, ops_t)
    out_h = out.cpu().tolist()
    cnt_h = cnt.cpu().tolist()
    for i, (_, op, oname) in enumerate(aggs):
        out_counts[oname] = int(cnt_h[i])
        out_vals[oname] = (
            float(cnt_h[i]) if op == AGG_COUNT else float(out_h[i])
        )
    return out_vals, out_counts


def groupby_aggregate_hashed(
    df: HipDataFrame,
    keys: List[str],
    aggs: List[Tuple[str, int, str]],
) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor]:
    """Group-by for key tuples that can't be packed exactly (string keys):
    groups on a 64-bit hash with an independent second hash verified
    in-kernel.  An h1 collision between distinct keys raises
    :class:`HashCollisionError` (caller falls back to the exact host
    path); the undetected-failure probability is that of a full 128-bit
    collision (~n²·2⁻¹²⁹).

    Returns (representative_row_indices, {out_name: fp64}, counts).
    """
    key_cols = [df.col(k) for k in keys]
    h1 = hash_rows(key_cols)
    h2 = hash_rows(key_cols, seed=_H2_SEED)
    n = df.count()
    if _is_cpu(h1):
        import pandas as pd

        pdf = pd.DataFrame({"__h1": h1.numpy(), "__h2": h2.numpy()})
        pdf["__idx"] = np.arange(n, dtype=np.int64)
        for cname, op, oname in aggs:
            c = df.col(cname)
            v = _agg_input(c, n).numpy()
            if c.valid is not None:
                v = np.where(c.valid.numpy(), v, np.nan)
            pdf[oname] = v
        g = pdf.groupby("__h1", sort=False)
        if int((g["__h2"].nunique() > 1).sum()) > 0:
            raise HashCollisionError("h1 collision on string keys")
        reps = torch.from_numpy(g["__idx"].first().to_numpy())
        counts = torch.from_numpy(g.size().to_numpy().astype(np.int64))
        out: Dict[str, torch.Tensor] = {}
        for cname, op, oname in aggs:
            if op == AGG_SUM:
                sr = g[oname].sum(min_count=0)
            elif op == AGG_MIN:
                sr = g[oname].min()
            elif op == AGG_MAX:
                sr = g[oname].max()
            elif op == AGG_COUNT:
                sr = g[oname].count().astype("float64")
            else:
                raise FugueBug(f"op {op}")
            out[oname] = torch.from_numpy(sr.to_numpy().astype("float64"))
        return reps, out, counts
    ext = get_ext()
    device = h1.device
    n_aggs = len(aggs)
    if n_aggs > 0:
        vals = torch.empty((n_aggs, n), dtype=torch.float64, device=device)
        valids: Optional[torch.Tensor] = None
        if any(df.col(c).valid is not None for c, _, _ in aggs):
            valids = torch.ones((n_aggs, n), dtype=torch.bool, device=device)
        for i, (cname, op, _) in enumerate(aggs):
            c = df.col(cname)
            vals[i] = _agg_input(c, n)
            if valids is not None and c.valid is not None:
                valids[i] = c.valid
        ops = torch.tensor(
            [op for _, op, _ in aggs], dtype=torch.int32, device=device
        )
    else:
        vals = torch.zeros((1, n), dtype=torch.float64, device=device)
        valids = None
        ops = torch.tensor([AGG_COUNT], dtype=torch.int32, device=device)
    # distinct estimate over h1 (own kernel, one readback, memoized)
    _, _, expected = _key_stats_device([h1], [None], False)
    tsize = _next_pow2(max(16, int(expected * 2)))
    tkeys, gaggs, gcount = ext.gb_aggregate(
        h1, vals, valids, ops, tsize, expected <= 100_000
    )
    rep, th2, conflict = ext.gb_mark_reps(h1, h2, tkeys, tsize)
    if int(conflict.item()) > 0:
        raise HashCollisionError("h1 collision on string keys")
    _, out_aggs, counts, reps = _compact_groups(
        ext, tkeys, gcount, gaggs, aggs, extra=rep
    )
    return reps, out_aggs, counts


def distinct_reps(h1: torch.Tensor, h2: torch.Tensor) -> torch.Tensor:
    """One representative row index per distinct (h1, h2) row-content key
    (raises HashCollisionError on an h1 collision — caller falls back)."""
    n = int(h1.numel())
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=h1.device)
    if _is_cpu(h1):
        import pandas as pd

        pdf = pd.DataFrame({"h1": h1.numpy(), "h2": h2.numpy()})
        pdf["idx"] = np.arange(n, dtype=np.int64)
        g = pdf.groupby("h1", sort=False)
        if int((g["h2"].nunique() > 1).sum()) > 0:
            raise HashCollisionError("h1 collision in distinct")
        return torch.from_numpy(g["idx"].first().to_numpy())
    ext = get_ext()
    device = h1.device
    _, _, expected = _key_stats_device([h1], [None], False)
    tsize = _next_pow2(max(16, int(expected * 2)))
    vals = torch.zeros((1, max(n, 1)), dtype=torch.float64, device=device)
    ops = torch.tensor([AGG_COUNT], dtype=torch.int32, device=device)
    tkeys, _gaggs, _gcount = ext.gb_aggregate(
        h1, vals, None, ops, tsize, expected <= 100_000
    )
    rep, _th2, conflict = ext.gb_mark_reps(h1, h2, tkeys, tsize)
    if int(conflict.item()) > 0:
        raise HashCollisionError("h1 collision in distinct")
    ck, cc, _ca, _ce, bases = ext.gb_compact(
        tkeys, rep,
        torch.empty((0, 0), dtype=torch.float64, device=device), None,
    )
    return cc.narrow(0, 0, int(bases[-1].item()))


@dataclass
class _JoinBuild:
    """Chained table of one build-key tensor.  ``dup`` is the duplicate
    flag as a host int once some caller has read ``dup_dev`` back (it
    rides in that caller's own readback), None until then."""

    heads: torch.Tensor
    nxt: torch.Tensor
    tsize: int
    dup_dev: torch.Tensor
    dup: Optional[int] = None


def _join_build_table(build_keys: torch.Tensor, stats: Any = None) -> _JoinBuild:
    """The chained join table of ``build_keys``, from _JOIN_BUILD_MEMO when
    this very tensor (same bytes, still alive) was built before."""
    use_memo = os.environ.get("FUGUE_JOIN_BUILD_MEMO", "1") != "0"
    key = (
        build_keys.data_ptr(),
        build_keys.numel(),
        str(build_keys.dtype),
        str(build_keys.device),
    )
    if use_memo:
        hit = _JOIN_BUILD_MEMO.get(key)
        if hit is not None:
            ref, tab = hit
            if ref() is not None:
                if stats is not None:
                    stats.add("join.build_memo_hit")
                return tab
            del _JOIN_BUILD_MEMO[key]
        # tables of dead key tensors (join inputs computed per call) go
        # before the new one is allocated: they never push a persistent
        # table out, and their memory is free for this build
        for k in [k for k, (r, _) in _JOIN_BUILD_MEMO.items() if r() is None]:
            del _JOIN_BUILD_MEMO[k]
    nb = int(build_keys.numel())
    tsize = _next_pow2(max(16, nb * 2))
    heads, nxt, dup = get_ext().join_build(build_keys, tsize)
    tab = _JoinBuild(heads, nxt, tsize, dup)
    if use_memo:
        if stats is not None:
            stats.add("join.build_memo_miss")
        nbytes = 4 * (int(heads.numel()) + int(nxt.numel()))
        if nbytes <= _JOIN_BUILD_MEMO_MAX_BYTES:
            if len(_JOIN_BUILD_MEMO) >= _JOIN_BUILD_MEMO_CAP:
                _JOIN_BUILD_MEMO.pop(next(iter(_JOIN_BUILD_MEMO)))
            _JOIN_BUILD_MEMO[key] = (weakref.ref(build_keys), tab)
    return tab


def join_unique_select(
    probe_keys: torch.Tensor,
    build_keys: torch.Tensor,
    pred: Optional[Tuple[int, Tuple[int, Any], Tuple[int, Any]]],
    out_specs: List[Tuple[int, torch.Tensor]],
    stats: Any = None,
) -> Optional[List[torch.Tensor]]:
    """Inner join on exact int64 keys against UNIQUE build keys, with a
    residual comparison and a projection, in one kernel
    (``ext.join_unique_select``): the projected columns, narrowed to the
    surviving rows, in no defined order.  None when the build keys hold a
    duplicate — the caller takes the count+emit join.

    The walk is speculative on first sight of a build tensor: the
    duplicate flag comes back in the same single readback as the row
    total.  A table from _JOIN_BUILD_MEMO knows its flag already."""
    tab = _join_build_table(build_keys, stats)
    if tab.dup:
        return None
    outs = get_ext().join_unique_select(
        probe_keys, build_keys, tab.heads, tab.nxt, pred, out_specs
    )
    if tab.dup is None:
        flags = torch.cat([tab.dup_dev.reshape(1), outs[-1].reshape(1)]).cpu()
        tab.dup = int(flags[0].item())
        total = int(flags[1].item())
        if tab.dup:
            return None
    else:
        total = int(outs[-1].item())  # the step's only readback
    return [t.narrow(0, 0, total) for t in outs[:-1]]


def hash_join_indices(
    probe_keys: torch.Tensor,
    build_keys: torch.Tensor,
    how: str,
    probe_h2: Optional[torch.Tensor] = None,
    build_h2: Optional[torch.Tensor] = None,
    stats: Any = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Join on exact int64 keys; returns (probe_idx, build_idx) where
    build_idx == -1 marks no-match rows (left/anti).

    ``how`` ∈ {inner, left, semi, anti}.  CDNA4 chained-bucket hash join
    (replaces the reference's delegation to pandas/duckdb/spark joins,
    SURVEY.md §2.3 row "join ×9 types").
    """
    if _is_cpu(probe_keys):
        return _hash_join_indices_cpu(
            probe_keys, build_keys, how, probe_h2, build_h2
        )
    ext = get_ext()
    if how not in ("inner", "left", "semi", "anti"):
        raise FugueBug(f"unsupported join mode {how}")
    nb = int(build_keys.numel())
    import os as _os_j

    skip_unique_walk = False
    if probe_h2 is None and _os_j.environ.get("FUGUE_JOIN_OA", "0") == "1":
        # open-addressed unique join (16B key+idx entries, ~1 random
        # cache line per probe).  MEASURED SLOWER than chains on q3
        # (4.36 vs 4.22 ms/step): the doubled table footprint falls out
        # of the 256MB Infinity Cache while the chained layout fits —
        # kept env-gated for small-build workloads.  Build duplicates /
        # sentinel keys fall back to the chained join below.
        np_ = int(probe_keys.numel())
        out_p, out_b, matched, flags = ext.join_open_unique(
            probe_keys, build_keys, how == "left", how != "left",
            how == "anti",
        )
        if how == "left":
            fl = flags.cpu()
            if int(fl[0]) == 0 and int(fl[1]) == 0:
                return out_p, out_b
            skip_unique_walk = int(fl[0]) != 0 and int(fl[1]) == 0
        else:
            cols = [None] if how == "anti" else [None, out_b]
            outs = ext.compact_columns_cap(matched, cols)
            vals = torch.cat([flags, outs[-1].reshape(1)]).cpu()
            if int(vals[0]) == 0 and int(vals[1]) == 0:
                total = int(vals[2])
                if how == "anti":
                    pi = outs[0].narrow(0, 0, total)
                    return pi, torch.full_like(pi, -1)
                return (
                    outs[0].narrow(0, 0, total),
                    outs[1].narrow(0, 0, total),
                )
            # dup with no sentinel: the chained unique walk would fail
            # the same way — go straight to the duplicate-emit path
            skip_unique_walk = int(vals[0]) != 0 and int(vals[1]) == 0

    # a repeated build tensor takes its table and its duplicate flag from
    # _JOIN_BUILD_MEMO: no build kernels, and no flag in the readback
    tab = _join_build_table(build_keys, stats)
    tsize, heads, nxt = tab.tsize, tab.heads, tab.nxt
    mode = {"inner": 0, "left": 1, "semi": 2, "anti": 3}[how]
    if tab.dup:
        skip_unique_walk = True  # known duplicates: count+emit directly

    if not skip_unique_walk and _os_j.environ.get(
        "FUGUE_JOIN_UNIQUE", "1"
    ) != "0":
        # unique build keys (≤1 match per probe): ONE chain walk writes
        # the match index positionally; inner/semi/anti then compact
        # with the block-scan compaction kernel (no global-cursor
        # contention, no second walk).  The walk is SPECULATIVE: it runs
        # before the duplicate flag is read so the dup check, the
        # compaction total and the emit all resolve in ONE host sync
        # (dup build keys are rare — dim joins and groupby outputs are
        # unique — and merely discard this walk).
        np_ = int(probe_keys.numel())
        out_p, out_b, _cur, matched = ext.join_emit_unique(
            probe_keys, build_keys, probe_h2, build_h2, heads, nxt, 1,
            how == "left", how != "left", how == "anti",
        )
        if how == "left":
            if tab.dup is None:
                tab.dup = int(tab.dup_dev.item())
            if tab.dup == 0:
                return out_p, out_b
        else:
            # matched mask came out of the walk kernel itself;
            # None column = "emit the row index" (no arange materialized)
            cols = [None] if how == "anti" else [None, out_b]
            outs = ext.compact_columns_cap(matched, cols)
            if tab.dup is None:
                flags = torch.cat(
                    [tab.dup_dev.reshape(1), outs[-1].reshape(1)]
                ).cpu()
                tab.dup = int(flags[0].item())
                total = int(flags[1].item())
            else:
                total = int(outs[-1].item())
            if tab.dup == 0:
                if how == "anti":
                    pi = outs[0].narrow(0, 0, total)
                    return pi, torch.full_like(pi, -1)
                return (
                    outs[0].narrow(0, 0, total),
                    outs[1].narrow(0, 0, total),
                )
    # duplicate build keys: 2-pass count+prefix+emit; a 3-pass
    # total+chunked-reservation variant (ext.join_pairs) measured
    # SLOWER — the random chain walk dominates, not the streaming
    # counts/cumsum (profiles/NOTES.md)
    counts = ext.join_count(
        probe_keys, build_keys, probe_h2, build_h2, heads, nxt, tsize
    )
    counts64 = counts.to(torch.int64)
    if how == "inner":
        out_counts = counts64
    elif how == "left":
        out_counts = torch.clamp(counts64, min=1)
    elif how == "semi":
        out_counts = (counts64 > 0).to(torch.int64)
    else:
        out_counts = (counts64 == 0).to(torch.int64)
    offsets = torch.zeros_like(out_counts)
    if out_counts.numel() > 1:
        torch.cumsum(out_counts[:-1], 0, out=offsets[1:])
    total = int(out_counts.sum().item())
    out_p, out_b = ext.join_emit(
        probe_keys, build_keys, probe_h2, build_h2, heads, nxt, tsize,
        offsets, total, mode
    )
    return out_p, out_b


def mark_matched_build_rows(
    probe_keys: torch.Tensor,
    build_keys: torch.Tensor,
    probe_h2: Optional[torch.Tensor] = None,
    build_h2: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    if _is_cpu(probe_keys):
        if probe_h2 is None:
            bk = build_keys.numpy()
            matched = np.isin(bk, np.unique(probe_keys.numpy()))
            return torch.from_numpy(matched)
        import pandas as pd

        b = pd.DataFrame(
            {"k": build_keys.numpy(), "k2": build_h2.numpy()}
        )
        pset = pd.DataFrame(
            {"k": probe_keys.numpy(), "k2": probe_h2.numpy()}
        ).drop_duplicates()
        pset["__m"] = True
        m = b.merge(pset, on=["k", "k2"], how="left")
        return torch.from_numpy(m["__m"].notna().to_numpy())
    ext = get_ext()
    nb = int(build_keys.numel())
    tab = _join_build_table(build_keys)
    return ext.join_mark_build(
        probe_keys, build_keys, probe_h2, build_h2, tab.heads, tab.nxt,
        tab.tsize, nb
    )


def sort_indices(
    df: HipDataFrame, by: List[str], ascending: List[bool]
) -> torch.Tensor:
    """Stable multi-key sort permutation (rocPRIM radix sort via torch,
    least-significant key first)."""
    n = df.count()
    device = torch.device(df.device)
    perm = torch.arange(n, dtype=torch.int64, device=device)
    for name, asc in reversed(list(zip(by, ascending))):
        c = df.col(name)
        if isinstance(c, StringDeviceColumn):
            raise NotImplementedError("string sort keys not yet on device")
        vals = c.data.index_select(0, perm)
        if c.valid is not None:
            # nulls last regardless of direction (pandas na_position
            # default): sentinel is +extreme for asc, -extreme for desc
            if vals.is_floating_point():
                sentinel = float("inf") if asc else float("-inf")
            else:
                info = torch.iinfo(vals.dtype)
                sentinel = info.max if asc else info.min
            v = c.valid.index_select(0, perm)
            vals = torch.where(v, vals, torch.full_like(vals, sentinel))
        idx = torch.argsort(vals, stable=True, descending=not asc)
        perm = perm.index_select(0, idx)
    return perm


def sort_perm_keys_first(
    df: HipDataFrame,
    key_tensor: torch.Tensor,
    presort: List[str],
    ascending: List[bool],
) -> torch.Tensor:
    """Stable sort permutation by (key_tensor, presort columns): the
    int64 key tensor is the most significant key.  Used for string-keyed
    grouping where the key identity is a 64-bit row hash (strings have
    no device ordering; group boundaries only need identity)."""
    n = df.count()
    device = key_tensor.device
    perm = torch.arange(n, dtype=torch.int64, device=device)
    for name, asc in reversed(list(zip(presort, ascending))):
        c = df.col(name)
        if isinstance(c, StringDeviceColumn):
            raise NotImplementedError("string presort keys not on device")
        vals = c.data.index_select(0, perm)
        if c.valid is not None:
            if vals.is_floating_point():
                sentinel = float("inf") if asc else float("-inf")
            else:
                info = torch.iinfo(vals.dtype)
                sentinel = info.max if asc else info.min
            v = c.valid.index_select(0, perm)
            vals = torch.where(v, vals, torch.full_like(vals, sentinel))
        idx = torch.argsort(vals, stable=True, descending=not asc)
        perm = perm.index_select(0, idx)
    kv = key_tensor.index_select(0, perm)
    idx = torch.argsort(kv, stable=True)
    return perm.index_select(0, idx)


def group_boundaries(sorted_keys: torch.Tensor) -> torch.Tensor:
    """Start offsets of each group in a key-sorted int64 tensor."""
    n = sorted_keys.numel()
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=sorted_keys.device)
    change = torch.ones(n, dtype=torch.bool, device=sorted_keys.device)
    change[1:] = sorted_keys[1:] != sorted_keys[:-1]
    return change.nonzero(as_tuple=True)[0]


# ------------------------------------------------------------------ #
# segmented rank over a sorted permutation                             #
# ------------------------------------------------------------------ #
RANK_KINDS = {"row_number": 0, "rank": 1, "dense_rank": 2}


def sort_indices_exact(
    df: HipDataFrame,
    by: List[str],
    ascending: List[bool],
    na_position: str = "last",
    key_tensor: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Stable multi-key sort permutation like :func:`sort_indices`, but
    nulls are placed by a separate stable pass over the validity flag
    instead of a sentinel value: ``INT64_MAX``/``±inf`` stay distinct
    from null and both ``na_position`` values work.  NaN counts as null
    (pandas semantics).  ``key_tensor``, when given, is an int64 tensor
    in row order that becomes the most significant (ascending) key."""
    if na_position not in ("first", "last"):
        raise ValueError(f"invalid na_position {na_position!r}")
    n = df.count()
    device = (
        key_tensor.device if key_tensor is not None else torch.device(df.device)
    )
    perm = torch.arange(n, dtype=torch.int64, device=device)
    for name, asc in reversed(list(zip(by, ascending))):
        c = df.col(name)
        if isinstance(c, StringDeviceColumn):
            raise NotImplementedError("string sort keys not yet on device")
        vals = c.data.index_select(0, perm)
        if vals.dtype == torch.bool:
            vals = vals.to(torch.uint8)
        isnull: Optional[torch.Tensor] = None
        if c.valid is not None:
            isnull = ~c.valid.index_select(0, perm)
        if vals.is_floating_point():
            nan = torch.isnan(vals)
            if bool(nan.any().item()):
                isnull = nan if isnull is None else (isnull | nan)
        if isnull is not None:
            # values under a null must not influence the order
            vals = torch.where(isnull, torch.zeros_like(vals), vals)
        idx = torch.argsort(vals, stable=True, descending=not asc)
        perm = perm.index_select(0, idx)
        if isnull is not None:
            flag = isnull.index_select(0, idx).to(torch.uint8)
            if na_position == "first":
                flag = 1 - flag
            idx = torch.argsort(flag, stable=True)
            perm = perm.index_select(0, idx)
    if key_tensor is not None:
        kv = key_tensor.index_select(0, perm)
        idx = torch.argsort(kv, stable=True)
        perm = perm.index_select(0, idx)
    return perm


def _order_col_parts(c: Any) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(8-byte data, validity) of an order column given as a
    ``DeviceColumn`` or a ``(data, valid)`` pair; narrower dtypes widen."""
    if isinstance(c, StringDeviceColumn):
        raise NotImplementedError("string order columns not on device")
    if isinstance(c, DeviceColumn):
        data, valid = c.data, c.valid
    else:
        data, valid = c
    if data.is_floating_point():
        data = data.to(torch.float64)
    else:
        data = data.to(torch.int64)
    return data.contiguous(), (None if valid is None else valid.contiguous())


def _segment_flags_cpu(
    perm: torch.Tensor,
    pkeys: torch.Tensor,
    order_cols: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]],
) -> Tuple[torch.Tensor, torch.Tensor]:
    n = perm.numel()
    ks = pkeys.index_select(0, perm)
    head = torch.ones(n, dtype=torch.bool)
    head[1:] = ks[1:] != ks[:-1]
    peer = head.clone()
    for data, valid in order_cols:
        v = data.index_select(0, perm)
        eqv = v[1:] == v[:-1]
        if v.is_floating_point():
            eqv = eqv | (torch.isnan(v[1:]) & torch.isnan(v[:-1]))
        if valid is not None:
            ok = valid.index_select(0, perm)
            eqv = torch.where(ok[1:] & ok[:-1], eqv, ok[1:] == ok[:-1])
        peer[1:] |= ~eqv
    return head, peer


def _segmented_rank_cpu(
    perm: torch.Tensor,
    pkeys: torch.Tensor,
    order_cols: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]],
    kind: int,
) -> torch.Tensor:
    """Ranks per SORTED position (not yet scattered to row order)."""
    n = perm.numel()
    head, peer = _segment_flags_cpu(perm, pkeys, order_cols)
    pos = torch.arange(n, dtype=torch.int64)
    zero = torch.zeros_like(pos)
    seg_start = torch.cummax(torch.where(head, pos, zero), 0).values
    if kind == 0:
        return pos - seg_start + 1
    if kind == 1:
        peer_start = torch.cummax(torch.where(peer, pos, zero), 0).values
        return peer_start - seg_start + 1
    c = torch.cumsum(peer.to(torch.int64), 0)
    return c - c.index_select(0, seg_start) + 1


def segmented_rank(
    perm: torch.Tensor,
    pkeys: torch.Tensor,
    order_cols: Sequence[Any],
    kind: str,
) -> torch.Tensor:
    """``row_number`` / ``rank`` / ``dense_rank`` of every row within its
    partition, as int64 in ORIGINAL row order.

    ``perm`` is a stable sort permutation by (partition key, order keys);
    ``pkeys`` (int64) and ``order_cols`` are in original row order.  Each
    order column is a ``DeviceColumn`` or a ``(data, valid)`` pair; rows
    are peers when they share the partition and every order column is
    equal (null equals null, NaN equals NaN).  ``row_number`` ignores the
    order columns: ties keep the permutation's order."""
    if kind not in RANK_KINDS:
        raise ValueError(f"unknown rank kind {kind!r}")
    k = RANK_KINDS[kind]
    cols = [] if k == 0 else [_order_col_parts(c) for c in order_cols]
    if len(cols) > 4:
        raise NotImplementedError("at most 4 order columns on device")
    perm = perm.contiguous()
    pkeys = pkeys.contiguous()
    n = perm.numel()
    if _is_cpu(perm):
        out = torch.empty(n, dtype=torch.int64)
        if n > 0:
            out[perm] = _segmented_rank_cpu(perm, pkeys, cols, k)
        return out
    return get_ext().seg_rank(
        perm, pkeys, [c[0] for c in cols], [c[1] for c in cols], k
    )


SCAN_FUNCS = {"sum": 0, "min": 1, "max": 2}


def _value_col_parts(c: Any) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(8-byte data, validity) of a window value column; a NaN counts as
    null, as it does for the host executor."""
    data, valid = _order_col_parts(c)
    if data.is_floating_point():
        notnan = ~torch.isnan(data)
        valid = notnan if valid is None else (valid & notnan)
    return data, valid


def _segmented_shift_cpu(
    perm: torch.Tensor,
    pkeys: torch.Tensor,
    data: torch.Tensor,
    valid: Optional[torch.Tensor],
    offset: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Shifted (data, valid) per SORTED position."""
    n = perm.numel()
    pos = torch.arange(n, dtype=torch.int64)
    src = pos - max(-n, min(n, offset))
    inside = (src >= 0) & (src < n)
    srcc = torch.where(inside, src, pos)
    ks = pkeys.index_select(0, perm)
    inside &= ks.index_select(0, srcc) == ks
    rows = perm.index_select(0, srcc)
    ok = inside
    if valid is not None:
        ok = inside & valid.index_select(0, rows)
    v = data.index_select(0, rows)
    return torch.where(inside, v, torch.zeros_like(v)), ok


def segmented_shift(
    perm: torch.Tensor, pkeys: torch.Tensor, col: Any, offset: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``LAG`` (``offset > 0``) / ``LEAD`` (``offset < 0``) of one value
    column inside its partition: ``(data, valid)`` in ORIGINAL row order,
    where row ``perm[i]`` holds the value of row ``perm[i - offset]`` and
    is valid iff that position exists, lies in the same partition and
    holds a non-null value.  Inputs as :func:`segmented_rank`; ``col`` is
    a ``DeviceColumn`` or a ``(data, valid)`` pair.  ``data`` comes back
    widened to int64/float64 and is 0 where the partition has no source
    row."""
    data, valid = _value_col_parts(col)
    perm = perm.contiguous()
    pkeys = pkeys.contiguous()
    offset = int(offset)
    if _is_cpu(perm):
        n = perm.numel()
        out = torch.empty_like(data)
        out_valid = torch.empty(n, dtype=torch.bool)
        if n > 0:
            d, v = _segmented_shift_cpu(perm, pkeys, data, valid, offset)
            out[perm] = d
            out_valid[perm] = v
        return out, out_valid
    n = perm.numel()
    offset = max(-n, min(n, offset))  # beyond ±n nothing has a source
    out, out_valid = get_ext().seg_shift(perm, pkeys, data, valid, offset)
    return out, out_valid


def _segmented_scan_cpu(
    perm: torch.Tensor,
    pkeys: torch.Tensor,
    data: torch.Tensor,
    valid: Optional[torch.Tensor],
    op: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(acc, cnt) per SORTED position: a segmented Hillis-Steele scan, so
    a float sum only ever adds values of its own partition."""
    n = perm.numel()
    head, _ = _segment_flags_cpu(perm, pkeys, [])
    acc = data.index_select(0, perm)
    if valid is not None:
        ok = valid.index_select(0, perm)
        acc = torch.where(ok, acc, torch.zeros_like(acc))
        cnt = ok.to(torch.int64)
    else:
        cnt = torch.ones(n, dtype=torch.int64)
    pos = torch.arange(n, dtype=torch.int64)
    seg_start = torch.cummax(torch.where(head, pos, torch.zeros_like(pos)), 0).values
    longest = int((pos - seg_start).max().item()) + 1
    flag = head.clone()
    off = 1
    while off < longest:
        la, lc, lf = acc[:-off], cnt[:-off], flag[:-off]
        ra, rc, rf = acc[off:], cnt[off:], flag[off:]
        if op == 0:
            both = la + ra  # int64 wraps like the unsigned device add
        elif op == 1:
            both = torch.where(ra < la, ra, la)
        elif op == 2:
            both = torch.where(ra > la, ra, la)
        else:  # first / last non-null value (segmented_total only)
            both = la if op == 3 else ra
        merged = torch.where(lc == 0, ra, torch.where(rc == 0, la, both))
        new_acc = torch.where(rf, ra, merged)
        new_cnt = torch.where(rf, rc, lc + rc)
        new_flag = rf | lf
        acc = torch.cat([acc[:off], new_acc])
        cnt = torch.cat([cnt[:off], new_cnt])
        flag = torch.cat([flag[:off], new_flag])
        off <<= 1
    return acc, cnt


def segmented_scan(
    perm: torch.Tensor, pkeys: torch.Tensor, col: Any, func: str
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Running ``sum`` / ``min`` / ``max`` of one value column from the
    first sorted position of the row's partition to the row itself (ROWS
    UNBOUNDED PRECEDING .. CURRENT ROW; peers are not merged).  Returns
    ``(acc, cnt)`` in ORIGINAL row order: ``cnt`` (int64) is the number of
    non-null values folded so far and ``acc`` (int64 or float64) their
    aggregate, 0 while ``cnt`` is 0.  A null row carries the running value
    through; the caller decides the validity of its result.  Integer sums
    wrap.  Inputs as :func:`segmented_shift`."""
    if func not in SCAN_FUNCS:
        raise ValueError(f"unknown scan function {func!r}")
    op = SCAN_FUNCS[func]
    data, valid = _value_col_parts(col)
    perm = perm.contiguous()
    pkeys = pkeys.contiguous()
    if _is_cpu(perm):
        n = perm.numel()
        acc = torch.empty_like(data)
        cnt = torch.empty(n, dtype=torch.int64)
        if n > 0:
            a, c = _segmented_scan_cpu(perm, pkeys, data, valid, op)
            acc[perm] = a
            cnt[perm] = c
        return acc, cnt
    acc, cnt = get_ext().seg_scan(perm, pkeys, data, valid, op)
    return acc, cnt


TOTAL_FUNCS = {"sum": 0, "min": 1, "max": 2, "first": 3, "last": 4}


def _segmented_total_cpu(
    perm: torch.Tensor,
    pkeys: torch.Tensor,
    data: torch.Tensor,
    valid: Optional[torch.Tensor],
    op: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(acc, cnt) per SORTED position: the running scan's value at the
    last position of the partition, copied to all of its positions."""
    n = perm.numel()
    acc, cnt = _segmented_scan_cpu(perm, pkeys, data, valid, op)
    head, _ = _segment_flags_cpu(perm, pkeys, [])
    tail = torch.ones(n, dtype=torch.bool)
    tail[:-1] = head[1:]
    seg = torch.cumsum(head.to(torch.int64), 0) - 1
    last = torch.nonzero(tail).reshape(-1).index_select(0, seg)
    return acc.index_select(0, last), cnt.index_select(0, last)


def segmented_total(
    perm: torch.Tensor, pkeys: torch.Tensor, col: Any, func: str
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Whole-partition ``sum`` / ``min`` / ``max`` / ``first`` / ``last``
    of one value column, given to every row of the partition.  Returns
    ``(acc, cnt)`` in ORIGINAL row order: ``cnt`` (int64) is the number of
    non-null values of the row's partition and ``acc`` (int64 or float64)
    their aggregate, 0 when ``cnt`` is 0.  ``first`` / ``last`` are the
    first / last non-null value in sorted order.  All rows of a partition
    hold the same bits, and for ``sum`` / ``min`` / ``max`` those are the
    bits :func:`segmented_scan` yields at the partition's last sorted
    position.  Integer sums wrap.  Inputs as :func:`segmented_scan`."""
    if func not in TOTAL_FUNCS:
        raise ValueError(f"unknown total function {func!r}")
    op = TOTAL_FUNCS[func]
    data, valid = _value_col_parts(col)
    perm = perm.contiguous()
    pkeys = pkeys.contiguous()
    if _is_cpu(perm):
        n = perm.numel()
        acc = torch.empty_like(data)
        cnt = torch.empty(n, dtype=torch.int64)
        if n > 0:
            a, c = _segmented_total_cpu(perm, pkeys, data, valid, op)
            acc[perm] = a
            cnt[perm] = c
        return acc, cnt
    acc, cnt = get_ext().seg_total(perm, pkeys, data, valid, op)
    return acc, cnt


# Largest frame reach seg_frame takes: a copy of SEG_FRAME_MAX_REACH in
# csrc/relational.h for hosts without the extension (a GPU test compares
# the two).
SEG_FRAME_MAX_REACH = 1024


def _segmented_frame_cpu(
    perm: torch.Tensor,
    pkeys: torch.Tensor,
    data: torch.Tensor,
    valid: Optional[torch.Tensor],
    op: int,
    lo: int,
    hi: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(acc, cnt) per SORTED position: one pass per offset from ``lo`` to
    ``hi``, each folding the value ``d`` positions away where that row is
    in the same partition and non-null.  A sum therefore adds its frame
    left to right, starting from 0."""
    n = perm.numel()
    ks = pkeys.index_select(0, perm)
    xs = data.index_select(0, perm)
    if valid is not None:
        ok = valid.index_select(0, perm)
    else:
        ok = torch.ones(n, dtype=torch.bool)
    acc = torch.zeros_like(xs)
    cnt = torch.zeros(n, dtype=torch.int64)
    for d in range(lo, hi + 1):
        if abs(d) >= n:
            continue
        dst = slice(0, n - d) if d >= 0 else slice(-d, n)
        src = slice(d, n) if d >= 0 else slice(0, n + d)
        take = (ks[src] == ks[dst]) & ok[src]
        x, a, c = xs[src], acc[dst], cnt[dst]
        if op == 0:
            new = a + x  # int64 wraps like the unsigned device add
        elif op == 1:
            new = torch.where((c == 0) | (x < a), x, a)
        elif op == 2:
            new = torch.where((c == 0) | (x > a), x, a)
        elif op == 3:
            new = torch.where(c == 0, x, a)
        else:
            new = x
        acc[dst] = torch.where(take, new, a)
        cnt[dst] = c + take.to(torch.int64)
    return acc, cnt


def segmented_frame(
    perm: torch.Tensor,
    pkeys: torch.Tensor,
    col: Any,
    func: str,
    lo: int,
    hi: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``sum`` / ``min`` / ``max`` / ``first`` / ``last`` of one value
    column over the moving frame ROWS BETWEEN ``lo`` AND ``hi``: signed
    offsets in sorted positions from the row itself (``-2`` is 2
    PRECEDING), clipped to the row's partition; ``lo > hi`` is legal and
    leaves every frame empty.  Returns ``(acc, cnt)`` in ORIGINAL row
    order: ``cnt`` (int64) is the number of non-null values in the row's
    frame and ``acc`` (int64 or float64) their aggregate, 0 when ``cnt``
    is 0.  A sum starts from 0 and adds the frame's values in sorted
    order, fresh for every row, so the CPU and the device form agree bit
    for bit; integer sums wrap.  ``first`` / ``last`` are the first /
    last non-null value of the frame.  Inputs as :func:`segmented_scan`.
    Offsets are clamped to ``[-n, n]``.  A frame whose reach ``max(0,
    -lo) + max(0, hi)`` then exceeds ``SEG_FRAME_MAX_REACH`` raises
    ``NotImplementedError`` (unless it is empty for every row)."""
    if func not in TOTAL_FUNCS:
        raise ValueError(f"unknown frame function {func!r}")
    op = TOTAL_FUNCS[func]
    data, valid = _value_col_parts(col)
    perm = perm.contiguous()
    pkeys = pkeys.contiguous()
    n = perm.numel()
    lo = max(-n, min(n, int(lo)))  # beyond ±n nothing is in the frame
    hi = max(-n, min(n, int(hi)))
    if n == 0 or lo > hi or lo >= n or hi <= -n:
        # no row has anything in its frame
        return torch.zeros_like(data), torch.zeros_like(perm)
    if max(0, -lo) + max(0, hi) > SEG_FRAME_MAX_REACH:
        raise NotImplementedError("window frame reach beyond the kernel's")
    if _is_cpu(perm):
        acc = torch.empty_like(data)
        cnt = torch.empty(n, dtype=torch.int64)
        a, c = _segmented_frame_cpu(perm, pkeys, data, valid, op, lo, hi)
        acc[perm] = a
        cnt[perm] = c
        return acc, cnt
    acc, cnt = get_ext().seg_frame(perm, pkeys, data, valid, op, lo, hi)
    return acc, cnt


def take_per_group_indices(
    perm: torch.Tensor, pkeys: torch.Tensor, n: int
) -> torch.Tensor:
    """Row indices of the first ``n`` sorted positions of every partition,
    in sorted order (deterministic).  Inputs as :func:`segmented_rank`."""
    perm = perm.contiguous()
    pkeys = pkeys.contiguous()
    if perm.numel() == 0 or n <= 0:
        return perm[:0]
    if _is_cpu(perm):
        rn = _segmented_rank_cpu(perm, pkeys, [], 0)
        return perm[rn <= n]
    out, bases = get_ext().seg_take(perm, pkeys, int(n))
    total = int(bases[-1].item())  # the one host read of this op
    return out.narrow(0, 0, total)
