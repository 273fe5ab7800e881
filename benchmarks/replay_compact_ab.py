"""Interleaved A/B of the compact binned dense replay on the flagship
pipeline (same box/process): FUGUE_GB_REPLAY_COMPACT 0 (the 10 B/row
binned layout) against 1 (4 B/row, no per-row destination, 16-bit ids) and
2 (8 B/row: no per-row destination, int32 ids and the binned aggregate).

For every side the recording call (the one-time preparation) is host-timed
twice (the first sample of the first side carries first-use code loads),
the flagship step is host-timed interleaved (medians of 5 rounds of 8
steps), and the scatter and the aggregate are event-timed on the side's own
cached layout (medians of 5); the compact scatter at 512 and 1024 threads
per block.  ``--copy`` adds a plain 1 GB device copy as the same-session
bandwidth yardstick.

Every GPU section runs under its own time limit (``--limit`` seconds),
kept by a watchdog thread that ends the process with status 124 even while
the main thread is blocked in a device synchronisation; any error ends the
process too, so nothing is started on the GPU after a failure.  Run it
under an outer limit as well:

    timeout -k 10 600 python benchmarks/replay_compact_ab.py [--copy]
        [--rounds 5] [--limit 120]"""
import argparse
import os
import sys
import threading
import time
from contextlib import contextmanager

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

_KNOB = "FUGUE_GB_REPLAY_COMPACT"


def _median(xs):
    return sorted(xs)[len(xs) // 2]


@contextmanager
def _limit(seconds, what):
    """ends the process when the section takes longer than ``seconds``.
    The timer runs on its own thread: a signal handler would not run while
    the main thread sits in a blocking synchronize call."""

    def _over():
        print(f"TIME LIMIT: {what} exceeded {seconds} s", flush=True)
        os._exit(124)

    timer = threading.Timer(seconds, _over)
    timer.daemon = True
    timer.start()
    try:
        yield
    finally:
        timer.cancel()


def _event_ms(fn, reps=5):
    """median device time of fn() over reps, after one warm-up call"""
    fn()
    out = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return _median(out)


def _host_ms(fn, n=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--copy", action="store_true")
    args = ap.parse_args()

    import pyarrow as pa

    import fugue_amd.api as fa
    from fugue_amd.hip import ops as dops
    from fugue_amd.hip.execution_engine import HipExecutionEngine
    from fugue_amd.hip.ext import get_ext
    from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
    from fugue_amd.schema import Schema

    ext = get_ext()
    engine = HipExecutionEngine()
    device = torch.device(engine.device)
    gen = torch.Generator(device=device)
    gen.manual_seed(42)
    n = 125_000_000
    with _limit(args.limit, "input generation"):
        fact = HipDataFrame.from_columns(
            {"k": DeviceColumn(torch.randint(0, 1_000_000, (n,),
                                             dtype=torch.int64, device=device,
                                             generator=gen), None, pa.int64()),
             "v": DeviceColumn(torch.rand(n, dtype=torch.float64,
                                          device=device, generator=gen),
                               None, pa.float64())},
            Schema("k:long,v:double"), engine.device)
        dims = HipDataFrame.from_columns(
            {"k": DeviceColumn(torch.arange(0, 1_000_000, dtype=torch.int64,
                                            device=device), None, pa.int64()),
             "w": DeviceColumn(torch.rand(1_000_000, dtype=torch.float64,
                                          device=device, generator=gen),
                               None, pa.float64())},
            Schema("k:long,w:double"), engine.device)
        torch.cuda.synchronize()

    def scale(df: HipDataFrame) -> HipDataFrame:
        v = df.col("v")
        return HipDataFrame.from_columns(
            {"k": df.col("k"),
             "v": DeviceColumn(v.data * 1.000001, v.valid, pa.float64())},
            Schema("k:long,v:double"), df.device)

    SQL = ("t = TRANSFORM fact USING scale SCHEMA k:long,v:double\n"
           "agg = SELECT k, SUM(v) AS s, COUNT(v) AS n FROM t GROUP BY k\n"
           "res = SELECT agg.k, s, n, w FROM agg INNER JOIN dims "
           "ON agg.k = dims.k WHERE s > w\nYIELD DATAFRAME AS result\n")

    def step():
        fa.fugue_sql(SQL, fact=fact, dims=dims, scale=scale, engine=engine,
                     as_fugue=True)

    if args.copy:
        with _limit(args.limit, "copy yardstick"):
            src = torch.empty(1 << 27, dtype=torch.float64, device=device)
            dstb = torch.empty_like(src)
            ms = _event_ms(lambda: dstb.copy_(src))
            print(f"copy 1 GB: {ms:.3f} ms "
                  f"({2 * src.numel() * 8 / ms / 1e9:.2f} TB/s read+write)",
                  flush=True)
            del src, dstb

    vals = fact.col("v").data
    pvals = torch.empty_like(vals)
    with _limit(args.limit, "first sight"):
        _host_ms(step)  # first sight of the keys and first-use code loads
    entries = {}
    sides = ("0", "1", "2")
    dops._LAYOUT_MEMO_CAP = max(dops._LAYOUT_MEMO_CAP, len(sides))
    for side in sides:
        os.environ[_KNOB] = side
        records = []
        for _ in range(2):
            dops._LAYOUT_SEEN.clear()
            for k in [k for k, e in dops._LAYOUT_MEMO.items()
                      if e is entries.get(side)]:
                del dops._LAYOUT_MEMO[k]
            entries.pop(side, None)
            before = set(dops._LAYOUT_MEMO)
            with _limit(args.limit, f"recording, knob {side}"):
                first = _host_ms(step)  # first sight under this memo key
                records.append(_host_ms(step))  # the one-time preparation
                _host_ms(step)  # one replay
            new = [k for k in dops._LAYOUT_MEMO if k not in before]
            entries[side] = dops._LAYOUT_MEMO[new[0]]
        ent = entries[side]
        record = records[1]
        per_row = sum(
            t.numel() * t.element_size()
            for t in (ent.gid, ent.rank, ent.dst, ent.rel, ent.tile_start,
                      ent.tile_delta) if t is not None
        ) / n
        print(f"prep knob={side}: compact={ent.tile_start is not None} "
              f"bin_parts={ent.bin_parts} first-sight {first:.1f} ms, "
              f"recording {record:.1f} ms (first sample {records[0]:.1f}), "
              f"cached {per_row:.2f} B/row",
              flush=True)

    def rate(nbytes, ms):
        return f"{ms:.3f} ms ({n * nbytes / ms / 1e9:.2f} TB/s)"

    old, new = entries["0"], entries["1"]
    agg_args = lambda e: (  # noqa: E731
        pvals, e.bin_offsets, e.bin_group_base, e.bin_chunk_base,
        e.bin_chunks, e.n_groups, e.bin_chunk, e.bin_slots)
    with _limit(args.limit, "binned kernels"):
        sc = _event_ms(lambda: ext.scatter_tile(vals, old.rank, old.dst,
                                                old.tile))
        ag = _event_ms(lambda: ext.gb_dense_aggregate_binned(
            old.gid, *agg_args(old)))
        print(f"binned: scatter_tile {rate(22, sc)}, aggregate+zero "
              f"{rate(12, ag)}", flush=True)
    if new.rel is None:
        print("knob 1 did not build a compact layout", flush=True)
        sys.exit(1)
    for th in (512, 1024):
        with _limit(args.limit, f"compact scatter, {th} threads"):
            sc = _event_ms(lambda: ext.scatter_tile_compact(
                vals, new.rank, new.tile_start, new.tile_delta, new.tile, th,
                pvals))
            print(f"compact: scatter_tile_compact threads={th} "
                  f"{rate(18, sc)}", flush=True)
    with _limit(args.limit, "compact aggregate"):
        ag = _event_ms(lambda: ext.gb_dense_aggregate_compact(
            new.rel, *agg_args(new)))
        print(f"compact: aggregate+zero {rate(10, ag)}", flush=True)

    with _limit(args.limit, "binned aggregate on the knob-2 layout"):
        mid = entries["2"]
        ag = _event_ms(lambda: ext.gb_dense_aggregate_binned(
            mid.gid, *agg_args(mid)))
        print(f"knob 2: binned aggregate+zero {rate(12, ag)}", flush=True)

    res = {side: [] for side in sides}
    for _ in range(args.rounds):
        for side in sides:
            os.environ[_KNOB] = side
            with _limit(args.limit, f"flagship steps, knob {side}"):
                res[side].append(_host_ms(step, 8))
    os.environ.pop(_KNOB, None)
    for side in sides:
        print(f"flagship knob={side}: median {_median(res[side]):.3f} ms "
              f"all={[round(x, 3) for x in res[side]]}", flush=True)


if __name__ == "__main__":
    main()
