"""Interleaved A/B of the fused join + filter + projection and of the join
build-table memo on the flagship pipeline (same box/process), over the two
knobs FUGUE_JOIN_FUSED and FUGUE_JOIN_BUILD_MEMO (four sides).

The flagship step is host-timed interleaved (medians of ``--rounds`` rounds
of 8 steps per side).  The tail alone — everything after the group-by: the
join of the 1M-row aggregate with ``dims``, ``WHERE s > w`` and the
projection, on one fixed aggregate frame — is timed per side with device
events and with the host clock (medians of 9; it ends in a readback, so
both clocks see the whole tail).

Every GPU section runs under its own time limit (``--limit`` seconds), kept
by a watchdog thread that ends the process with status 124; any error ends
the process too, so nothing is started on the GPU after a failure.  Run it
under an outer limit as well:

    timeout -k 10 600 python benchmarks/join_select_ab.py [--rounds 5]"""
import argparse
import os
import sys
import threading
import time
from contextlib import contextmanager

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

_FUSED = "FUGUE_JOIN_FUSED"
_MEMO = "FUGUE_JOIN_BUILD_MEMO"
SIDES = (("0", "0"), ("0", "1"), ("1", "0"), ("1", "1"))  # (fused, memo)


def _median(xs):
    return sorted(xs)[len(xs) // 2]


@contextmanager
def _limit(seconds, what):
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


def _host_ms(fn, n=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1000


def _event_ms(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--rows", type=int, default=125_000_000)
    args = ap.parse_args()

    import pyarrow as pa

    import fugue_amd.api as fa
    from fugue_amd.collections.partition import PartitionSpec
    from fugue_amd.column import functions as f
    from fugue_amd.column.expressions import col
    from fugue_amd.column.sql import SelectColumns
    from fugue_amd.hip.execution_engine import HipExecutionEngine
    from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
    from fugue_amd.schema import Schema

    engine = HipExecutionEngine()
    device = torch.device(engine.device)
    gen = torch.Generator(device=device)
    gen.manual_seed(42)
    n = args.rows
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

    def knobs(side):
        os.environ[_FUSED], os.environ[_MEMO] = side

    with _limit(args.limit, "first sight, recording, first replay"):
        for _ in range(4):
            _host_ms(step)
    agg = engine.aggregate(
        fact, PartitionSpec(by=["k"]),
        [f.sum(col("v")).alias("s"), f.count(col("v")).alias("n")])
    sc = SelectColumns(col("k"), col("s"), col("n"), col("w"))
    where = col("s") > col("w")

    def tail():
        try:
            return engine.join_select(agg, dims, "inner", None, sc, where)
        except NotImplementedError:  # FUGUE_JOIN_FUSED=0
            return engine.select(engine.join(agg, dims, how="inner"), sc,
                                 where=where)

    for side in SIDES:
        knobs(side)
        with _limit(args.limit, f"tail, fused={side[0]} memo={side[1]}"):
            rows = tail().count()
            tail()
            ev = [_event_ms(tail) for _ in range(9)]
            ho = [_host_ms(tail) for _ in range(9)]
        print(f"tail fused={side[0]} memo={side[1]}: device events "
              f"{_median(ev):.3f} ms, host {_median(ho):.3f} ms "
              f"(min {min(ho):.3f} max {max(ho):.3f}), {rows} rows",
              flush=True)

    res = {side: [] for side in SIDES}
    for _ in range(args.rounds):
        for side in SIDES:
            knobs(side)
            with _limit(args.limit, f"flagship steps, {side}"):
                _host_ms(step)
                res[side].append(_host_ms(step, 8))
    os.environ.pop(_FUSED, None)
    os.environ.pop(_MEMO, None)
    for side in SIDES:
        print(f"flagship fused={side[0]} memo={side[1]}: median "
              f"{_median(res[side]):.3f} ms "
              f"all={[round(x, 3) for x in res[side]]}", flush=True)
    print("engine counters:", {k: v for k, v in engine.stats.snapshot().items()
                               if k.startswith("join")}, flush=True)


if __name__ == "__main__":
    main()
