"""LAG + running SUM per group: device value windows vs the host path.

``SELECT k, v, LAG(v) OVER w AS p, SUM(v) OVER w AS s`` with ``w =
(PARTITION BY k ORDER BY v)`` through FugueSQL on one GPU, at the shapes
of ``take_group_bench.py``.  The device path is ``engine.window_over``
(one partition sort, then the ``seg_shift`` / ``seg_scan_*`` kernels);
the host path is what the engine did before it (gather to pandas, the
SQL executor, H2D), forced here through ``FUGUE_HIP_FORCE_HOST_WINDOW=1``.
The two paths alternate step by step, every step ends in a device
synchronise, and both results are compared once per shape.  ``sort_ms``
is the partition sort alone, timed the same way.  Prints one JSON line
per shape.

    python benchmarks/window_bench.py [--rows 1000000,4000000]
        [--groups 1000,1000000] [--steps 5] [--host-steps 3] [--warmup 2]

``--partition`` runs the whole-partition case instead: percent-of-total
plus ``FIRST_VALUE`` (``engine.partition_over``, the ``seg_total_*``
kernels) against the same forced host path, and times the
``segmented_total`` launch chain alone with device events next to a plain
copy of the bytes it moves at the least (120 B/row: 24 for the forward
summary, 40 for the forward apply, 8 for the backward summary, 48 for the
backward apply).

``--frame`` runs the framed case: a 7-row moving ``AVG`` (6 PRECEDING ..
CURRENT ROW) plus a centred 7-row ``SUM`` (3 PRECEDING .. 3 FOLLOWING),
``engine.frame_over`` on the ``seg_frame`` kernel against the same forced
host path, and times each ``segmented_frame`` launch alone with device
events.

``--kernels N`` instead runs only the kernels (and a plain copy of the
bytes they move at the least: 33 B/row for the shift, 24 + 40 B/row for
the scan's summary and apply) N times on the first shape, for a
``rocprofv3 --kernel-trace --stats`` run of its own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fugue_amd.hip import ops as dops  # noqa: E402
from fugue_amd.hip.execution_engine import HipExecutionEngine  # noqa: E402
from fugue_amd.hip.frame import HipDataFrame  # noqa: E402
from fugue_amd.sql.api import fugue_sql  # noqa: E402

_FORCE_HOST = "FUGUE_HIP_FORCE_HOST_WINDOW"
_SQL = (
    "SELECT k, v, LAG(v) OVER (PARTITION BY k ORDER BY v) AS p, "
    "SUM(v) OVER (PARTITION BY k ORDER BY v) AS s FROM df"
)


_PARTITION_SQL = (
    "SELECT k, v, v / t AS share, f FROM (SELECT k, v, "
    "SUM(v) OVER (PARTITION BY k) AS t, "
    "FIRST_VALUE(v) OVER (PARTITION BY k) AS f FROM df)"
)
_TOTAL_BYTES_PER_ROW = 120

_FRAME_SQL = (
    "SELECT k, v, AVG(v) OVER (PARTITION BY k ORDER BY v "
    "ROWS BETWEEN 6 PRECEDING AND CURRENT ROW) AS m, "
    "SUM(v) OVER (PARTITION BY k ORDER BY v "
    "ROWS BETWEEN 3 PRECEDING AND 3 FOLLOWING) AS c FROM df"
)


def _step(engine, hdf, host: bool, sql: str = _SQL):
    if host:
        os.environ[_FORCE_HOST] = "1"
    else:
        os.environ.pop(_FORCE_HOST, None)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fugue_sql(sql, df=hdf, engine=engine, as_fugue=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res
    finally:
        os.environ.pop(_FORCE_HOST, None)


def _sort_step(engine, hdf):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pkeys, perm = engine._partition_sort(hdf, ["k"], ["v"], [True], "last")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, pkeys, perm


def _digest(res) -> tuple:
    pdf = res.as_pandas()
    return (
        len(pdf), int(pdf["k"].sum()), float(pdf["p"].sum()),
        int(pdf["p"].isna().sum()), float(pdf["s"].sum()),
    )


def _frame(engine, n: int, g: int) -> HipDataFrame:
    rng = np.random.default_rng(n % 1000 + g)
    pdf = pd.DataFrame(
        dict(
            k=rng.integers(0, g, n),
            # integer-valued and unique: exact sums, no ties
            v=rng.permutation(n).astype(np.float64),
            w=rng.integers(0, 1 << 40, n),
        )
    )
    hdf = engine.to_df(pdf)
    assert isinstance(hdf, HipDataFrame)
    return hdf


def _kernels_only(engine, hdf, reps: int) -> None:
    _, pkeys, perm = _sort_step(engine, hdf)
    c = hdf.col("v")
    n = perm.numel()
    src = {b: torch.empty(n * b // 16, dtype=torch.int64, device=perm.device)
           for b in (33, 24, 40)}
    for _ in range(reps):
        dops.segmented_shift(perm, pkeys, c, 1)
        dops.segmented_scan(perm, pkeys, c, "sum")
        for t in src.values():  # a copy reads and writes half the bytes each
            t.clone()
    torch.cuda.synchronize()
    print(json.dumps(dict(bench="window_kernels", rows=n, reps=reps,
                          copy_elems={str(b): int(t.numel()) for b, t in src.items()})))


def _event_ms(fn, reps: int) -> float:
    """Median device time of one call of ``fn`` (device events)."""
    out = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def _partition_digest(res) -> tuple:
    pdf = res.as_pandas()
    return (
        len(pdf), int(pdf["k"].sum()), float(pdf["share"].sum()),
        int(pdf["share"].isna().sum()), float(pdf["f"].sum()),
    )


def _partition_case(engine, args, n: int, g: int) -> None:
    hdf = _frame(engine, n, g)
    before = engine.stats.get("window.device_partition")
    for _ in range(args.warmup):
        _, dres = _step(engine, hdf, False, _PARTITION_SQL)
    _, hres = _step(engine, hdf, True, _PARTITION_SQL)
    assert engine.stats.get("window.device_partition") == before + 2 * args.warmup
    same = _partition_digest(dres) == _partition_digest(hres)
    dev_ms, host_ms = [], []
    for i in range(max(args.steps, args.host_steps)):
        if i < args.steps:
            dev_ms.append(_step(engine, hdf, False, _PARTITION_SQL)[0])
        if i < args.host_steps:
            host_ms.append(_step(engine, hdf, True, _PARTITION_SQL)[0])
    pkeys, perm = engine._partition_sort(hdf, ["k"], [], [], "last")
    c = hdf.col("v")
    src = torch.empty(
        n * _TOTAL_BYTES_PER_ROW // 16, dtype=torch.int64, device=perm.device
    )
    for _ in range(3):
        dops.segmented_total(perm, pkeys, c, "sum")
        src.clone()
    total_ms = _event_ms(lambda: dops.segmented_total(perm, pkeys, c, "sum"), 20)
    copy_ms = _event_ms(lambda: src.clone(), 20)
    d, h = float(np.median(dev_ms)), float(np.median(host_ms))
    nbytes = n * _TOTAL_BYTES_PER_ROW
    print(
        json.dumps(
            dict(
                bench="window_partition_share_first",
                rows=n,
                groups=g,
                device_ms=round(d, 3),
                device_ms_min=round(min(dev_ms), 3),
                device_ms_max=round(max(dev_ms), 3),
                host_ms=round(h, 3),
                host_ms_min=round(min(host_ms), 3),
                host_ms_max=round(max(host_ms), 3),
                host_over_device=round(h / d, 2),
                results_equal=bool(same),
                seg_total_ms=round(total_ms, 4),
                seg_total_gbps=round(nbytes / total_ms / 1e6, 1),
                copy_ms=round(copy_ms, 4),
                copy_gbps=round(nbytes / copy_ms / 1e6, 1),
                steps=args.steps,
                host_steps=args.host_steps,
                warmup=args.warmup,
            )
        ),
        flush=True,
    )


def _frame_digest(res) -> tuple:
    pdf = res.as_pandas()
    return (
        len(pdf), int(pdf["k"].sum()), float(pdf["m"].sum()),
        int(pdf["m"].isna().sum()), float(pdf["c"].sum()),
    )


def _frame_case(engine, args, n: int, g: int) -> None:
    hdf = _frame(engine, n, g)
    before = engine.stats.get("window.device_frame")
    for _ in range(args.warmup):
        _, dres = _step(engine, hdf, False, _FRAME_SQL)
    _, hres = _step(engine, hdf, True, _FRAME_SQL)
    assert engine.stats.get("window.device_frame") == before + 2 * args.warmup
    same = _frame_digest(dres) == _frame_digest(hres)
    dev_ms, host_ms = [], []
    for i in range(max(args.steps, args.host_steps)):
        if i < args.steps:
            dev_ms.append(_step(engine, hdf, False, _FRAME_SQL)[0])
        if i < args.host_steps:
            host_ms.append(_step(engine, hdf, True, _FRAME_SQL)[0])
    pkeys, perm = engine._partition_sort(hdf, ["k"], ["v"], [True], "last")
    c = hdf.col("v")
    for _ in range(3):
        dops.segmented_frame(perm, pkeys, c, "sum", -6, 0)
    avg_ms = _event_ms(
        lambda: dops.segmented_frame(perm, pkeys, c, "sum", -6, 0), 20
    )
    ctr_ms = _event_ms(
        lambda: dops.segmented_frame(perm, pkeys, c, "sum", -3, 3), 20
    )
    d, h = float(np.median(dev_ms)), float(np.median(host_ms))
    print(
        json.dumps(
            dict(
                bench="window_frame_avg7_sum7",
                rows=n,
                groups=g,
                device_ms=round(d, 3),
                device_ms_min=round(min(dev_ms), 3),
                device_ms_max=round(max(dev_ms), 3),
                device_rows_per_s=round(n / d * 1e3),
                host_ms=round(h, 3),
                host_ms_min=round(min(host_ms), 3),
                host_ms_max=round(max(host_ms), 3),
                host_rows_per_s=round(n / h * 1e3),
                host_over_device=round(h / d, 2),
                results_equal=bool(same),
                seg_frame_trailing7_ms=round(avg_ms, 4),
                seg_frame_centred7_ms=round(ctr_ms, 4),
                steps=args.steps,
                host_steps=args.host_steps,
                warmup=args.warmup,
            )
        ),
        flush=True,
    )


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,4000000,16000000")
    ap.add_argument("--groups", default="1000,1000000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--partition", action="store_true")
    ap.add_argument("--frame", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_bench needs a GPU")
    engine = HipExecutionEngine()
    rows = [int(x) for x in args.rows.split(",")]
    groups = [int(x) for x in args.groups.split(",")]
    if args.kernels > 0:
        _kernels_only(engine, _frame(engine, rows[0], groups[0]), args.kernels)
        return
    if args.frame:
        for n in rows:
            for g in groups:
                _frame_case(engine, args, n, g)
        return
    if args.partition:
        for n in rows:
            for g in groups:
                _partition_case(engine, args, n, g)
        return
    for n in rows:
        for g in groups:
            hdf = _frame(engine, n, g)
            before = engine.stats.get("window.device_value")
            for _ in range(args.warmup):
                _, dres = _step(engine, hdf, host=False)
            _, hres = _step(engine, hdf, host=True)
            assert engine.stats.get("window.device_value") == before + 2 * args.warmup
            same = _digest(dres) == _digest(hres)
            dev_ms, host_ms, sort_ms = [], [], []
            for i in range(max(args.steps, args.host_steps)):
                if i < args.steps:
                    dev_ms.append(_step(engine, hdf, host=False)[0])
                    sort_ms.append(_sort_step(engine, hdf)[0])
                if i < args.host_steps:
                    host_ms.append(_step(engine, hdf, host=True)[0])
            d, h = float(np.median(dev_ms)), float(np.median(host_ms))
            s = float(np.median(sort_ms))
            print(
                json.dumps(
                    dict(
                        bench="window_lag_sum",
                        rows=n,
                        groups=g,
                        device_ms=round(d, 3),
                        device_ms_min=round(min(dev_ms), 3),
                        device_ms_max=round(max(dev_ms), 3),
                        sort_ms=round(s, 3),
                        sort_share=round(s / d, 2),
                        host_ms=round(h, 3),
                        host_ms_min=round(min(host_ms), 3),
                        host_ms_max=round(max(host_ms), 3),
                        host_over_device=round(h / d, 2),
                        results_equal=bool(same),
                        steps=args.steps,
                        host_steps=args.host_steps,
                        warmup=args.warmup,
                    )
                ),
                flush=True,
            )


if __name__ == "__main__":
    main()
