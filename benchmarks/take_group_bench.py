"""Top-3 rows per group: device partitioned take vs the host (pandas) path.

``fa.take(df, 3, presort="v desc", partition=by k)`` on one GPU at a few
row counts and group cardinalities.  The device path is the segmented
rank kernels; the host path is what the engine did before them (D2H,
pandas sort + ``groupby().head()``, H2D), forced here through
``FUGUE_HIP_FORCE_HOST_TAKE=1``.  The two paths alternate step by step,
every step ends in a device synchronise, and both results are compared
once per shape.  Prints one JSON line per shape.

    python benchmarks/take_group_bench.py [--rows 1000000,4000000]
        [--groups 1000,1000000] [--steps 5] [--host-steps 3] [--warmup 2]
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

import fugue_amd.api as fa  # noqa: E402
from fugue_amd.hip.execution_engine import HipExecutionEngine  # noqa: E402
from fugue_amd.hip.frame import HipDataFrame  # noqa: E402

_FORCE_HOST = "FUGUE_HIP_FORCE_HOST_TAKE"


def _step(engine, hdf, host: bool):
    if host:
        os.environ[_FORCE_HOST] = "1"
    else:
        os.environ.pop(_FORCE_HOST, None)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fa.take(
            hdf, 3, presort="v desc", partition=dict(by=["k"]),
            engine=engine, as_fugue=True,
        )
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res
    finally:
        os.environ.pop(_FORCE_HOST, None)


def _digest(res) -> tuple:
    pdf = res.as_pandas()
    return (len(pdf), int(pdf["k"].sum()), float(pdf["v"].sum()))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,4000000,16000000")
    ap.add_argument("--groups", default="1000,1000000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("take_group_bench needs a GPU")
    engine = HipExecutionEngine()
    for n in [int(x) for x in args.rows.split(",")]:
        for g in [int(x) for x in args.groups.split(",")]:
            rng = np.random.default_rng(n % 1000 + g)
            pdf = pd.DataFrame(
                dict(
                    k=rng.integers(0, g, n),
                    v=rng.permutation(n).astype(np.float64),
                    w=rng.integers(0, 1 << 40, n),
                )
            )
            hdf = engine.to_df(pdf)
            assert isinstance(hdf, HipDataFrame)
            del pdf
            before = engine.stats.get("take.device_partitioned")
            for _ in range(args.warmup):
                _, dres = _step(engine, hdf, host=False)
            _, hres = _step(engine, hdf, host=True)
            assert engine.stats.get("take.device_partitioned") == before + args.warmup
            same = _digest(dres) == _digest(hres)
            dev_ms, host_ms = [], []
            for i in range(max(args.steps, args.host_steps)):
                if i < args.steps:
                    dev_ms.append(_step(engine, hdf, host=False)[0])
                if i < args.host_steps:
                    host_ms.append(_step(engine, hdf, host=True)[0])
            d, h = float(np.median(dev_ms)), float(np.median(host_ms))
            print(
                json.dumps(
                    dict(
                        bench="take_group_top3",
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
                        steps=args.steps,
                        host_steps=args.host_steps,
                        warmup=args.warmup,
                    )
                ),
                flush=True,
            )


if __name__ == "__main__":
    main()
