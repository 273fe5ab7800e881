"""Interleaved A/B of FUGUE_GB_REPLAY_DENSE on the flagship and q3
pipelines (same box/process), medians of 5 rounds.

Flagship variants: the plain replay (DENSE=0), the dense aggregate with
the by-position value scatter (DENSE=1, FUGUE_GB_REPLAY_TILE=0) and the
dense aggregate with the tile-coalesced scatter (DENSE=1, default tile),
so the two halves of the dense replay are measured separately.  q3 draws
fresh keys every step and never replays: it only checks the gate costs
nothing there."""
import importlib.util
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

FLAGSHIP_VARIANTS = [
    ("DENSE=0", {"FUGUE_GB_REPLAY_DENSE": "0"}),
    ("DENSE=1 TILE=0", {"FUGUE_GB_REPLAY_DENSE": "1",
                        "FUGUE_GB_REPLAY_TILE": "0"}),
    ("DENSE=1", {"FUGUE_GB_REPLAY_DENSE": "1"}),
]
Q3_VARIANTS = [FLAGSHIP_VARIANTS[0], FLAGSHIP_VARIANTS[2]]
_KNOBS = ("FUGUE_GB_REPLAY_DENSE", "FUGUE_GB_REPLAY_TILE")


def _select(env):
    for name in _KNOBS:
        os.environ.pop(name, None)
    os.environ.update(env)


def run_ab(step, label, variants, rounds=5, k=8):
    def timed(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1000

    for _, env in variants:
        _select(env)
        timed(3)  # first sight, recording call, one replay
    res = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, env in variants:
            _select(env)
            res[name].append(timed(k))
    _select({})
    for name, _ in variants:
        med = sorted(res[name])[len(res[name]) // 2]
        print(f"{label} {name}: median {med:.3f} ms "
              f"all={[round(x, 2) for x in res[name]]}", flush=True)


def main():
    import pyarrow as pa

    import fugue_amd.api as fa
    from fugue_amd.hip import ops as dops
    from fugue_amd.hip.execution_engine import HipExecutionEngine
    from fugue_amd.hip.frame import DeviceColumn, HipDataFrame
    from fugue_amd.schema import Schema

    # one layout entry per variant must stay cached side by side
    dops._LAYOUT_MEMO_CAP = max(dops._LAYOUT_MEMO_CAP, len(FLAGSHIP_VARIANTS))

    engine = HipExecutionEngine()
    device = torch.device(engine.device)
    gen = torch.Generator(device=device)
    gen.manual_seed(42)
    n = 125_000_000
    fact = HipDataFrame.from_columns(
        {"k": DeviceColumn(torch.randint(0, 1_000_000, (n,),
                                         dtype=torch.int64, device=device,
                                         generator=gen), None, pa.int64()),
         "v": DeviceColumn(torch.rand(n, dtype=torch.float64, device=device,
                                      generator=gen), None, pa.float64())},
        Schema("k:long,v:double"), engine.device)
    dims = HipDataFrame.from_columns(
        {"k": DeviceColumn(torch.arange(0, 1_000_000, dtype=torch.int64,
                                        device=device), None, pa.int64()),
         "w": DeviceColumn(torch.rand(1_000_000, dtype=torch.float64,
                                      device=device, generator=gen),
                           None, pa.float64())},
        Schema("k:long,w:double"), engine.device)

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

    def flag_step():
        fa.fugue_sql(SQL, fact=fact, dims=dims, scale=scale, engine=engine,
                     as_fugue=True)

    run_ab(flag_step, "flagship", FLAGSHIP_VARIANTS)
    dops._LAYOUT_MEMO.clear()

    spec = importlib.util.spec_from_file_location(
        "q3b", os.path.join(os.path.dirname(__file__), "q3_bench.py"))
    q3 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(q3)
    customer, orders, lineitem, _ = q3.gen_tables(10.0, engine.device, 0)

    def q3_step():
        fa.fugue_sql(q3.Q3, customer=customer, orders=orders,
                     lineitem=lineitem, engine=engine, as_fugue=True)

    run_ab(q3_step, "q3", Q3_VARIANTS)


if __name__ == "__main__":
    main()
