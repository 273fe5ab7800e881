"""GPU tests of the segmented rank kernels (``seg_rank_*`` /
``seg_take_*``) against the torch-CPU implementation of the ops layer,
which ``test_segmented_rank.py`` pins to pandas.  Every size derives from
the kernels' chunk size, the block size and the wave size."""
from typing import Dict, List, Tuple

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

import fugue_amd.api as fa
from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine
from fugue_amd.hip.ext import get_ext
from fugue_amd.hip.frame import HipDataFrame
from fugue_amd.sql.api import fugue_sql

C = int(get_ext().seg_rank_chunk())
BLOCK = 256
WAVE = 64
SIZES = [
    1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1,
    C - 1, C, C + 1, 3 * C + 17,
]
LAYOUTS = ["one", "singletons", "chunk-start", "chunk-end", "random"]
KINDS = ["row_number", "rank", "dense_rank"]
TAKES = [1, 3, 10_000]


def _heads(layout: str, n: int, rng: np.random.Generator) -> np.ndarray:
    """Sorted positions at which a new segment starts."""
    if layout == "one":
        # no head after position 0: the carry crosses whole chunks
        return np.array([0])
    if layout == "singletons":
        return np.arange(n)
    if layout == "chunk-start":
        # segments start exactly at chunk starts and nowhere else
        return np.arange(0, n, C)
    if layout == "chunk-end":
        # a segment begun inside a chunk ends on the chunk's last
        # position; the next chunk opens with a singleton
        h = {0}
        for c0 in range(0, n, C):
            h.update((c0, c0 + C // 3, c0 + 1))
        return np.array(sorted(x for x in h if x < n))
    lens = rng.integers(1, 201, size=n)
    starts = np.concatenate([[0], np.cumsum(lens)])
    return starts[starts < n]


def _case(layout: str, n: int, seed: int) -> Dict[str, "torch.Tensor"]:
    """perm, pkeys and one int order column, all in original row order."""
    rng = np.random.default_rng(seed)
    heads = _heads(layout, n, rng)
    flag = np.zeros(n, dtype=np.int64)
    flag[heads] = 1
    seg = np.cumsum(flag) - 1
    # non-decreasing inside a segment with many duplicates (peers)
    step = rng.integers(0, 3, size=n) // 2
    order = np.cumsum(step)
    perm = rng.permutation(n)
    pkeys = np.empty(n, dtype=np.int64)
    ocol = np.empty(n, dtype=np.int64)
    # segment ids are scrambled so equal keys are only ever adjacent
    ids = rng.permutation(len(heads)).astype(np.int64) * 7919 - 3
    pkeys[perm] = ids[seg]
    ocol[perm] = order
    return dict(
        perm=torch.from_numpy(perm.astype(np.int64)),
        pkeys=torch.from_numpy(pkeys),
        ocol=torch.from_numpy(ocol),
    )


def _to_gpu(t: Dict[str, "torch.Tensor"]) -> Dict[str, "torch.Tensor"]:
    return {k: v.cuda() for k, v in t.items()}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_window_and_take_modes(n, layout):
    cpu = _case(layout, n, seed=n * 31 + len(layout))
    gpu = _to_gpu(cpu)
    for kind in KINDS:
        exp = dops.segmented_rank(
            cpu["perm"], cpu["pkeys"], [(cpu["ocol"], None)], kind
        )
        got = dops.segmented_rank(
            gpu["perm"], gpu["pkeys"], [(gpu["ocol"], None)], kind
        )
        assert got.is_cuda and got.dtype == torch.int64
        # original row order: position j holds row j's rank
        assert torch.equal(got.cpu(), exp), (kind, layout, n)
    for n_take in TAKES:
        exp = dops.take_per_group_indices(cpu["perm"], cpu["pkeys"], n_take)
        got = dops.take_per_group_indices(gpu["perm"], gpu["pkeys"], n_take)
        # exact index-vector equality: deterministic sorted-order emit
        assert torch.equal(got.cpu(), exp), (n_take, layout, n)


def test_row_number_lands_in_original_row_order():
    n = C + WAVE + 1
    cpu = _case("random", n, seed=5)
    got = dops.segmented_rank(
        cpu["perm"].cuda(), cpu["pkeys"].cuda(), [], "row_number"
    ).cpu()
    # recompute from the sorted side and scatter by hand
    ks = cpu["pkeys"][cpu["perm"]].numpy()
    rn = np.ones(n, dtype=np.int64)
    for i in range(1, n):
        rn[i] = rn[i - 1] + 1 if ks[i] == ks[i - 1] else 1
    exp = np.empty(n, dtype=np.int64)
    exp[cpu["perm"].numpy()] = rn
    np.testing.assert_array_equal(got.numpy(), exp)


def test_summary_scan_spans_more_than_one_tile():
    # more chunks than one scan tile holds
    n = C * (BLOCK + 3) + 17
    cpu = _case("random", n, seed=99)
    gpu = _to_gpu(cpu)
    exp = dops.segmented_rank(cpu["perm"], cpu["pkeys"], [], "row_number")
    got = dops.segmented_rank(gpu["perm"], gpu["pkeys"], [], "row_number")
    assert torch.equal(got.cpu(), exp)
    exp = dops.take_per_group_indices(cpu["perm"], cpu["pkeys"], 3)
    got = dops.take_per_group_indices(gpu["perm"], gpu["pkeys"], 3)
    assert torch.equal(got.cpu(), exp)


def test_long_single_segment_over_many_tiles():
    # one segment over more chunks than a scan tile: the carry has to
    # survive headless chunks AND the tile boundary of the scan
    n = C * (BLOCK + 2) + 1
    perm = torch.arange(n, dtype=torch.int64, device="cuda")
    pkeys = torch.zeros(n, dtype=torch.int64, device="cuda")
    got = dops.segmented_rank(perm, pkeys, [], "row_number")
    assert torch.equal(got, perm + 1)
    ocol = perm // 5
    got = dops.segmented_rank(perm, pkeys, [(ocol, None)], "dense_rank")
    assert torch.equal(got, ocol + 1)
    got = dops.segmented_rank(perm, pkeys, [(ocol, None)], "rank")
    assert torch.equal(got, ocol * 5 + 1)


def test_peer_comparison_two_columns():
    n = 3 * C + 17
    rng = np.random.default_rng(17)
    # the kernels compare neighbours; they do not need a real sort
    perm = torch.from_numpy(rng.permutation(n).astype(np.int64))
    pkeys = torch.empty(n, dtype=torch.int64)
    pkeys[perm] = torch.from_numpy(np.sort(rng.integers(0, n // 50 + 1, n)))
    a = torch.from_numpy(rng.integers(0, 2, n))
    a_valid = torch.from_numpy(rng.random(n) < 0.7)
    f = torch.from_numpy(
        rng.choice(np.array([0.0, -0.0, np.nan, 1.0]), size=n)
    )
    f_valid = torch.from_numpy(rng.random(n) < 0.8)
    cols_cpu = [(a, a_valid), (f, f_valid)]
    cols_gpu = [(x.cuda(), v.cuda()) for x, v in cols_cpu]
    for kind in ("rank", "dense_rank"):
        exp = dops.segmented_rank(perm, pkeys, cols_cpu, kind)
        got = dops.segmented_rank(perm.cuda(), pkeys.cuda(), cols_gpu, kind)
        assert torch.equal(got.cpu(), exp), kind
    # spot rules on a hand-made run: +0.0 == -0.0, NaN == NaN,
    # null == null whatever lies under it, null != value
    perm = torch.arange(8, dtype=torch.int64)
    pkeys = torch.zeros(8, dtype=torch.int64)
    f = torch.tensor([0.0, -0.0, float("nan"), float("nan"), 5.0, 6.0, 7.0, 7.0],
                     dtype=torch.float64)
    fv = torch.tensor([True, True, True, True, False, False, True, True])
    got = dops.segmented_rank(
        perm.cuda(), pkeys.cuda(), [(f.cuda(), fv.cuda())], "dense_rank"
    )
    assert got.cpu().tolist() == [1, 1, 2, 2, 3, 3, 4, 4]


def test_empty_input_launches_nothing():
    z = torch.zeros(0, dtype=torch.int64, device="cuda")
    assert dops.segmented_rank(z, z, [], "row_number").numel() == 0
    assert dops.take_per_group_indices(z, z, 3).numel() == 0


# ------------------------------------------------------------------ #
# end to end on the GPU engine                                         #
# ------------------------------------------------------------------ #
def _rows(pdf: pd.DataFrame) -> List[Tuple]:
    return sorted(map(tuple, pdf.to_numpy().tolist()))


@pytest.fixture(scope="module")
def engine():
    return HipExecutionEngine()


@pytest.fixture(scope="module")
def frame() -> pd.DataFrame:
    rng = np.random.default_rng(3)
    n = 100_003
    return pd.DataFrame(
        dict(
            k=rng.integers(0, 2000, n),
            g=rng.integers(0, 3, n).astype("int32"),
            v=rng.permutation(n).astype(np.float64),
        )
    )


def test_engine_take_partitioned(engine, frame):
    hdf = engine.to_df(frame)
    assert isinstance(hdf, HipDataFrame)
    before = engine.stats.get("take.device_partitioned")
    res = fa.take(
        hdf, 3, presort="v desc", partition=dict(by=["k", "g"]),
        engine=engine, as_fugue=True,
    )
    assert engine.stats.get("take.device_partitioned") == before + 1
    assert isinstance(res, HipDataFrame)
    exp = (
        frame.sort_values("v", ascending=False, kind="stable")
        .groupby(["k", "g"], sort=False)
        .head(3)
    )
    assert _rows(res.as_pandas()) == _rows(exp)


def test_sql_top3_per_group(engine, frame):
    before = engine.stats.get("window.device")
    sql = (
        "SELECT k, g, v FROM (SELECT *, ROW_NUMBER() OVER "
        "(PARTITION BY k ORDER BY v) AS rn FROM df) WHERE rn <= 3"
    )
    res = fugue_sql(sql, df=engine.to_df(frame), engine=engine, as_fugue=True)
    assert engine.stats.get("window.device") == before + 1
    exp = (
        frame.sort_values("v", kind="stable").groupby("k", sort=False).head(3)
    )
    assert _rows(res.as_pandas()) == _rows(exp[["k", "g", "v"]])
