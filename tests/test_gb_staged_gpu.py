"""The LDS-staged scatter and the chunk-strided phase-3 aggregate at a
small shape.  By default they only run from 48M rows up
(FUGUE_GB_STAGED_MIN_ROWS); here the threshold is 0 and n = 300_001
leaves a last partial scatter chunk and a last partial aggregate chunk.

Reference: ``torch.unique`` + ``scatter_add_`` in fp64 + ``bincount``.
Keys and counts must match exactly, sums within ``rtol=1e-12`` (atomic
order varies).  No key holds more than a few rows (the reference's
global atomics go quadratic on a hot key), and ``expected_groups`` does
not understate the group count (the global table's insert loop could not
finish)."""
import functools

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import pyarrow as pa  # noqa: E402

from fugue_amd.hip import ops as dops  # noqa: E402
from fugue_amd.hip.frame import DeviceColumn, HipDataFrame  # noqa: E402
from fugue_amd.schema import Schema  # noqa: E402

N = 300_001
GROUPS = 200_000


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(r, vals, uniq, ref_sum, ref_count) for a key shape; r in [0,
    GROUPS) is the group code every key shape is a bijection of.
    Computed once, never written to."""
    seed = {"fits": 1, "overflow": 2, "meta": 3}[shape]
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.randint(0, GROUPS, (N,), dtype=torch.int64, device="cuda",
                      generator=g)
    vals = torch.rand(N, dtype=torch.float64, device="cuda",
                      generator=g) * 4.0 - 1.0
    uniq, inv = torch.unique(r, return_inverse=True)
    ref_sum = torch.zeros(uniq.numel(), dtype=torch.float64, device="cuda")
    ref_sum.scatter_add_(0, inv, vals)
    ref_count = torch.bincount(inv, minlength=uniq.numel())
    assert int(ref_count.max()) < 300
    return r, vals, uniq, ref_sum, ref_count


def _key_columns(shape, r):
    """({name: key column}, schema, codes_of(key columns) -> r)"""
    if shape == "fits":  # speculative narrow, every key in [0, 2^31)
        return (
            {"k": DeviceColumn(r, None, pa.int64())}, "k:long",
            lambda cols: cols[0].data,
        )
    if shape == "overflow":  # speculative narrow overflows: wide redo
        keys = (r - 100_000) * 3_000_000_019
        assert int(keys.min()) < 0 and int(keys.max()) >= (1 << 31)
        return (
            {"k": DeviceColumn(keys, None, pa.int64())}, "k:long",
            lambda cols: cols[0].data // 3_000_000_019 + 100_000,
        )
    # two int32 columns packed into 9 + 9 bits: narrow known from meta
    a = (r // 400).to(torch.int32)
    b = (r % 400).to(torch.int32)
    return (
        {"a": DeviceColumn(a, None, pa.int32()),
         "b": DeviceColumn(b, None, pa.int32())}, "a:int,b:int",
        lambda cols: cols[0].data.to(torch.int64) * 400
        + cols[1].data.to(torch.int64),
    )


class _Recorder:
    """The extension with every ``gb_aggregate_partitioned`` call noted
    as (narrow argument, dtype of the spill keys it produced)."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def gb_aggregate_partitioned(self, **kw):
        out = self._ext.gb_aggregate_partitioned(**kw)
        assert not kw["record_layout"] and not kw["force_simple"]
        self.calls.append((kw["narrow"], out[4].dtype))
        return out


def _run(monkeypatch, parts, shape, aggs):
    monkeypatch.setenv("FUGUE_GB_STAGED_MIN_ROWS", "0")
    monkeypatch.setenv("FUGUE_GB_LAYOUT_REUSE", "0")
    monkeypatch.setenv("FUGUE_GB_PARTS", str(parts))
    rec = _Recorder(dops.get_ext())
    monkeypatch.setattr(dops, "get_ext", lambda: rec)
    r, vals, uniq, ref_sum, ref_count = _case(shape)
    cols, schema, codes_of = _key_columns(shape, r)
    names = list(cols)
    cols["v"] = DeviceColumn(vals, None, pa.float64())
    df = HipDataFrame.from_columns(
        cols, Schema(schema + ",v:double"), "cuda"
    )
    out_keys, out_aggs, out_count, meta = dops.groupby_aggregate(
        df, names, aggs, expected_groups=GROUPS
    )
    got = codes_of(
        dops.unpack_keys(out_keys, meta, [df.col(c) for c in names])
    )
    perm = torch.argsort(got)
    assert torch.equal(got.index_select(0, perm), uniq)
    assert torch.equal(out_count.index_select(0, perm), ref_count)
    if aggs:
        assert torch.allclose(
            out_aggs["s"].index_select(0, perm), ref_sum, rtol=1e-12
        )
    else:
        assert out_aggs == {}
    return rec.calls


_EXPECTED_CALLS = {
    "fits": [(-1, torch.int32)],
    "overflow": [(-1, torch.int32), (0, torch.int64)],
    "meta": [(1, torch.int32)],
}


@pytest.mark.parametrize("shape", ["fits", "overflow", "meta"])
@pytest.mark.parametrize("parts", [512, 1024, 2048])
def test_staged_sum(monkeypatch, parts, shape):
    calls = _run(monkeypatch, parts, shape, [("v", dops.AGG_SUM, "s")])
    assert calls == _EXPECTED_CALLS[shape]


def test_staged_count_only(monkeypatch):
    calls = _run(monkeypatch, 1024, "fits", [])
    assert calls == _EXPECTED_CALLS["fits"]
