"""The plan of the partitioned (high-cardinality) group-by is a pure
function of the problem and the FUGUE_GB_* knobs: checked here without a
GPU.  The expected values are the rules of ``groupby_aggregate`` as they
stood before the plan was split out of it."""
import dataclasses

import pytest

from fugue_amd.hip.ops import _GbKnobs, _plan_partitioned

_KNOBS = (
    "FUGUE_GB_STAGED_MAX", "FUGUE_GB_PARTS", "FUGUE_GB_SCATTER_CHUNK",
    "FUGUE_GB_AGG_CHUNK", "FUGUE_GB_NARROW", "FUGUE_GB_STAGED_MIN_ROWS",
    "FUGUE_GB_LAYOUT_REUSE", "FUGUE_GB_REPLAY_DENSE", "FUGUE_GB_REPLAY_TILE",
    "FUGUE_GB_DENSE_SLOTS",
)

N = 125_000_000
EG = 1_000_000


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)


def _plan(n=N, eg=EG, n_aggs=1, fp64_sum=True, key_bits=None,
          key_range=None):
    return _plan_partitioned(
        n, eg, n_aggs, fp64_sum, key_bits, key_range, _GbKnobs.from_env()
    )


def test_default_plan():
    p = _plan()
    assert dataclasses.asdict(p) == dict(
        num_parts=1024, tsize=1 << 21, narrow=-1, force_simple=False,
        reuse=True, dense_ok=True, tile=8192, sc_chunk=0, ag_chunk=0,
    )
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.num_parts = 512
    # COUNT-only (no aggregates) is staged too, but records no layout
    p = _plan(n_aggs=0, fp64_sum=False)
    assert (p.num_parts, p.reuse, p.dense_ok, p.tile) == (1024, False, False, 0)


def test_table_size():
    assert _plan(eg=100_001).tsize == 1 << 18
    assert _plan(eg=131_072).tsize == 1 << 18
    assert _plan(eg=131_073).tsize == 1 << 19


@pytest.mark.parametrize(
    "env,parts", [("512", 512), ("1024", 1024), ("2048", 2048), ("777", 512)]
)
def test_parts_knob(monkeypatch, env, parts):
    monkeypatch.setenv("FUGUE_GB_PARTS", env)
    p = _plan()
    assert p.num_parts == parts and p.reuse


@pytest.mark.parametrize(
    "eg,parts",
    [(1_000_000, 2048), (200_000, 512), (100_001, 256), (5_000_000, 4096)],
)
def test_two_aggregates_use_the_generic_partition_count(eg, parts):
    p = _plan(eg=eg, n_aggs=2, fp64_sum=False)
    assert p.num_parts == parts
    assert not p.reuse and not p.dense_ok and p.tile == 0


def test_staged_max(monkeypatch):
    assert _plan(eg=1_200_000).num_parts == 1024
    p = _plan(eg=1_200_001)
    # min(4096, next_pow2(max(16, 1_200_001 // 512))) = next_pow2(2343)
    assert p.num_parts == 4096 and not p.reuse and not p.dense_ok
    monkeypatch.setenv("FUGUE_GB_STAGED_MAX", "150000")
    p = _plan(eg=150_001)
    assert p.num_parts == 512  # next_pow2(292)
    # 512 is one of the staged partition counts, so the layout is reusable
    assert p.reuse
    assert _plan(eg=400_000).num_parts == 1024  # next_pow2(781)
    assert _plan(eg=150_000).num_parts == 1024  # the knob's default


def test_narrow(monkeypatch):
    assert _plan(key_bits=31).narrow == 1
    assert _plan(key_bits=32).narrow == 0
    # pack meta wins over measured bounds
    assert _plan(key_bits=32, key_range=(0, 5)).narrow == 0
    assert _plan(key_range=(0, (1 << 31) - 1)).narrow == 1
    assert _plan(key_range=(0, 1 << 31)).narrow == 0
    assert _plan(key_range=(-1, 10)).narrow == 0
    assert _plan().narrow == -1
    monkeypatch.setenv("FUGUE_GB_NARROW", "0")
    assert _plan().narrow == 0
    assert _plan(key_bits=8).narrow == 0
    assert _plan(key_range=(0, 10)).narrow == 0


def test_force_simple(monkeypatch):
    assert _plan(n=47_999_999).force_simple
    assert not _plan(n=48_000_000).force_simple
    monkeypatch.setenv("FUGUE_GB_STAGED_MIN_ROWS", "0")
    assert not _plan(n=300_001).force_simple
    monkeypatch.setenv("FUGUE_GB_STAGED_MIN_ROWS", "300002")
    assert _plan(n=300_001).force_simple


def test_reuse(monkeypatch):
    assert _plan(n=(1 << 31) - 1).reuse
    p = _plan(n=1 << 31)
    assert not p.reuse and not p.dense_ok and p.tile == 0
    monkeypatch.setenv("FUGUE_GB_LAYOUT_REUSE", "0")
    p = _plan()
    assert not p.reuse and not p.dense_ok and p.tile == 0


def test_dense_ok(monkeypatch):
    # MIN, a nullable input and a non-fp64 input all reach the plan as
    # "not a null-free fp64 SUM"; MIN and nullable inputs never take the
    # partitioned path at all
    p = _plan(fp64_sum=False)
    assert p.reuse and not p.dense_ok and p.tile == 0
    monkeypatch.setenv("FUGUE_GB_REPLAY_DENSE", "0")
    p = _plan()
    assert p.reuse and not p.dense_ok and p.tile == 0


def test_fp64_sum_as_groupby_aggregate_derives_it():
    """The dense gate's input, from the frame: SUM of a null-free fp64
    column only."""
    torch = pytest.importorskip("torch")
    from fugue_amd.hip import ops as dops
    from fugue_amd.hip.frame import DeviceColumn, HipDataFrame  # noqa: F401

    n = 4
    f64 = torch.zeros(n, dtype=torch.float64)

    class _Frame:
        device = "cpu"

        def __init__(self, col):
            self._col = col

        def col(self, name):
            return self._col

    def fp64_sum(col, op):
        aggs = [("v", op, "s")]
        _, valids, _, zero_copy = dops._agg_inputs(
            _Frame(col), aggs, n, torch.device("cpu")
        )
        return valids is None and zero_copy and op == dops.AGG_SUM

    assert fp64_sum(DeviceColumn(f64, None, None), dops.AGG_SUM)
    assert not fp64_sum(DeviceColumn(f64, None, None), dops.AGG_MIN)
    assert not fp64_sum(
        DeviceColumn(f64, torch.ones(n, dtype=torch.bool), None),
        dops.AGG_SUM,
    )
    assert not fp64_sum(
        DeviceColumn(f64.to(torch.float32), None, None), dops.AGG_SUM
    )


def test_tile_knob(monkeypatch):
    assert _plan().tile == 8192
    monkeypatch.setenv("FUGUE_GB_REPLAY_TILE", "0")
    p = _plan()
    assert p.dense_ok and p.tile == 0
    monkeypatch.setenv("FUGUE_GB_REPLAY_TILE", "512")
    assert _plan().tile == 512
    monkeypatch.setenv("FUGUE_GB_REPLAY_TILE", "300")
    with pytest.raises(ValueError):
        _plan()


def test_chunk_and_slot_knobs(monkeypatch):
    monkeypatch.setenv("FUGUE_GB_SCATTER_CHUNK", "8192")
    monkeypatch.setenv("FUGUE_GB_AGG_CHUNK", "16384")
    p = _plan()
    assert (p.sc_chunk, p.ag_chunk) == (8192, 16384)
    assert _GbKnobs.from_env().dense_slots == 4096
    monkeypatch.setenv("FUGUE_GB_DENSE_SLOTS", "8192")
    assert _GbKnobs.from_env().dense_slots == 8192
    monkeypatch.setenv("FUGUE_GB_DENSE_SLOTS", "1000")
    assert _GbKnobs.from_env().dense_slots == 4096
