"""GPU run of the engine-level join and set-operation cases of
``join_setop_refs.py``: the same frames as ``test_join_engine.py``, built
column by column on the device, through the join kernels (chained unique
walk, count + emit, open-addressed table, fused join-select), the hash
kernels and the distinct path.  Every comparison is exact, against the
plain-Python references.

The whole case list runs on the default path.  ``FUGUE_JOIN_OA=1`` and
``FUGUE_JOIN_UNIQUE=0`` pick other kernels for the same keys; they run on
every case too — the frames are small, and which cases a switch can
affect depends on the key route, the very thing under test."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not torch.cuda.is_available():
    pytest.skip("no GPU available", allow_module_level=True)

from fugue_amd.hip import ops as dops
from fugue_amd.hip.execution_engine import HipExecutionEngine

import join_setop_refs as R
from test_join_engine import HOST_CASES

SWITCHES = {
    "default": {},
    "open-addressed": {"FUGUE_JOIN_OA": "1"},
    "no-unique-walk": {"FUGUE_JOIN_UNIQUE": "0"},
}


@pytest.fixture(scope="module")
def engine():
    return HipExecutionEngine()


@pytest.fixture(autouse=True)
def _paths(monkeypatch):
    for name in ("FUGUE_JOIN_OA", "FUGUE_JOIN_UNIQUE", "FUGUE_JOIN_FUSED"):
        monkeypatch.delenv(name, raising=False)
    dops._JOIN_BUILD_MEMO.clear()
    yield
    dops._JOIN_BUILD_MEMO.clear()


@pytest.mark.parametrize("switch", list(SWITCHES.keys()))
@pytest.mark.parametrize("name", R.join_case_names())
def test_join(monkeypatch, engine, name, switch):
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    R.check_join_case(
        engine, engine.device, R.join_cases()[name], monkeypatch,
        name in HOST_CASES,
    )


@pytest.mark.parametrize("op,distinct", R.SET_OPS)
@pytest.mark.parametrize("name", R.set_case_names())
def test_set_op(monkeypatch, engine, name, op, distinct):
    R.check_set_case(
        engine, engine.device, R.set_cases()[name], op, distinct, monkeypatch
    )


@pytest.mark.parametrize("name", list(R.sql_cases().keys()))
def test_sql_join_select_double_key(monkeypatch, name):
    e1 = R.check_sql_case(
        HipExecutionEngine, "cuda:0", R.sql_cases()[name], monkeypatch
    )
    # a unique double key is the fused kernel's input: the key is the
    # column's bit pattern, an exact int64 like the flagship's (NaN rows
    # are split off first, and the rows that stay carry no mask);
    # duplicated build keys take the join followed by the select
    want = 0 if name == "sql-double-dup" else 1
    assert e1.stats.get("join.fused_select") == want
