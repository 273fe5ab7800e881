"""Joins and set operations of ``HipExecutionEngine`` over every key type,
on CPU tensors: the engine's own Python (null split, key packing, float
bit keys, the hashed 128-bit route, build-side swap, output padding,
``_row_keys``) down to ``hash_join_indices``, which on CPU tensors takes
the ``_hash_join_indices_cpu`` twin of the kernels.
``test_join_engine_gpu.py`` runs the same cases through the kernels.

Every comparison is exact, against the plain-Python references of
``join_setop_refs.py`` (which ``test_join_setop_refs.py`` holds to the
native engine).  The ``FUGUE_JOIN_OA`` / ``FUGUE_JOIN_UNIQUE`` switches
select between kernels and are read on the GPU path only; they are
exercised in the GPU module."""
import pytest

from fugue_amd.hip.execution_engine import HipExecutionEngine

import join_setop_refs as R

# the only cases that may reach the host join: a float key against a key
# of another type has no exact common device key
HOST_CASES = {
    "mixed-long-double", "mixed-double-long",
    "mixed-float-double", "mixed-double-float",
}


def _engine() -> HipExecutionEngine:
    e = HipExecutionEngine()
    e._device = "cpu"  # CPU tensors also where a GPU is present
    return e


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for name in ("FUGUE_JOIN_OA", "FUGUE_JOIN_UNIQUE", "FUGUE_JOIN_FUSED"):
        monkeypatch.delenv(name, raising=False)


def test_host_cases_exist():
    assert HOST_CASES <= set(R.join_case_names())
    assert HOST_CASES <= set(R.MIXED_CASES)


@pytest.mark.parametrize("name", R.join_case_names())
def test_join(monkeypatch, name):
    R.check_join_case(
        _engine(), "cpu", R.join_cases()[name], monkeypatch, name in HOST_CASES
    )


@pytest.mark.parametrize("op,distinct", R.SET_OPS)
@pytest.mark.parametrize("name", R.set_case_names())
def test_set_op(monkeypatch, name, op, distinct):
    R.check_set_case(
        _engine(), "cpu", R.set_cases()[name], op, distinct, monkeypatch
    )


@pytest.mark.parametrize("name", list(R.sql_cases().keys()))
def test_sql_join_select_double_key(monkeypatch, name):
    R.check_sql_case(_engine, "cpu", R.sql_cases()[name], monkeypatch)
