"""bench.py command line on tiny synthetic data (single process):
``--steps`` sets the timed step count, the result line carries
``ms_per_step``, ``--dump-outputs`` writes the last step's result columns
reproducibly, and the secondary figures appear only with ``--full``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 20000


def _bench(*args: str) -> dict:
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--rows", str(ROWS), *args],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300,
    )
    assert res.returncode == 0, (
        f"bench.py failed\nSTDOUT:\n{res.stdout[-4000:]}\n"
        f"STDERR:\n{res.stderr[-4000:]}"
    )
    lines = [x for x in res.stdout.strip().splitlines() if x.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _load(directory: str) -> dict:
    names = sorted(os.listdir(directory))
    assert names == ["k.npy", "n.npy", "s.npy", "w.npy"]
    cols = {x[:-4]: np.load(os.path.join(directory, x)) for x in names}
    order = np.argsort(cols["k"], kind="stable")
    return {k: v[order] for k, v in cols.items()}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dump_a"))
    rec = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", d)
    return rec, d


def test_plain_result_line(plain_run):
    rec, _ = plain_run
    assert rec["metric"] == "rows_per_sec_transform_fuguesql_groupby_join"
    assert rec["unit"] == "rows/s"
    assert rec["higher_is_better"] is True
    assert rec["dtype"] == "int64+fp64"
    assert rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0
    # value and ms_per_step describe the same timed window
    assert rec["value"] == pytest.approx(
        ROWS / (rec["ms_per_step"] / 1000.0), rel=1e-9
    )
    assert "engine_ops_ms_per_step" not in rec["config"]


def test_dump_outputs_columns(plain_run):
    rec, d = plain_run
    cols = _load(d)
    for v in cols.values():
        assert v.dtype == np.float64
        assert v.shape == (rec["config"]["out_rows"],)
    # rows are written in key order, whatever order the engine emitted
    assert (np.diff(np.load(os.path.join(d, "k.npy"))) > 0).all()
    # group keys are unique, counts sum to at most the fact rows, filter held
    assert len(np.unique(cols["k"])) == len(cols["k"])
    assert 0 < cols["n"].sum() <= ROWS
    assert (cols["s"] > cols["w"]).all()


def test_dump_outputs_reproducible_and_full(plain_run, tmp_path):
    _, d = plain_run
    d2 = str(tmp_path / "dump_b")
    rec = _bench("--steps", "2", "--warmup", "0", "--full",
                 "--dump-outputs", d2)
    assert rec["steps"] == 2
    assert rec["config"]["engine_ops_ms_per_step"] > 0
    a, b = _load(d), _load(d2)
    # same seeded inputs: keys, counts and dimension values are exact;
    # each sum adds a handful of fp64 terms whose order may differ
    for name in ("k", "n", "w"):
        assert np.array_equal(a[name], b[name])
    np.testing.assert_allclose(a["s"], b["s"], rtol=1e-12, atol=0)
