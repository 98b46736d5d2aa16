"""bench.py's plain run, --full and --dump-outputs (GPU): a plain run times its steps and prints the
line without the figures that need runs of their own; --full puts them back; --dump-outputs writes
what the last timed step computed, checked here against the oracle on a small pair whose rows are no
multiple of a strip (64 rows)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import ROOT

N, M = 1500, 1000  # text / pattern length: 16 strips of 64 rows, the last one partial


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], env=env,
                         capture_output=True, text=True, timeout=170)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return lines[0]


@pytest.mark.gpu
@pytest.mark.parametrize("workload,mode", [("headline", 0), ("local", 1)])
def test_plain_run_dumps_the_last_fill(tmp_path, workload, mode):
    from sa_amd import synthetic
    d = _bench("--workload", workload, "--size", str(N), "--pattern-len", str(M), "--steps", "3", "--warmup", "1",
               "--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0, d
    assert d["unit"] == "GCUPS" and d["higher_is_better"] is True and d["dtype"] == "int32", d
    assert abs(d["value"] - N * M / (d["ms_per_step"] * 1e-3) / 1e9) <= 0.01 * d["value"], d
    for moved in ("e2e_ms", "gcups_fill_plus_traceback", "cpu_baseline"):
        assert moved not in d, moved
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["directions_col_sums", "directions_row_sums", "directions_sample", "directions_sample_rows"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    exp = np.empty((M + 1) * (N + 1), np.uint8)
    oracle.fill_only(mode, synthetic.random_sequence(6, N, 4), synthetic.random_sequence(7, M, 4),
                     synthetic.blast_matrix(), 5, exp)
    exp = exp.reshape(M + 1, N + 1)
    rows = got["directions_sample_rows"].astype(np.int64)
    # (a matrix this small fits the sample whole: the seeded draw is then every row, in order)
    assert np.array_equal(rows, np.arange(M + 1))
    assert np.array_equal(got["directions_sample"], exp[rows].astype(np.float32))
    assert np.array_equal(got["directions_row_sums"], exp.sum(axis=1, dtype=np.int64).astype(np.float64))
    assert np.array_equal(got["directions_col_sums"], exp.sum(axis=0, dtype=np.int64).astype(np.float64))


@pytest.mark.gpu
def test_full_run_adds_traceback_and_cpu_baseline():
    from sa_amd import synthetic
    d = _bench("--size", str(N), "--pattern-len", str(M), "--steps", "2", "--warmup", "1", "--full")
    assert d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0, d
    assert d["e2e_ms"]["fill"] > 0 and d["e2e_ms"]["traceback"] > 0 and d["gcups_fill_plus_traceback"] > 0, d
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["unit"] == "GCUPS", d
    exp = oracle.align(0, synthetic.random_sequence(6, N, 4), synthetic.random_sequence(7, M, 4),
                       synthetic.blast_matrix(), 5)
    assert d["sample_result"]["pair0_score"] == exp["score"], d
