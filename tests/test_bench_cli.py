"""bench.py's command line: a plain run times the headline step only, --full switches
the other measurements on, and --dump-outputs writes the destination of the last timed
step (whole, or a fixed seeded row sample above bench.DUMP_BYTES), which must be what the
oracle computes from the same seeds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, TABLES = 3000, len(bench.CRITEO_KAGGLE_ROWS)
LD = TABLES * bench.DIM
FULL_ONLY = ("cpu_baseline", "config2_gather", "config3_fp16", "config3_prepend16",
             "config4_zipf_update")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full and a.dump_outputs == "somewhere"


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_counts_that_cannot_be_timed_are_rejected(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_dump_sample_fits_the_size_limit():
    # the headline destination (65536 x 3328 fp32) is cut to whole rows under 64 MB
    keep = bench.DUMP_BYTES // (LD * 4)
    assert 0 < keep < bench.BATCH and keep * LD * 4 <= 64_000_000


# batch 64: the whole destination; batch 4000 (53 MB of fp32): the row sample
@pytest.mark.gpu
@pytest.mark.parametrize("batch,steps,warmup", [(64, 1, 0), (4000, 3, 1)])
def test_plain_run_dumps_the_oracle_result(batch, steps, warmup, tmp_path, oracle):
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", str(warmup), "--batch", str(batch), "--rows", str(ROWS),
           "--dump-outputs", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["warmup"] == warmup
    assert res["unit"] == "lookups/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(batch * TABLES * bench.POOL / (res["ms_per_step"] * 1e-3))
    assert not [k for k in FULL_ONLY if k in res] and "classes" not in res["roofline"]

    assert os.listdir(out) == ["maplookup_dst.npy"]
    got = np.load(os.path.join(out, "maplookup_dst.npy"))
    tabs = [oracle.fill_uniform((ROWS, bench.DIM), np.float32, bench.TABLE_SEED + t)
            for t in range(TABLES)]
    idx = [oracle.fill_index_uniform((batch, bench.POOL), ROWS, bench.INDEX_SEED + t)
           for t in range(TABLES)]
    want = oracle.maplookup_prealloc(tabs, idx)
    keep = bench.DUMP_BYTES // (LD * 4)
    if batch > keep:
        rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(batch, keep, replace=False))
        want = want[rows]
        assert res["dumped_outputs"]["maplookup_dst"]["rows_written"] == keep
    assert got.dtype == np.float32 and got.nbytes <= 64_000_000
    assert got.shape == want.shape and np.array_equal(got, want)
