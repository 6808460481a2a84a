"""CPU: bench.py's option handling (a plain run is the headline only, --full switches the other legs on) and the
--dump-outputs writer (bench_local.dump_outputs): float64 files, a fixed sample above the size limit.  GPU: one
small run longer than the ring of pre-generated batches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import bench_local


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu and a.no_e2e and a.no_parity
    # the single switches cannot bring a leg back without --full
    a = _parse(monkeypatch, "--no-cpu")
    assert a.no_cpu and a.no_e2e and a.no_parity


def test_full_switches_every_leg_on_and_the_single_switches_off_again(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_cpu or a.no_e2e or a.no_parity)
    a = _parse(monkeypatch, "--full", "--no-e2e", "--dump-outputs", "d")
    assert a.no_e2e and not (a.no_cpu or a.no_parity) and a.dump_outputs == "d"


def test_dump_outputs_small_arrays_whole_as_float64(tmp_path):
    dec = np.array([0, 1, -1, 4], np.int8)
    wait = np.array([0, 2**31 - 1, -(2**31), 7], np.int32)
    bench_local.dump_outputs(str(tmp_path / "o"), 0, {"decision": dec, "wait_ms": wait})
    got = {p.name: np.load(p) for p in (tmp_path / "o").iterdir()}
    assert sorted(got) == ["decision.npy", "sample_index.npy", "wait_ms.npy"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert (got["decision.npy"] == dec).all() and (got["wait_ms.npy"] == wait).all()
    assert (got["sample_index.npy"] == np.arange(4)).all()


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench_local, "DUMP_SAMPLE", 100)
    a = np.arange(1000, dtype=np.int32) * 3
    for d in ("x", "y"):
        bench_local.dump_outputs(str(tmp_path / d), 1, {"a": a, "b": -a}, index="idx")
    x = {p.name: np.load(p) for p in (tmp_path / "x").iterdir()}
    y = {p.name: np.load(p) for p in (tmp_path / "y").iterdir()}
    assert sorted(x) == ["a.rank1.npy", "b.rank1.npy", "idx.rank1.npy"]
    idx = x["idx.rank1.npy"].astype(np.int64)
    assert 50 < len(idx) <= 100 and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < 1000
    assert (x["a.rank1.npy"] == a[idx]).all() and (x["b.rank1.npy"] == -a[idx]).all()
    assert all((x[k] == y[k]).all() and x[k].shape == y[k].shape for k in x)


@pytest.mark.gpu
def test_run_longer_than_the_batch_ring_stays_exact_and_dumps(tmp_path):
    """More warmup + timed steps than bench.RING_BATCHES at a small size: the run goes round the pre-generated
    batches in new virtual time, the first two timed batches (past the ring's end, in buffers of their own) match
    the oracle request for request, and the last step's results are dumped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    warm, steps = bench.RING_BATCHES + 1, 8
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warm), "--batch", str(1 << 16), "--rules", "20000", "--full", "--no-cpu",
                        "--no-e2e", "--dump-outputs", str(tmp_path / "o")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert (line["steps"], line["warmup"], line["config"]["distinct_batches"]) == (steps, warm, bench.RING_BATCHES)
    assert line["ms_per_step"] > 0 and line["cpu_baseline"] is None and line["end_to_end_host_buffers"] is None
    par = line["parity_sample"]
    assert par["timed_batches"] == [warm, warm + 1] and par["requests"] > 1 << 16 and par["mismatches"] == 0
    got = {p.name: np.load(p) for p in (tmp_path / "o").iterdir()}
    assert sorted(got) == ["remaining.npy", "sample_index.npy", "status.npy", "wait_in_ms.npy"]
    n = len(got["sample_index.npy"])
    assert n > 0 and all(v.dtype == np.float64 and v.shape == (n,) for v in got.values())
    assert abs(float((got["status.npy"] == 0).mean()) - line["ok_fraction_last_batch"]) < 1e-6


def test_dump_stays_under_the_size_limit():
    # at most four arrays and their index per call, 8 bytes per kept element
    assert 5 * 8 * bench_local.DUMP_SAMPLE <= 64 << 20
