"""The one JSON line bench.py prints, as the driver reads it: checked on the lines committed under profiles/ (no GPU here
to print a fresh one).  A line that loses a field of the contract - or reports a rate its own step time does not give -
would otherwise only be noticed by the driver at round end."""
import glob
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINES = sorted(glob.glob(os.path.join(ROOT, "profiles", "r05*bench*.json")))


def _line(path):
    txt = [l for l in open(path).read().splitlines() if l.startswith("{")]
    return json.loads(txt[-1])


def test_committed_lines_exist():
    assert len(LINES) >= 4


@pytest.mark.parametrize("path", LINES, ids=[os.path.basename(p) for p in LINES])
def test_bench_line_contract(path):
    d = _line(path)
    for key, typ in (("metric", str), ("value", (int, float)), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", (int, float)), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                     ("config", dict)):
        assert isinstance(d[key], typ), key
    assert "vs_baseline" in d and d["vs_baseline"] is None          # BASELINE.md publishes no number for this metric
    assert d["metric"].startswith("Groth16 proofs/sec") and d["unit"] == "proofs/s" and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["data"] == "synthetic" and "workload" in d["config"]
    # value = whole-job proofs / the timed region: proofs per GPU and step x GPUs / step time
    per_step = d["config"]["proofs_per_gpu_per_step"] * d["n_gpus"]
    assert abs(d["value"] - per_step / (d["ms_per_step"] / 1e3)) <= 0.01 * d["value"]
    if "roofline" in d and d["roofline"]:
        r = d["roofline"]
        for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert key in r, key
        assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
        # achieved = algorithmic bytes per launch / the launch's average duration
        assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9) <= 0.01 * r["achieved"]
    if "cpu_baseline" in d and d["cpu_baseline"]:
        c = d["cpu_baseline"]
        for key in ("value", "unit", "cores", "kind", "sample"):
            assert key in c, key
        assert c["kind"] in ("port", "reference") and c["cores"] >= 1


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("zk_bench_dump", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_options():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in out.stdout, opt


def test_dump_outputs_exact_and_bounded(tmp_path, monkeypatch):
    """--dump-outputs: the proofs of a step as float32 byte values, row for row; above the size cap a fixed sample of rows
    with their indices, the same on every call."""
    import numpy as np
    bench = _bench_module()
    proofs = np.random.default_rng(3).integers(0, 256, size=(1000, 192), dtype=np.uint8)
    bench.dump_proofs(str(tmp_path / "all"), proofs.tobytes())
    assert sorted(os.listdir(tmp_path / "all")) == ["proofs.npy"]
    got = np.load(tmp_path / "all" / "proofs.npy")
    assert got.dtype == np.float32 and got.shape == (1000, 192)
    assert np.array_equal(got.astype(np.uint8), proofs)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 256 * 1024)
    for d in ("s1", "s2"):
        bench.dump_proofs(str(tmp_path / d), proofs.tobytes())
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 256 * 1024
    rows, idx = np.load(tmp_path / "s1" / "proofs.npy"), np.load(tmp_path / "s1" / "proofs_index.npy")
    assert idx.dtype == np.float64 and len(idx) == len(rows) and 0 < len(rows) < 1000
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(rows.astype(np.uint8), proofs[idx.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "proofs.npy"))
