"""bench.py output obeys the driver contract."""
import json
import subprocess
import sys


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "8", "--distinct", "2", "--nodes", "20"],
        capture_output=True, text=True, timeout=600)
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in d, key
    assert d["metric"] == "episodes/sec"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["vs_baseline"] - d["value"] / 4.0) < 1e-6
    assert "global_batch" in d["config"] and "parallelism" in d["config"]


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float .npy
    files, identical from run to run for the same arguments; --full is
    accepted and leaves the result line's contract fields in place."""
    import os
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "3",
             "--warmup", "1", "--batch", "8", "--distinct", "2",
             "--nodes", "20", "--device", "cpu",
             "--dump-outputs", str(d)] + extra,
            capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        assert rec["metric"] == "episodes/sec" and rec["dtype"] == "fp64"
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert set(a) == set(b) == {"tau", "congest", "num_jobs", "delay_emp",
                                "loss_fn", "loss_mse", "params"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    assert a["tau"].shape == (8,) and a["delay_emp"].shape[0] == 8
    assert (a["num_jobs"] >= 1).all() and (a["tau"] > 0).all()
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
