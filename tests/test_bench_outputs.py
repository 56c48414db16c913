"""bench.py's plain run and --dump-outputs: the plain line carries the headline figure only, the dumped arrays are the last timed step's
outputs and repeat bit for bit from run to run, and --full adds the per-kernel and roofline figures without changing what is computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_dump_outputs_keeps_a_fixed_sample_within_the_limit(tmp_path):
    import bench
    n, limit = 50000, 1 << 20
    x = np.arange(3 * n, dtype=np.float64).reshape(n, 3)
    w = -np.arange(n, dtype=np.float64)
    names = bench.dump_outputs(str(tmp_path / "a"), {"loglik": [-1.25], "particles": x, "weights": w}, n_rows=n, limit=limit)
    assert names == ["loglik", "particles", "sample_rows", "weights"]
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= limit
    rows = np.load(tmp_path / "a" / "sample_rows.npy").astype(np.int64)
    assert 0 < rows.size < n and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "particles.npy"), x[rows]) and np.array_equal(np.load(tmp_path / "a" / "weights.npy"), w[rows])
    assert np.load(tmp_path / "a" / "loglik.npy").tolist() == [-1.25]
    bench.dump_outputs(str(tmp_path / "b"), {"loglik": [-1.25], "particles": x, "weights": w}, n_rows=n, limit=limit)
    assert np.array_equal(np.load(tmp_path / "b" / "sample_rows.npy"), rows.astype(np.float64))       # the same rows every run
    small = bench.dump_outputs(str(tmp_path / "c"), {"particles": x[:10], "weights": w[:10]}, n_rows=10, limit=limit)
    assert small == ["particles", "weights"] and np.array_equal(np.load(tmp_path / "c" / "particles.npy"), x[:10])


def test_steps_below_one_are_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--steps must be >= 1" in out.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_and_full_adds_the_figures(tmp_path):
    # (the filter's random stream runs on from pass to pass: the outputs are those of the same arguments, not of any step count)
    common = ["--particles", "20000", "--T", "60", "--warmup", "1", "--steps", "3"]
    a = _bench(common + ["--dump-outputs", str(tmp_path / "a")])
    b = _bench(common + ["--dump-outputs", str(tmp_path / "b")])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in a, key
    assert a["steps"] == 3 and a["ms_per_step"] > 0 and a["value"] == pytest.approx(3 * 20000 * 60 / (3 * a["ms_per_step"] * 1e-3))
    assert not {"roofline", "kernel_us", "cpu_baseline", "accuracy", "other_configs"} & set(a)
    for name in ("loglik", "particles", "weights"):
        da, db = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert da.dtype == np.float64 and np.array_equal(da, db), name
    assert np.load(tmp_path / "a" / "particles.npy").shape == (20000, 2)
    assert np.load(tmp_path / "a" / "loglik.npy")[0] == a["loglik"] == b["loglik"]
    full = _bench(common + ["--full", "--no-cpu-baseline"])
    assert "roofline" in full and "kernel_us" in full and full["loglik"] == a["loglik"]
