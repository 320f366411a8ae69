"""The driver's bench contract: `python bench.py` must print ONE JSON line
with the exact keys BASELINE.json's harness expects. Guarded here so no
refactor silently breaks round-end measurement."""

import json
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


@pytest.mark.timeout(600)
def test_bench_json_contract_tiny():
    proc = subprocess.run(
        [sys.executable, "bench.py", "--model", "tiny", "--src-size", "64",
         "--scale", "2", "--tile", "32", "--steps", "1", "--warmup", "0",
         "--sampler-steps", "1", "--tile-batch", "4"],
        cwd=ROOT, capture_output=True, text=True, timeout=540,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    json_lines = [ln for ln in proc.stdout.splitlines()
                  if ln.startswith("{")]
    assert len(json_lines) == 1, proc.stdout
    data = json.loads(json_lines[0])
    assert REQUIRED_KEYS.issubset(data), REQUIRED_KEYS - set(data)
    assert data["value"] > 0 and data["ms_per_step"] > 0
    assert data["n_gpus"] == 1 and data["steps"] == 1
    assert data["higher_is_better"] is True
    assert data["scaling"] == "weak"
    assert data["unit"] == "tiles/s"
    assert data["data"] == "synthetic"
    cfg = data["config"]
    for key in ("model", "global_batch", "parallelism"):
        assert key in cfg, key


@pytest.mark.timeout(600)
def test_bench_dump_outputs_is_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's canvas as float32 .npy,
    identical between two runs with the same arguments; --full is accepted
    and leaves the single JSON result line intact."""
    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out = tmp_path / name
        proc = subprocess.run(
            [sys.executable, "bench.py", "--model", "tiny", "--src-size", "64",
             "--scale", "2", "--tile", "32", "--steps", "2", "--warmup", "0",
             "--sampler-steps", "1", "--tile-batch", "4",
             "--dump-outputs", str(out), *extra],
            cwd=ROOT, capture_output=True, text=True, timeout=540,
        )
        assert proc.returncode == 0, proc.stderr[-2000:]
        json_lines = [ln for ln in proc.stdout.splitlines()
                      if ln.startswith("{")]
        assert len(json_lines) == 1, proc.stdout
        data = json.loads(json_lines[0])
        assert REQUIRED_KEYS.issubset(data)
        assert data["steps"] == 2 and data["ms_per_step"] > 0
        files = sorted(p.name for p in out.iterdir())
        assert files == ["canvas.npy"], files
        dumps.append(np.load(out / "canvas.npy"))
    a, b = dumps
    assert a.dtype == np.float32 and a.shape == (1, 128, 128, 3)
    assert np.isfinite(a).all()
    assert a.nbytes <= 64 * 1024 * 1024
    # the CPU path is exactly deterministic
    assert np.array_equal(a, b)


def test_bench_dump_samples_large_outputs(tmp_path):
    """An output above the dump budget is reduced to a fixed, seeded sample."""
    import numpy as np
    import torch

    import bench  # conftest puts the repository root on sys.path

    n =bench.DUMP_MAX_ELEMENTS + 12345
    big = torch.arange(n, dtype=torch.float32).reshape(1, -1)
    small = torch.ones(2, 3, dtype=torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "x"), {"big": big})
    bench.dump_outputs(str(tmp_path / "y"), {"big": big, "small": small})
    x = np.load(tmp_path / "x" / "big.npy")
    y = np.load(tmp_path / "y" / "big.npy")
    s = np.load(tmp_path / "y" / "small.npy")
    assert x.dtype == np.float32 and x.shape == (bench.DUMP_MAX_ELEMENTS,)
    assert y.shape == (bench.DUMP_MAX_ELEMENTS // 2,)
    assert (np.diff(x) >= 0).all() and x.max() < n  # sorted, in range
    assert s.dtype == np.float32 and s.shape == (2, 3)
    assert x.nbytes <= 64 * 1024 * 1024
    bench.dump_outputs(str(tmp_path / "z"), {"big": big})
    assert np.array_equal(x, np.load(tmp_path / "z" / "big.npy"))


@pytest.mark.timeout(600)
def test_bench_generation_branch_contract():
    """The seed-parallel generation branch (gen-sdxl / gen-flux / wan-t2v
    presets) also honors the JSON contract."""
    proc = subprocess.run(
        [sys.executable, "bench.py", "--config", "gen-flux", "--model",
         "flux_tiny", "--steps", "1", "--warmup", "0",
         "--sampler-steps", "1"],
        cwd=ROOT, capture_output=True, text=True, timeout=540,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    json_lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(json_lines) == 1, proc.stdout
    data = json.loads(json_lines[0])
    assert REQUIRED_KEYS.issubset(data)
    assert data["unit"] == "images/s" and data["value"] > 0
