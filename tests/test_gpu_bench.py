"""GPU: `bench.py --dump-outputs DIR` writes what the last timed step computed -- float32 / float64 .npy files, 64 MB at most --
and two runs with the same arguments store the same values (seeded inputs, weights and image-pool draws).  Each run is a child
process, as a user starts the benchmark."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--nb", "1", "--lr-size", "32", "--dtype", "fp32"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bench(config, out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "SRCGAN_FORCE_DIST")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, *SMALL, *extra, "--dump-outputs", str(out_dir)],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return line, arrays


@pytest.mark.parametrize("config,losses", [("paired", ("loss_G", "loss_D")), ("cycle", ("loss_G",))])
def test_dump_outputs_is_the_last_step_and_reproducible(tmp_path, config, losses):
    line, a = _bench(config, tmp_path / "a")
    assert line["steps"] == 2 and line["warmup"] == 1
    assert a and all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert all(np.isfinite(v).all() for v in a.values())
    for k in losses:                                     # the JSON line reads the same step's losses
        assert float(a[k]) == line[k]
    _, b = _bench(config, tmp_path / "b")
    _same(a, b)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape, k
        scale = max(float(np.abs(a[k]).max()), 1e-30)
        assert float(np.abs(a[k].astype(np.float64) - b[k]).max()) <= 1e-4 * scale, k


def test_full_adds_profile_and_cpu_baseline_after_the_same_steps(tmp_path):
    """A plain run measures the headline alone; `--full` adds the per-kernel profile step and the CPU oracle baseline after the
    timed steps and the dump, so its line carries both and what its timed steps computed is what a plain run computes."""
    plain, a = _bench("paired", tmp_path / "plain")
    assert plain["roofline"] is None and plain["kernels"] == [] and plain["cpu_baseline"] is None
    full, b = _bench("paired", tmp_path / "full", "--full")
    assert full["roofline"] is not None and full["roofline"]["achieved"] > 0 and full["kernels"]
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["c1"]["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert full[k] == plain[k], k
    for k in ("loss_G", "loss_D"):                       # read before the profile step
        assert float(b[k]) == full[k]
    _same(a, b)
