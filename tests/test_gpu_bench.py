"""A plain bench.py run (no --full) on small meshes: the timed steps and the result line only, and --dump-outputs writes what
the last timed step computed."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]


def _bench(args, out_dir):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--dump-outputs", str(out_dir)] + args,
                       capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {p.stem: np.load(p) for p in out_dir.glob("*.npy")}


def test_plain_obstacle_run_and_its_outputs(require_gpu, tmp_path):
    d, o = _bench(["--cells", "128", "--steps", "2", "--warmup", "1"], tmp_path)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Newton iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["roofline"] is None and "cpu_baseline" not in d and "vcycle_parts" not in d
    assert set(o) == {"u", "psi", "history"} and all(a.dtype == np.float64 for a in o.values())
    assert o["u"].shape == o["psi"].shape == (129 * 129,)
    h = o["history"]  # one row per proximal iteration of the last timed solve
    assert h.shape == (d["config"]["proximal_iterations_per_step"], 8)
    assert h[:, 4].sum() == d["config"]["newton_iterations_per_step"]
    assert np.all(np.isfinite(o["u"])) and np.linalg.norm(o["u"]) > 0


@pytest.mark.parametrize("workload,cells,latent", [("ex06", 24, "latent"), ("ex02", 6, "psi")])
def test_plain_lu_workload_run_and_its_outputs(require_gpu, tmp_path, workload, cells, latent):
    d, o = _bench(["--workload", workload, "--cells", str(cells), "--steps", "1", "--warmup", "1"], tmp_path)
    assert d["steps"] == 1 and d["ms_per_step"] > 0 and d["roofline"] is None and "cpu_baseline" not in d
    assert set(o) == {"u", latent, "newton_per_lvpp_step"}
    assert list(o["newton_per_lvpp_step"]) == d["config"]["newton_per_lvpp_step"]
    assert np.all(np.isfinite(o["u"])) and np.linalg.norm(o["u"]) > 0 and o[latent].size > 0
