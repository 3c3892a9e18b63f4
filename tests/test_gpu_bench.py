"""`python bench.py` without --full on a real MI355X: it times its steps and prints the headline line, and nothing of what --full
adds runs.  Each run is a subprocess of its own, as the benchmark is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

FULL_ONLY = ("dense_err_vs_fp32", "sustained", "full_model", "cfg5", "mixed", "eval_batch", "small_batch")


def _run(*flags, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, env=env,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [s for s in p.stdout.splitlines() if s.strip()]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_a_plain_run_prints_the_headline_and_runs_no_extra_leg(tmp_path):
    line = _run("--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path))
    bench.validate_line(line, full=False)
    assert line["metric"] == "GQA questions/sec" and line["unit"] == "questions/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(4096 * 1e3 / line["ms_per_step"], rel=1e-3)
    # what the timed steps gave without launches of their own stays: the roofline from their HIP events, their fallbacks
    assert line["roofline"]["launches_timed"] == 5 * 3 and line["roofline"]["achieved"] > 0
    assert line["fallbacks"]["torch_linear"] == 0
    assert line["roofline"]["unfused_kernel"] is None and line["cpu_baseline"] is None
    assert not [k for k in FULL_ONLY if k in line], line.keys()
    logits = np.load(tmp_path / "logits.npy")
    assert logits.shape == (4096, 1842) and np.isfinite(logits).all()
    assert line["dumped_outputs"]["arrays"]["logits"]["shape"] == [4096, 1842]


@pytest.mark.timeout(300)
def test_a_plain_captured_run_leaves_its_eager_roofline_steps_to_full():
    line = _run("--gpus", "1", "--graphs", "256", "--steps", "5", "--warmup", "2", "--launch", "graph")
    bench.validate_line(line, full=False)
    assert line["config"]["launch"].startswith("hipgraph") and line["ms_per_step"] > 0
    assert "roofline" not in line and line["fallbacks"] is None and line["config"]["edge_projection"] is None
    assert not [k for k in FULL_ONLY if k in line], line.keys()
