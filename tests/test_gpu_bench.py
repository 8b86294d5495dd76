"""bench.py end to end on the Dubrovnik-16 shape (small: seconds per run): a plain run prints the headline line and measures nothing
beyond it; `--full` runs the other legs after the same timed steps and fills their fields."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def run_bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "dubrovnik16", "--steps", "5", "--warmup", "2", *args]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("LM trust-region steps/sec") and d["unit"] == "steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["steps"] == 5 and d["warmup"] == 2
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-3)
    assert d["config"]["workload"].startswith("dubrovnik16") and d["config"]["step_finite"] is True
    assert 0 < d["step_roofline"]["frac"] < 1
    return d


@pytest.mark.gpu
def test_plain_bench_run_measures_the_headline_figure_alone(tmp_path):
    d = run_bench("--dump-outputs", str(tmp_path))
    assert d["full"] is False
    for k in ("roofline", "cpu_baseline", "oracle_check", "host_boundary", "scene_trust_region", "scene_step", "value_host_boundary"):
        assert d[k] is None, k
    assert "roofline_jtjx" not in d and set(d["extra"]) == {"set_structure_s", "device_bytes"}
    assert sorted(os.listdir(tmp_path)) == ["model_cost_change.npy", "num_iterations.npy", "residual_norm.npy", "step.npy",
                                            "termination_type.npy"]


@pytest.mark.gpu
def test_full_bench_run_fills_the_other_fields():
    # (live counter passes off: they run rocprofv3 in child processes; a short CPU leg)
    d = run_bench("--full", "--pmc-live", "0", "--cpu-seconds", "2")
    assert d["full"] is True
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["achieved"] == pytest.approx(r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9, rel=1e-3)
    assert d["roofline_jtjx"]["achieved"] > 0 and d["extra"]["cgnr"]["steps_per_s"] > 0
    assert d["oracle_check"]["step_rel_diff_vs_oracle"] < 1e-9
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0
    assert d["host_boundary"]["steps_per_s"] > 0 and d["scene_trust_region"]["lm_iterations"] >= 1
    assert d["extra"]["shard_ceiling"]["cases"] and "solve_phases_ms" in d["extra"]
