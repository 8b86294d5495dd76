"""The bench line contract, checked on the lines committed under profiles/ (no GPU needed):
one JSON object with the driver's fields, a `roofline` object for the dominant kernel and a
`cpu_baseline` object; `config` names a workload (no model keys)."""
import glob
import json
import os

import pytest

from conftest import ROOT

LINES = sorted(glob.glob(os.path.join(ROOT, "profiles", "r01f_bench_*.json")) + glob.glob(os.path.join(ROOT, "profiles", "r02x_bench_*.json")) +
               [os.path.join(ROOT, "profiles", f) for f in ("r03n_bench_default_iterative_schur.json", "r03zb_bench_default_iterative_schur.json", "r03zm_bench_default_iterative_schur.json",
                                                          "r03zq_bench_default_iterative_schur.json", "r03p_bench_cgnr.json",
                                                          "r04a_bench_default_iterative_schur.json", "r04l_bench_default_iterative_schur.json",
                                                          "r04_final_bench_default_iterative_schur.json", "r05_final_bench_default_iterative_schur.json",
                                                          "r05_final_bench_under_rocprof_iterative_schur.json", "r05_final_bench_under_rocprof_cgnr.json",
                                                          "r05x_bench_default_iterative_schur_second_box.json",
                                                          "r06_final_bench_default_iterative_schur.json", "r06_final_bench_under_rocprof_iterative_schur.json",
                                                          "r06_final_bench_under_rocprof_cgnr.json")])


@pytest.mark.parametrize("path", LINES, ids=[os.path.basename(p) for p in LINES])
def test_committed_bench_lines_follow_the_contract(path):
    text = open(path).read().strip()
    assert "\n" not in text, "one JSON line"
    d = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["unit"] == "steps/s" and d["higher_is_better"] is True and d["scaling"] == "strong"
    assert d["vs_baseline"] is None            # BASELINE.md publishes no number for this metric
    two_ranks = "two_ranks" in path   # bench.py's N > 1 code path run with two ranks on ONE GPU (validation only, timings meaningless)
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["n_gpus"] == (2 if two_ranks else 1)
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-3)
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 * d["n_gpus"]   # whole-job peak
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], abs=1e-3)
    if not two_ranks:   # N > 1: `achieved` is the sum over ranks, bytes and time on the line are rank 0's shard
        assert r["achieved"] == pytest.approx(r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9, rel=1e-3)
    assert r["traffic"] is None or r["traffic"] > r["algorithmic_bytes_per_launch"]
    cpu = d.get("cpu_baseline")
    if "under_rocprof" not in path and "fp32" not in path and not two_ranks:   # profiled / fp32-storage / validation runs skip the CPU leg
        assert cpu and cpu["kind"] == "port" and cpu["unit"] == "steps/s" and cpu["cores"] >= 1 and cpu["value"] > 0
        assert "sample" in cpu
    if os.path.basename(path).startswith(("r02", "r03", "r04", "r05", "r06")):   # since round 2: what the traffic figure is, and the probe for real Ceres
        assert r["traffic"] is None or "profiles/" in r["traffic_source"]
        if cpu:
            assert "tools/probe.sh" in cpu["sample"]


@pytest.mark.parametrize("tag", ["r01f", "r02x"])
def test_default_line_carries_both_rooflines(tag):
    d = json.loads(open(os.path.join(ROOT, "profiles", f"{tag}_bench_default_iterative_schur.json")).read())
    assert "kSx" in d["roofline"]["kernel"] and "kJtJx" in d["roofline_jtjx"]["kernel"]
    assert d["config"]["solver"].startswith("ITERATIVE_SCHUR")
    assert d["extra"]["cgnr"]["steps_per_s"] > 0


def test_round2_default_line_says_the_whole_truth():
    """VERDICT r01 "weak" 5 / 7: the host-boundary rate, the scene-valued trust-region rate and the provenance of the
    traffic figure are first-class fields of the N = 1 line; `value` stays the resident-inputs rate."""
    d = json.loads(open(os.path.join(ROOT, "profiles", "r02x_bench_default_iterative_schur.json")).read())
    hb, tr = d["host_boundary"], d["scene_trust_region"]
    assert hb["steps_per_s"] == pytest.approx(1e3 / hb["ms_per_step"], rel=1e-3) and hb["steps_per_s"] < d["value"] / 5
    assert hb["upload_ms"] < hb["ms_per_step"] and hb["bytes_h2d"] > 1e9
    assert tr["lm_iterations"] >= 1 and len(tr["cg_iterations"]) >= tr["lm_iterations"] and tr["ms_per_lm_iteration"] > d["ms_per_step"]
    assert d["config"]["inputs_resident_in_hbm"] is True


def test_synthetic10m_lines_name_the_many_camera_configuration():
    for storage in ("fp64", "fp32"):
        d = json.loads(open(os.path.join(ROOT, "profiles", f"r02x_bench_synthetic10M_{storage}.json")).read())
        assert d["config"]["workload"].startswith("synthetic10M") and d["config"]["jacobian_storage"].startswith(storage)
        assert d["config"]["camera_accumulators_in_lds"] is False and d["dtype"] == "f64"


def test_round3_default_line_carries_the_configurations_the_review_asked_for():
    """VERDICT r02 "next" 1d / 3c / 4 / 8 / 9: BASELINE.json configs[4] (synthetic10M) on the driver-style line, the roofline of the WHOLE step,
    the scene-valued steps at both eta, S.x / JtJx on real visibility, DENSE_SCHUR's factorisation with the ceiling it is measured against."""
    d = json.loads(open(os.path.join(ROOT, "profiles", "r03n_bench_default_iterative_schur.json")).read())
    e = d["extra"]
    s10 = e["synthetic10M"]
    assert s10["workload"].startswith("synthetic10M") and s10["sx"]["frac"] >= 0.40 and s10["jtjx"]["frac"] >= 0.40
    sr = d["step_roofline"]
    assert sr["bound"] == "hbm" and 0.3 < sr["frac"] < 1.0 and sr["frac"] == pytest.approx(sr["achieved"] / sr["peak"], abs=1e-3)
    assert set(d["scene_step"]) >= {"eta_0.1", "eta_0.01"}
    rg = e["real_graph"]["cases"]
    assert [c["hybrid"] for c in rg] == [0, 1] and rg[1]["observations_summed_in_lds"] > 0.9 and rg[1]["cameras"] > 50000
    dc = e["dense_schur_cholesky"]
    assert dc["n"] == 8190 and not dc["failed"] and dc["rel_err_of_solve"] < 1e-12
    assert dc["frac_of_datasheet_peak"] == pytest.approx(dc["TFLOPs"] / 78.6, abs=1e-3) and dc["frac_of_datasheet_peak"] < 0.30   # said plainly: the 30 % is not met
    assert d["roofline"]["frac"] >= 0.65 and d["roofline_jtjx"]["frac"] >= 0.60


def test_end_of_round3_line_has_the_long_points_in_rounds():
    """The last default line of round 3: the real-visibility case (every point of the replicated libmv graph owns 3 - 7 tiles) runs with
    the long points taken in cooperative rounds — S.x at twice the fraction of the HBM peak it had with one wave per point (0.20)."""
    d = json.loads(open(os.path.join(ROOT, "profiles", "r03zq_bench_default_iterative_schur.json")).read())
    rg = d["extra"]["real_graph"]["cases"]
    assert rg[1]["hybrid"] == 1 and rg[1]["sx"]["frac"] >= 0.35 and rg[1]["jtjx"]["frac"] >= 0.30
    assert d["roofline"]["frac"] >= 0.70 and d["extra"]["cgnr"]["jtjx_frac_hbm"] >= 0.60
    assert d["extra"]["synthetic10M"]["sx"]["frac"] >= 0.40


def test_round4_default_line_fields():
    """Round 4: the host-boundary rate next to `value`, the retry after a rejected step, the conditioned workload in which CG dominates,
    the structures beyond <2,3,9>, the full-size oracle check of configs[4], and a trust-region iteration under 4.1 ms."""
    d = json.loads(open(os.path.join(ROOT, "profiles", "r04_final_bench_default_iterative_schur.json")).read())
    assert "gpu_over_cpu" not in d and d["value_host_boundary"] == pytest.approx(d["host_boundary"]["steps_per_s"], rel=1e-6)
    retry = d["host_boundary"]["retry_after_rejection"]
    assert retry["ms_per_step"] < 0.15 * d["host_boundary"]["ms_per_step"] and retry["device_pointer_retry_ms_per_step"] < d["ms_per_step"]
    cond = d["extra"]["conditioned_step"]["eta_0.0001"]
    assert cond["cg_iterations"] >= 15 and cond["cg_share_of_step"] > 0.8
    assert d["extra"]["synthetic10M"]["step_rel_diff_vs_oracle"] < 1e-9
    cases = d["extra"]["other_shapes"]["cases"]
    assert len(cases) >= 4 and all(c["lm_step"]["step_rel_diff_vs_oracle_iterate_of_the_same_index"] < 1e-9 for c in cases)
    assert sum(c["kernel_path"] == "fused" for c in cases) >= 3
    assert d["scene_trust_region"]["ms_per_lm_iteration"] < 4.1
    assert d["config"]["collectives_per_step"] == 0   # one rank
    two = json.loads([l for l in open(os.path.join(ROOT, "profiles", "r04_final_bench_self_launched_2ranks_ladybug_iterative_schur.json")) if l.startswith("{")][-1])
    assert two["n_gpus"] == 2 and two["config"]["collectives_per_step"] == 4 and two["oracle_check"]["step_rel_diff_vs_oracle"] < 1e-9


def test_round5_default_line_fields():
    """Round 5: the timed step itself checked against the oracle at full size ON the headline line (and the CPU leg's figure, which compared
    steps of different radii until round 4, agrees with it), the fp32-tile leg next to it, S.x at 0.74 of peak with its kernel at 0.79 under
    rocprofv3 (the camera part of x for the popular cameras in LDS), CGNR's iteration under 0.30 ms, shapes of every row height / point width."""
    d = json.loads(open(os.path.join(ROOT, "profiles", "r05_final_bench_default_iterative_schur.json")).read())
    oc = d["oracle_check"]
    assert oc["observations"] == 5001946 and oc["step_rel_diff_vs_oracle"] < 1e-9 and oc["cg_iterations_gpu"] == oc["cg_iterations_oracle"]
    assert d["cpu_baseline"]["step_rel_diff_vs_gpu"] < 1e-9
    f32 = d["extra"]["fp32_tiles"]
    assert 1e-8 < f32["step_rel_diff_vs_fp64"] < 1e-5 and f32["sx_frac_hbm_of_fp32_bytes"] > 0.55 and f32["steps_per_s"] > d["value"]
    assert d["roofline"]["frac"] >= 0.73 and d["roofline_jtjx"]["frac"] >= 0.65 and d["value"] > 670
    assert d["extra"]["back_substitute_ms"] <= 0.205
    shapes = " ".join(c["structure"] for c in d["extra"]["other_shapes"]["cases"])
    assert "<2,4,9>" in shapes and "<3,3,3>" in shapes and all(c["lm_step"]["step_rel_diff_vs_oracle_iterate_of_the_same_index"] < 1e-9 for c in d["extra"]["other_shapes"]["cases"])
    # the rocprofv3 run of the same tree: S.x kernel + partial reduction = the line's launch time
    import csv
    rows = {r["Name"]: r for r in csv.DictReader(open(os.path.join(ROOT, "profiles", "r05_final_kernel_stats_iterative_schur_venice.csv")))}
    sx = [float(r["AverageNs"]) for n, r in rows.items() if "bal_stream_kernel<0, true, true, false>" in n][0]
    red = [float(r["AverageNs"]) for n, r in rows.items() if "bal_reduce_partials_kernel" in n][0]
    under = json.loads(open(os.path.join(ROOT, "profiles", "r05_final_bench_under_rocprof_iterative_schur.json")).read())
    assert (sx + red) * 1e-6 == pytest.approx(under["roofline"]["avg_launch_ms"], rel=0.03)
    assert 1072463720 / (sx * 1e-9) / 8e12 >= 0.78        # the tile pass alone
    cg = json.loads(open(os.path.join(ROOT, "profiles", "r05_final_long_cg_30_iterations_venice.jsonl")).read())
    assert cg["cgnr_cg_ms"] / cg["cgnr_its"] < 0.30 and cg["schur_cg_ms"] / cg["schur_its"] < 0.205


@pytest.mark.parametrize("solver,collectives", [("iterative_schur", 4), ("cgnr", 7)])
def test_round5_two_rank_lines_at_the_headline_size(solver, collectives):
    """`python bench.py --gpus 2` typed without a launcher (two ranks sharing one GPU: validation mode) on the Venice shape — shards large
    enough for the LDS copies of x to be on — the assembled step against the oracle at full size."""
    d = json.loads(open(os.path.join(ROOT, "profiles", f"r05w_bench_self_launched_2ranks_venice_{solver}.json")).read())
    assert d["n_gpus"] == 2 and d["config"]["collectives_per_step"] == collectives
    oc = d["oracle_check"]
    assert oc["ranks"] == 2 and oc["observations"] == 5001946 and oc["step_rel_diff_vs_oracle"] < 1e-9 and oc["cg_iterations_gpu"] == oc["cg_iterations_oracle"]


def test_round6_default_line_carries_what_the_review_asked_for():
    """VERDICT r05 "next" 1 / 2 / 4 / 5: the strong-scaling ceiling measured on one GPU, the streamed upload at the plugin boundary, the
    banded many-camera workload and BASELINE.json configs[1] / configs[2] are fields of the N = 1 line."""
    d = json.loads(open(os.path.join(ROOT, "profiles", "r06_final_bench_default_iterative_schur.json")).read())
    sc = d["extra"]["shard_ceiling"]
    assert [c["ranks"] for c in sc["cases"]] == [2, 4, 8] and "NOT measured" in sc["what"]
    for c in sc["cases"]:
        assert c["efficiency_ceiling"] == pytest.approx(sc["t1_ms"] / (c["ranks"] * c["ms_per_step"]), rel=2e-3)
        assert c["efficiency_with_link_estimate"] < c["efficiency_ceiling"] and c["collectives_per_step"] >= 4
    st = d["host_boundary"]["streamed"]
    assert st["ms_after_last_push"] < d["host_boundary"]["ms_per_step"] / 3 and st["bytes_sent_in_end"] == 0 and st["step_rel_diff_vs_plain_step"] < 1e-12
    b = d["extra"]["banded50k"]
    assert b["cameras"] == 50000 and b["observations_summed_in_lds"] > 0.9 and 0 < b["sx"]["frac"] < 1
    cases = d["extra"]["configs"]["cases"]
    assert cases[0]["solver"].startswith("CGNR") and "dubrovnik16" in cases[0]["workload"] and cases[1]["solver"].startswith("ITERATIVE_SCHUR") and "ladybug1723" in cases[1]["workload"]
    for c in cases:
        assert c["step_rel_diff_vs_oracle"] < 1e-9 and c["cpu_port"]["steps_per_s"] > 0 and c["steps_per_s"] == pytest.approx(1e3 / c["ms_per_step"], rel=1e-2)
    assert d["extra"]["synthetic10M"]["shard_ceiling"]["cases"][0]["ranks"] == 8


def test_dump_outputs_stays_within_its_budget_and_repeats(tmp_path):
    """bench.py --dump-outputs: float64 .npy files, at most 64 MB together; a vector larger than that becomes the same seeded sample of
    its entries on every run (bench.dump_outputs in a child process: importing bench.py sets OpenMP variables for its CPU leg)."""
    import subprocess
    import sys
    import numpy as np
    code = f'''
import sys; sys.path.insert(0, {ROOT!r})
import numpy as np
import bench
for d in ("a", "b"):
    bench.dump_outputs({str(tmp_path)!r} + "/" + d, {{"step": np.arange(10_000_000, dtype=np.float64), "model_cost_change": [2.5],
                                                     "num_iterations": [7]}})
'''
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1000:]
    for d in ("a", "b"):
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["model_cost_change.npy", "num_iterations.npy", "step.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= 64_000_000
    step = np.load(tmp_path / "a" / "step.npy")
    assert step.dtype == np.float64 and 7_000_000 < step.size < 8_000_000
    assert (np.diff(step) > 0).all() and step[0] >= 0 and step[-1] < 10_000_000 and (step == np.round(step)).all()   # sorted entries
    assert np.array_equal(step, np.load(tmp_path / "b" / "step.npy"))
    assert np.load(tmp_path / "a" / "model_cost_change.npy").tolist() == [2.5]
    assert np.load(tmp_path / "a" / "num_iterations.npy").tolist() == [7.0]
