#!/usr/bin/env python3
"""What inner iterations cost and give the BAL front end (ceres_hip_bal_set_inner_iterations): on the scene bench.py minimizes
(bal_scene(<workload>, seed=38401, skew=0.6)), one points pass and one cameras pass (ceres_hip_bal_inner_iterate, bracketed by HIP
events on the handle's device: the pass's kernels plus the two cost evaluations around it), the distribution of LM iterations per
block, and minimize(max_num_iterations=K) with and without AUTOMATIC.  One JSON line per measurement, then a summary of medians.
The per-kernel split of a pass: rocprofv3 --kernel-trace --stats -- python tools/inner_iteration_times.py ...

  python tools/inner_iteration_times.py [workload ...] [--rounds N] [--iterations K]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("ceres-solver_amd")
hs = pkg.hip_solver

ap = argparse.ArgumentParser()
ap.add_argument("workloads", nargs="*", default=["venice1778", "banded50k"])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iterations", type=int, default=8, help="max_num_iterations of each minimize")
args = ap.parse_args()

import torch  # noqa: E402  (HIP events: hs.load_library() loads torch first in this process)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)


def scene(name):
    if name == "banded50k":   # bench.py's extra.banded50k: synthetic1M's block counts (50 000 cameras), points seen by consecutive cameras
        bc, bpt, bo = pkg.problems.BAL_SHAPES["synthetic1M"]
        return pkg.problems.bal_scene(None, seed=38401, visibility="banded", num_cameras=bc, num_points=bpt, num_observations=bo)
    return pkg.problems.bal_scene(name, seed=38401, skew=0.6)


summary = {}
for wl in args.workloads:
    nc, npt, cam_i, pt_i, obs, par = scene(wl)
    bp = hs.BalProblem(hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, min_num_iterations=0,
                                              max_num_iterations=500), nc, npt, cam_i, pt_i, obs)
    x0 = bp.state_from_bal(par)
    passes = {k: [] for k in ("points", "cameras")}
    mins = {k: [] for k in ("none", "automatic")}
    its_hist = {}
    for kind in passes:   # warm-up (and the lists' first build)
        bp.set_inner_iterations(kind)
        bp.inner_iterate(x0)
    for rnd in range(args.rounds):
        for kind in passes:
            bp.set_inner_iterations(kind)
            (x, c0, c1, its), ms, wall = timed(lambda: bp.inner_iterate(x0))
            passes[kind].append(ms)
            sel = its[its >= 0]
            its_hist[kind] = {"mean": float(sel.mean()), "p50": int(np.percentile(sel, 50)), "p90": int(np.percentile(sel, 90)),
                              "max": int(sel.max()), "zero": int(np.sum(sel == 0)), "at_limit": int(np.sum(sel >= 50))}
            print(json.dumps({"workload": wl, "round": rnd, "pass": kind, "ms": round(ms, 3), "wall_ms": round(wall, 3), "cost_before": c0,
                              "cost_after": c1, "iterations": its_hist[kind]}), flush=True)
        for kind in mins:
            bp.set_inner_iterations(None if kind == "none" else kind)
            _, S = bp.minimize(x0, max_num_iterations=args.iterations)
            steps, secs, groups = bp.inner_iteration_stats()
            rec = {"outer_iterations": S.num_successful_steps + S.num_unsuccessful_steps, "final_cost": S.final_cost,
                   "total_seconds": S.total_seconds, "inner_steps": steps, "inner_seconds": secs, "groups": groups}
            mins[kind].append(rec)
            print(json.dumps({"workload": wl, "round": rnd, "minimize": kind, "initial_cost": S.initial_cost, **rec}), flush=True)
    summary[wl] = {"cameras": nc, "points": npt, "observations": int(cam_i.shape[0]),
                   "pass_ms_median": {k: round(statistics.median(v), 3) for k, v in passes.items()}, "block_iterations": its_hist,
                   "minimize_median": {k: {f: statistics.median(r[f] for r in v) for f in v[0]} for k, v in mins.items()}}
    bp.close()
print(json.dumps({"summary": summary}), flush=True)
