#!/usr/bin/env python3
"""What the camera model costs the BAL front end (ceres_hip_bal_create_with_camera): the caller-layout evaluator through
ceres_hip_bal_evaluate — cost only, and with the Jacobian (evaluation, load into the solver, J^T r, the gradient's download) — and
ceres_hip_bal_minimize's time per iteration, for the angle-axis camera (tile-order evaluator, and the two-pass form with
CERES_HIP_EVAL_TILES=0), the quaternion camera and the quaternion manifold, on the scene bench.py minimizes
(bal_scene(<workload>, seed=38401, skew=0.6)).  Evaluate times are host wall-clock per call (the state's upload and the synchronisation
included).  The variants alternate in one process after a warm-up; one JSON line per measurement, then a summary line of medians.

  python tools/quaternion_times.py [workload] [--rounds N] [--iterations K] [--calls C]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("ceres-solver_amd")
hs = pkg.hip_solver

ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="venice1778")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iterations", type=int, default=8, help="max_num_iterations of each minimize")
ap.add_argument("--calls", type=int, default=20, help="evaluate calls per timing")
args = ap.parse_args()

nc, npt, cam_i, pt_i, obs, par = pkg.problems.bal_scene(args.workload, seed=38401, skew=0.6)
opts = hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, min_num_iterations=0, max_num_iterations=500)
VARIANTS = {"angle_axis": ("angle_axis", None), "angle_axis_two_pass": ("angle_axis", "0"), "quaternion": ("quaternion", None),
            "quaternion_manifold": ("quaternion_manifold", None)}
problems = {}
for name, (model, _) in VARIANTS.items():
    if model not in problems:
        bp = hs.BalProblem(opts, nc, npt, cam_i, pt_i, obs, camera_model=model)
        problems[model] = (bp, bp.state_from_bal(par))


def with_env(value, fn):
    old = os.environ.pop("CERES_HIP_EVAL_TILES", None)
    if value is not None:
        os.environ["CERES_HIP_EVAL_TILES"] = value
    try:
        return fn()
    finally:
        os.environ.pop("CERES_HIP_EVAL_TILES", None)
        if old is not None:
            os.environ["CERES_HIP_EVAL_TILES"] = old


def evaluate_us(bp, x, jacobian):
    bp.evaluate(x, gradient=jacobian)
    t0 = time.perf_counter()
    for _ in range(args.calls):
        bp.evaluate(x, gradient=jacobian)
    return 1e6 * (time.perf_counter() - t0) / args.calls


for name, (model, env) in VARIANTS.items():   # warm-up
    bp, x0 = problems[model]
    with_env(env, lambda: bp.minimize(x0, max_num_iterations=1))

ev = {k: {"cost_only": [], "jacobian": []} for k in VARIANTS}
it_ms = {k: [] for k in VARIANTS}
for rnd in range(args.rounds):
    for name, (model, env) in VARIANTS.items():
        bp, x0 = problems[model]
        if env is None:   # (evaluate is the caller-layout evaluator whatever the environment: measured once per camera model)
            for key, jac in (("cost_only", False), ("jacobian", True)):
                us = evaluate_us(bp, x0, jac)
                ev[name][key].append(us)
                print(json.dumps({"round": rnd, "what": "evaluate", "variant": name, "form": key, "us": round(us, 1)}), flush=True)
        _, S = with_env(env, lambda: bp.minimize(x0, max_num_iterations=args.iterations))
        n_it = S.num_successful_steps + S.num_unsuccessful_steps
        ms = 1e3 * S.total_seconds / max(1, n_it)
        it_ms[name].append(ms)
        print(json.dumps({"round": rnd, "what": "minimize", "variant": name, "iterations": n_it, "initial_cost": S.initial_cost,
                          "final_cost": S.final_cost, "ms_per_iteration": round(ms, 3), "evaluation_seconds": round(S.evaluation_seconds, 5),
                          "linear_solver_seconds": round(S.linear_solver_seconds, 5), "total_seconds": round(S.total_seconds, 5)}), flush=True)

summary = {"workload": args.workload, "observations": int(cam_i.shape[0]), "rounds": args.rounds,
           "evaluate_us_median": {k: {f: round(statistics.median(v), 1) for f, v in d.items() if v} for k, d in ev.items()},
           "minimize_ms_per_iteration_median": {k: round(statistics.median(v), 3) for k, v in it_ms.items()}}
print(json.dumps({"summary": summary}), flush=True)
for bp, _ in problems.values():
    bp.close()
