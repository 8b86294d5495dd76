#!/usr/bin/env python3
"""What the dogleg trust region (ceres_hip_bal_set_trust_region_strategy) costs the BAL front end, on a DENSE_SCHUR scene
(bal_scene(None, seed=38401, skew=0.6) of C cameras, P points, O observations: DENSE_SCHUR takes at most 910 cameras):
- kernel level (ceres_hip_time_op, HIP events around back-to-back launches on device vectors): the dogleg pass over J
  (CERES_HIP_TIMED_JACOBIAN_GRAM) against the model-cost pass the LM step runs (CERES_HIP_TIMED_MODEL_COST: the kJx pass on the fused
  path), both on the loaded Jacobian;
- end to end: the operator entries ceres_hip_op_jacobian_gram and ceres_hip_op_right_multiply, host-vector copies (and the Gram
  entry's allocation) included;
- minimize(max_num_iterations=K) under LEVENBERG_MARQUARDT, traditional and subspace dogleg: seconds, num_linear_solves, final cost.
One JSON line per measurement, then a summary of medians.

  python tools/dogleg_times.py [CxPxO ...] [--rounds N] [--iterations K]"""
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
ap.add_argument("workloads", nargs="*", default=["256x40000x200000"])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iterations", type=int, default=10, help="max_num_iterations of each minimize")
ap.add_argument("--passes", type=int, default=20, help="back-to-back launches per timed pass")
args = ap.parse_args()

import torch  # noqa: E402  (HIP events: hs.load_library() loads torch first in this process)


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, 1e3 * (time.perf_counter() - t0) / reps


summary = {}
lib = hs.load_library()
for wl in args.workloads:
    C, Pn, O = (int(v) for v in wl.split("x"))
    nc, npt, cam_i, pt_i, obs, par = pkg.problems.bal_scene(None, seed=38401, skew=0.6, num_cameras=C, num_points=Pn, num_observations=O)
    bp = hs.BalProblem(hs.LinearSolverOptions(type=hs.DENSE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, min_num_iterations=0,
                                              max_num_iterations=500), nc, npt, cam_i, pt_i, obs)
    x0 = bp.state_from_bal(par)
    bp.evaluate(x0, jacobian=True)
    s = lib.ceres_hip_bal_linear_solver(bp._h)
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(bp.num_parameters), rng.standard_normal(bp.num_parameters)
    y = np.zeros(bp.num_residuals)
    out = np.zeros(5)
    P = hs._DP
    gram = lambda: lib.ceres_hip_op_jacobian_gram(s, a.ctypes.data_as(P), b.ctypes.data_as(P), out.ctypes.data_as(P))  # noqa: E731
    jx = lambda: lib.ceres_hip_op_right_multiply(s, a.ctypes.data_as(P), y.ctypes.data_as(P))  # noqa: E731
    passes = {"gram_kernel": [], "kjx_kernel": [], "gram_entry": [], "jx_entry": []}

    def time_op(op):
        ms = np.zeros(1)
        rc = lib.ceres_hip_time_op(s, op, args.passes, ms.ctypes.data_as(P))
        if rc != 0:
            raise hs.HipError(lib.ceres_hip_last_error(s).decode())
        return float(ms[0])
    mins = {k: [] for k in ("levenberg_marquardt", "traditional", "subspace")}
    gram(), jx()
    for rnd in range(args.rounds):
        bp.evaluate(x0, jacobian=True)   # (minimize leaves the last Jacobian loaded; the passes run on the start point's)
        for name, op in (("gram_kernel", hs.TIMED_JACOBIAN_GRAM), ("kjx_kernel", hs.TIMED_MODEL_COST)):
            ms = time_op(op)
            passes[name].append(ms)
            print(json.dumps({"workload": wl, "round": rnd, "pass": name, "ms": round(ms, 5)}), flush=True)
        for name, fn in (("gram_entry", gram), ("jx_entry", jx)):
            ms, wall = timed(fn, args.passes)
            passes[name].append(ms)
            print(json.dumps({"workload": wl, "round": rnd, "pass": name, "ms": round(ms, 4), "wall_ms": round(wall, 4)}), flush=True)
        for kind in mins:
            if kind == "levenberg_marquardt":
                bp.set_trust_region_strategy("levenberg_marquardt")
            else:
                bp.set_trust_region_strategy("dogleg", kind)
            _, S = bp.minimize(x0, max_num_iterations=args.iterations)
            rec = {"total_seconds": S.total_seconds, "linear_solver_seconds": S.linear_solver_seconds, "num_linear_solves": S.num_linear_solves,
                   "successful": S.num_successful_steps, "unsuccessful": S.num_unsuccessful_steps, "final_cost": S.final_cost}
            mins[kind].append(rec)
            print(json.dumps({"workload": wl, "round": rnd, "minimize": kind, "initial_cost": S.initial_cost, **rec}), flush=True)
    summary[wl] = {"cameras": nc, "points": npt, "observations": int(cam_i.shape[0]),
                   "pass_ms_median": {k: round(statistics.median(v), 5) for k, v in passes.items()},
                   "gram_over_kjx_kernel": round(statistics.median(passes["gram_kernel"]) / statistics.median(passes["kjx_kernel"]), 3),
                   "minimize_median": {k: {f: statistics.median(r[f] for r in v) for f in v[0]} for k, v in mins.items()}}
    bp.close()
print(json.dumps({"summary": summary}), flush=True)
