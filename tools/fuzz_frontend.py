#!/usr/bin/env python3
"""Randomised campaign on the BAL front end (GPU box): scenes of random size from the oracle's generator — the device
evaluator (cost, residuals, analytic Jacobian, gradient) against the oracle's dual numbers, and ceres_hip_bal_minimize against the
oracle's trust-region loop (same accept / reject sequence, CG counts within one, costs to 1e-6), both solvers.
--variants: the front end's other options (tests/test_gpu_frontend_matrix.py's factors: camera model, loss, trust-region strategy, linear
solver, inner iterations, Jacobi scaling, evaluator form) drawn at random among the allowed tuples, with that module's checks against the
composed restatement (tests/frontend_reference.py): the evaluation, one inner pass and the loop on a random edge scene
(test_gpu_frontend_matrix.edge_scene; the loop's costs, radii and state compared only where the restatement's own sensitivity to the
Jacobian's rounding, measured per case, allows: see EDGE_ILL_CONDITIONED), and the loop on a random clean scene (clean_scene).  One
JSON line per case, then the worst deviation of every check.
--masks: --variants with constant cameras and points drawn too (ceres_hip_bal_create_with_constant_blocks), with the checks of
tests/test_gpu_constant_blocks.py against tests/constant_blocks_reference.py: the evaluation, the fixed cost and one inner pass on a random
edge scene, the loop on a random clean scene (no case is excluded there).
usage: fuzz_frontend.py [first_seed] [count] [--variants | --masks]"""
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
oracle = entry.load_oracle()
hip = pkg.hip_solver
hip.load_library()
from test_gpu_bal_frontend import check_same_trajectory  # noqa: E402
from test_gpu_operators import rel  # noqa: E402


def run_case(seed):
    rng = np.random.default_rng(900007 * seed + 5)
    nc = int(rng.choice([3, 7, 16, 40, 65, 200, 700, 2600]))
    npts = int(rng.choice([20, 64, 65, 300, 1500, 5000]))
    per = float(rng.choice([2.0, 3.0, 5.0, 9.0]))
    nobs = int(min(max(2 * npts, per * npts), 0.8 * nc * npts))
    skew = float(rng.choice([0.0, 0.5, 1.0]))
    solver_type, pre = [(5, 2), (6, 1), (5, 1)][int(rng.integers(3))]
    out = dict(seed=seed, nc=nc, npts=npts, nobs=nobs, skew=skew, solver=[solver_type, pre])
    t0 = time.time()
    op = oracle.BalProblem.generate(nc, npts, nobs, seed=seed + 1, skew=skew, pixel_noise=float(rng.choice([0.1, 0.5, 2.0])), param_noise=float(rng.choice([0.005, 0.02])))
    bs, nelim = op.build_structure(True)
    cam, pt, obs = op.indices()
    o = hip.LinearSolverOptions(type=solver_type, preconditioner_type=pre, min_num_iterations=0, max_num_iterations=500)
    gp = hip.BalProblem(o, op.num_cameras, op.num_points, cam, pt, obs)
    worst = {}
    x0 = op.state()
    cost_o, res_o, vals_o = op.evaluate(x0)
    cost, res, grad, vals = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
    worst["cost"] = abs(cost - cost_o) / cost_o
    worst["residuals"] = float(rel(res, res_o))
    worst["jacobian"] = float(rel(vals, vals_o))
    worst["gradient"] = float(rel(grad, oracle.Matrix(bs, 0).left_multiply(vals_o, res_o)))
    Sa = op.lm_solve(solver_type=solver_type, preconditioner=pre, max_it=500, max_num_iterations=8)
    x, Sb = gp.minimize(x0, max_num_iterations=8)
    # a scene with as many unknowns as observations is fitted EXACTLY: its costs fall to rounding noise (1e-14 .. 1e-21 of the start),
    # where neither the trajectories nor two evaluations of one state agree to any digit — compared only while the cost is a number
    out.update(initial_cost=float(Sb.initial_cost), final_cost=float(Sb.final_cost))
    floor = 1e-9 * Sb.initial_cost
    diverged = None
    for i in range(min(Sa.num_iterations_logged, Sb.num_iterations_logged)):
        a, b = Sa.iterations[i], Sb.iterations[i]
        if min(a.cost, b.cost) <= floor:
            break
        if max(a.linear_solver_iterations, b.linear_solver_iterations) > 15:
            # dozens of CG iterations on a system whose column norms span ten orders of magnitude: the last bits of the LDS sums
            # (whose order varies from run to run) reach the third digit of the step — the product does not even repeat ITSELF there
            # (seed 57: 13.0821 in one run, 13.0794 in the next; the oracle 13.0793).  Nothing to compare from here on.
            diverged = i
            break
        assert abs(a.linear_solver_iterations - b.linear_solver_iterations) <= 1, i
        if a.linear_solver_iterations != b.linear_solver_iterations:
            # inexact Newton (eta = 0.1): the two CG solves left the same sequence one index apart (a tie on zeta) — both steps are
            # valid, the iterates differ by one CG update from here on and the trajectories part company; nothing further to compare
            diverged = i
            break
        assert a.step_is_successful == b.step_is_successful and a.step_is_valid == b.step_is_valid, i
        # the cost of a REJECTED candidate is a sample of the non-linear cost far from the linearisation point, at the end of twenty or
        # thirty CG iterations on a system whose column norms span 1e-4 .. 1e5: the two candidates agree to 1e-3 there and the
        # costs follow (profiles/r06zf: 151 794 against 150 927 for a step that is rejected either way; the accepted iterates before
        # and after agree to 1e-11).  Accepted steps: 1e-6, as in tests/test_gpu_bal_frontend.py.
        if a.step_is_successful:
            assert abs(a.cost - b.cost) <= 1e-6 * max(abs(a.cost), 1e-4 * Sb.initial_cost), (i, a.cost, b.cost)   # (near-exact fits: relative to the start)
            assert abs(a.radius - b.trust_region_radius) <= 1e-6 * a.radius, i
    out["compared_until"] = diverged
    if Sb.final_cost > floor and diverged is None:
        assert Sb.termination_type == Sa.termination, (Sb.termination_type, Sa.termination)
    if Sb.final_cost > floor:
        worst["final_cost_vs_evaluate"] = abs(gp.evaluate(x)[0] - Sb.final_cost) / Sb.final_cost
    gp.close()
    bad = {a: b for a, b in worst.items() if not (b <= 1e-10)}
    return dict(out, ok=not bad, worst=max(worst.values()), worst_key=max(worst, key=worst.get), bad=bad, iterations=int(Sb.num_iterations_logged),
                seconds=round(time.time() - t0, 2))


def run_variant(seed):
    import test_gpu_frontend_matrix as M
    rng = np.random.default_rng(700001 * seed + 3)
    while True:
        case = tuple(levels[int(rng.integers(len(levels)))] for _, levels in M.FACTORS)
        if M.allowed(case):
            break
    shape = dict(npts=int(rng.choice([90, 120, 160, 200])), track=int(rng.integers(5, 11)))
    t0 = time.time()
    sc = None
    for k in range(5):   # (a draw that leaves a camera without observations: the next scene seed)
        try:
            sc = M.edge_scene(oracle, seed=seed * 10 + k + 1, **shape)
            break
        except AssertionError:
            continue
    if sc is None:
        return dict(seed=seed, case=M.case_id(case), **shape, ok=False, error="no edge scene in five draws")
    loop_sc = M.clean_scene(oracle, seed=seed + 1)
    c = dict(zip(M.NAMES, case))
    for name, v in (("CERES_HIP_EVAL_TILES", c["tiles"]), ("CERES_HIP_INNER_FORM", c["inner_form"])):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = v
    dev = M.compare(hip, oracle, sc, loop_sc, case, conditioning=True)
    lim = M.limits(case, conditioning=dev["edge_conditioning"])
    bad = M.exceeded(dev, lim)
    return dict(seed=seed, case=M.case_id(case), nobs=int(sc[2].shape[0]), **shape, ok=not bad, bad=bad,
                dev={k: (float(v) if isinstance(v, (int, float, np.floating)) else v) for k, v in dev.items()},
                seconds=round(time.time() - t0, 2))


def run_masked(seed):
    import test_gpu_constant_blocks as T
    import test_gpu_frontend_matrix as M
    rng = np.random.default_rng(500009 * seed + 7)
    while True:
        case = tuple(levels[int(rng.integers(len(levels)))] for _, levels in M.FACTORS)
        if M.allowed(case):
            break
    shape = dict(npts=int(rng.choice([90, 120, 160, 200])), track=int(rng.integers(5, 11)))
    t0 = time.time()
    sc = None
    for k in range(5):
        try:
            sc = M.edge_scene(oracle, seed=seed * 10 + k + 1, **shape)
            break
        except AssertionError:
            continue
    if sc is None:
        return dict(seed=seed, case=M.case_id(case), **shape, ok=False, error="no edge scene in five draws")
    loop_sc = M.clean_scene(oracle, seed=seed + 1)
    c = dict(zip(M.NAMES, case))
    for name, v in (("CERES_HIP_EVAL_TILES", c["tiles"]), ("CERES_HIP_INNER_FORM", c["inner_form"])):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = v
    p_cam, p_pt = float(rng.choice([0.0, 0.05, 0.3])), float(rng.choice([0.0, 0.02, 0.3]))
    dev, drawn = {}, {}
    for key, scene, loop in (("edge", sc, False), ("clean", loop_sc, True)):
        cc = np.flatnonzero(rng.random(scene[0]) < p_cam)[:scene[0] - 1]   # (at least one camera and one point stay free)
        cp = np.flatnonzero(rng.random(scene[1]) < p_pt)[:scene[1] - 1]
        if rng.random() < 0.3:
            cc = np.union1d(cc, [0])
        drawn[key] = [int(cc.size), int(cp.size)]
        dev.update(T.one_side(hip, oracle, scene, ((cc.tolist(), cp.tolist()), case), loop=loop))
    lim = {k: v for k, v in T.cb_limits(("none", case)).items() if not k.startswith("edge_")}
    bad = M.exceeded(dev, lim)
    return dict(seed=seed, case=M.case_id(case), constant=drawn, **shape, ok=not bad, bad=bad,
                dev={k: (float(v) if isinstance(v, (int, float, np.floating)) else v) for k, v in dev.items()}, seconds=round(time.time() - t0, 2))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    first = int(args[0]) if args else 0
    count = int(args[1]) if len(args) > 1 else 40
    masks = "--masks" in sys.argv
    variants = "--variants" in sys.argv or masks
    failed = 0
    worst = {}
    for seed in range(first, first + count):
        try:
            r = run_masked(seed) if masks else run_variant(seed) if variants else run_case(seed)
            for k, v in r.get("dev", {}).items():
                if isinstance(v, float) and not (worst.get(k, (-1.0,))[0] >= v):
                    worst[k] = (v, r["case"])
        except Exception as ex:
            r = dict(seed=seed, ok=False, error=repr(ex)[:600], trace=traceback.format_exc()[-1000:])
        failed += 0 if r["ok"] else 1
        print(json.dumps(r), flush=True)
    print(json.dumps({"cases": count, "failed": failed, **({"worst": worst} if variants else {})}), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
