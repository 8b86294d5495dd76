#!/usr/bin/env python3
"""What CLUSTER_JACOBI costs and buys on one MI355X, next to SCHUR_JACOBI (design/14_cluster_jacobi.md).

usage: cluster_jacobi_times.py [--scenes conditioned,venice] [--workload venice1778] [--rounds 5] [--steps 5]
                               [--parent-library PATH] [--out FILE]

Scenes: "conditioned" = bench.py's conditioned_step leg (the Snavely Jacobian of a sequence-like scene from the device evaluator, LM
steps at eta 1e-2 / 1e-3 / 1e-4, radius 1e4); "venice" = the default workload of bench.py (random visibility, N(0,1) values, eta 0.1).

Two resident worker processes, one per library — this tree's, and (with --parent-library: a build of the parent commit, e.g. by
tools/build_variant.sh in a checkout of it, selected through CERES_HIP_LIBRARY) the parent's — hold the same scene and run their
configurations ALTERNATING, `--rounds` times, only one at a time: the boxes of the pool differ by several per cent and drift, so both
sides of every comparison are measured on the same machine in the same visit.  Per configuration: the median ms per whole LM step
(ceres_hip_lm_compute_step_device, inputs resident in HBM), its spread (max - min) / median over the rounds, and the CG iterations.
The parent's SCHUR_JACOBI must equal this tree's within that spread: the existing path did not move.
For CLUSTER_JACOBI also: host set-up seconds (clustering + pair lists), clusters and the largest dimension, and — the method of
tools/kernel_times.py, ceres_hip_time_op — microseconds of the elimination, assemble + factor, one application, next to one S.x."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS = 1e4


def worker():
    sys.path.insert(0, ROOT)
    import ctypes
    import numpy as np
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    hs = pkg.hip_solver
    probe = ctypes.CDLL(hs.library_path())   # an older build of the library lacks the exports added since: bind what it has
    hs.ABI = [e for e in hs.ABI if hasattr(probe, e[0])]
    hs.load_library()
    P = pkg.problems
    dev = torch.device("cuda:0")
    state = {}

    def reply(obj):
        print("REPLY " + json.dumps(obj), flush=True)

    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd["cmd"] == "quit":
            break
        if cmd["cmd"] == "scene":
            kind, wl, d = cmd["kind"], cmd["workload"], cmd["dir"]
            for s in state.get("solvers", {}).values():
                s.close()
            state.clear()
            if kind == "conditioned":
                prob = P.banded_bal(wl, seed=38401, with_values=False)
                fv, fr = os.path.join(d, "cond_values.npy"), os.path.join(d, "cond_residuals.npy")
                if not os.path.exists(fv):   # the Snavely Jacobian and residuals of the scene, from the device evaluator (as bench.py)
                    nc, npts, cam, pt, obs, par = P.bal_scene(wl, seed=38401, visibility="banded")
                    bp = hs.BalProblem(hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, min_num_iterations=0,
                                                              max_num_iterations=500), nc, npts, cam, pt, obs)
                    _, res, _, vals = bp.evaluate(bp.state_from_bal(par), residuals=True, jacobian=True)
                    bp.close()
                    np.save(fv, vals)
                    np.save(fr, res)
                vals, res = np.load(fv), np.load(fr)
            else:
                prob = P.synthetic_bal(wl, layout="schur", seed=38401, skew=0.6)
                vals, res = prob.values, prob.b
            state["prob"] = prob
            state["tv"], state["tb"] = torch.from_numpy(np.ascontiguousarray(vals)).to(dev), torch.from_numpy(np.ascontiguousarray(res)).to(dev)
            state["tx"] = torch.empty(prob.bs.num_cols, dtype=torch.float64, device=dev)
            state["solvers"] = {}
            torch.cuda.synchronize()
            reply({"ok": 1, "cameras": int(prob.bs.num_col_blocks - prob.num_eliminate_blocks), "points": int(prob.num_eliminate_blocks),
                   "observations": int(prob.bs.num_row_blocks)})
        elif cmd["cmd"] == "create":
            prob = state["prob"]
            kw = {}
            if cmd["pre"] == 4:
                kw["visibility_clustering_type"] = cmd["clustering"]
            o = hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=cmd["pre"], min_num_iterations=0, max_num_iterations=500,
                                       elimination_groups=[prob.num_eliminate_blocks], **kw)
            t0 = time.perf_counter()
            s = hs.HipLinearSolver(o)
            s.set_structure(prob.bs)
            out = {"set_structure_s": round(time.perf_counter() - t0, 3), "device_bytes": int(s.info().device_bytes)}
            if cmd["pre"] == 4:
                n, largest, nbytes, secs = s.cluster_jacobi_stats()
                out.update(num_clusters=n, largest_dimension=largest, factor_bytes=nbytes, host_setup_s=round(secs, 3))
            state["solvers"][cmd["name"]] = s
            reply(out)
        elif cmd["cmd"] == "time":
            s = state["solvers"][cmd["name"]]
            tv, tb, tx = state["tv"], state["tb"], state["tx"]
            its = []
            for _ in range(cmd.get("warmup", 1)):
                s.lm_compute_step_device(tv.data_ptr(), tb.data_ptr(), tx.data_ptr(), RADIUS, cmd["eta"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(cmd["steps"]):
                summ, mcc, finite = s.lm_compute_step_device(tv.data_ptr(), tb.data_ptr(), tx.data_ptr(), RADIUS, cmd["eta"])
                its.append(int(summ.num_iterations))
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            reply({"ms_per_step": 1e3 * el / cmd["steps"], "cg_iterations": its[-1], "termination": int(summ.termination_type),
                   "finite": bool(finite), "model_cost_change_positive": bool(mcc > 0)})
        elif cmd["cmd"] == "ops":
            s = state["solvers"][cmd["name"]]
            s.lm_compute_step_device(state["tv"].data_ptr(), state["tb"].data_ptr(), state["tx"].data_ptr(), RADIUS, 0.1)   # loads values and D
            out = {"sx_us": round(1e3 * min(s.time_op(hs.TIMED_SX, 20) for _ in range(3)), 2)}
            if cmd.get("cluster"):
                for key, op, n in (("eliminate_us", hs.TIMED_CLUSTER_ELIMINATE, 10), ("assemble_factor_us", hs.TIMED_CLUSTER_FACTOR, 10),
                                   ("apply_us", hs.TIMED_CLUSTER_APPLY, 20)):
                    out[key] = round(1e3 * min(s.time_op(op, n) for _ in range(3)), 2)
            else:
                out["schur_jacobi_update_us"] = round(1e3 * min(s.time_op(hs.TIMED_SCHUR_JACOBI, 20) for _ in range(3)), 2)
            reply(out)
    for s in state.get("solvers", {}).values():
        s.close()


class Worker:
    def __init__(self, library=None):
        env = dict(os.environ)
        if library:
            env["CERES_HIP_LIBRARY"] = os.path.abspath(library)
        else:
            env.pop("CERES_HIP_LIBRARY", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True, env=env, cwd=ROOT)

    def call(self, **cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"worker ended (exit {self.p.poll()}) during {cmd}")
            if line.startswith("REPLY "):
                return json.loads(line[6:])

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"cmd": "quit"}) + "\n")
            self.p.stdin.flush()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="conditioned,venice")
    ap.add_argument("--workload", default="venice1778")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker()
    workers = {"tree": Worker()}
    if a.parent_library:
        workers["parent"] = Worker(a.parent_library)
    # (worker, name, preconditioner, clustering)
    configs = [("tree", "schur_jacobi", 2, 0), ("tree", "cluster_jacobi_canonical_views", 4, 0), ("tree", "cluster_jacobi_single_linkage", 4, 1)]
    if a.parent_library:
        configs.insert(0, ("parent", "schur_jacobi_parent_commit", 2, 0))
    result = {"workload": a.workload, "rounds": a.rounds, "steps_per_round": a.steps, "radius": RADIUS, "scenes": {}}
    tmp = tempfile.mkdtemp(prefix="cluster_jacobi_times_")
    try:
        for scene in a.scenes.split(","):
            etas = (1e-2, 1e-3, 1e-4) if scene == "conditioned" else (0.1,)
            out = {"etas": list(etas), "configs": {}}
            for w in ("tree", "parent"):   # the tree's worker first: it evaluates the scene, the other one loads it
                if w in workers:
                    out["problem"] = workers[w].call(cmd="scene", kind=scene, workload=a.workload, dir=tmp)
            for w, name, pre, clustering in configs:
                out["configs"][name] = {"setup": workers[w].call(cmd="create", name=name, pre=pre, clustering=clustering)}
            for w, name, pre, clustering in configs:
                out["configs"][name]["operators"] = workers[w].call(cmd="ops", name=name, cluster=(pre == 4))
            for eta in etas:
                samples = {name: [] for _, name, _, _ in configs}
                its = {}
                for _ in range(a.rounds):   # alternating: one configuration at a time, round after round
                    for w, name, pre, clustering in configs:
                        r = workers[w].call(cmd="time", name=name, eta=eta, steps=a.steps)
                        samples[name].append(r["ms_per_step"])
                        its[name] = r["cg_iterations"]
                for name, v in samples.items():
                    out["configs"][name][f"eta_{eta:g}"] = {"ms_per_step_median": round(median(v), 4), "spread": round((max(v) - min(v)) / median(v), 4),
                                                           "cg_iterations": its[name], "samples_ms": [round(x, 4) for x in v]}
                if a.parent_library:
                    p, t = out["configs"]["schur_jacobi_parent_commit"][f"eta_{eta:g}"], out["configs"]["schur_jacobi"][f"eta_{eta:g}"]
                    out["configs"]["schur_jacobi"][f"eta_{eta:g}"]["vs_parent_commit"] = {
                        "relative_difference": round((t["ms_per_step_median"] - p["ms_per_step_median"]) / p["ms_per_step_median"], 4),
                        "within_spread": bool(abs(t["ms_per_step_median"] - p["ms_per_step_median"]) <= max(p["spread"], t["spread"]) * p["ms_per_step_median"])}
            result["scenes"][scene] = out
            print(json.dumps({scene: out}), flush=True)
    finally:
        for w in workers.values():
            w.close()
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
