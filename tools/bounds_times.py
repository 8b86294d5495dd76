#!/usr/bin/env python3
"""What bound constraints cost in the trust-region loop on one MI355X, and that the unbounded path did not move (design/23_bounds.md).

usage: bounds_times.py [--workload venice1778] [--rounds 5] [--iterations 3] [--parent-library PATH] [--out FILE]
       bounds_times.py --single CONFIG [--iterations 3]     (one configuration alone in this process: the thing to wrap in
                                                             rocprofv3 --kernel-trace --stats)

Timed as tools/fixed_intrinsics_times.py does, on its scene: ceres_hip_bal_minimize through ceres_hip_bal_create, ITERATIVE_SCHUR +
SCHUR_JACOBI, ms per LM iteration = Summary total seconds / iterations.  Two resident worker processes — this tree's library and (with
--parent-library) the parent commit's — run their configurations ALTERNATING, `--rounds` times, one at a time: median, spread =
(max - min) / median.

  free_parent   the parent commit's library, no bounds
  free          this tree, no bounds                         — expected equal to free_parent, inside the parent's spread
  far           this tree, every camera's f in [0.5 f0, 2 f0]: a constrained handle whose bounds never bind (every search accepts its
                first sample: one gradient evaluation per iteration)
  binding       this tree, every camera's f in [0.9995 f0, 1.0005 f0]: bounds that bind"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("free", "far", "binding")


def load():
    sys.path.insert(0, ROOT)
    import ctypes
    import __graft_entry__ as entry
    pkg = entry.load_package()
    hs = pkg.hip_solver
    probe = ctypes.CDLL(hs.library_path())   # an older build of the library lacks the exports added since: bind what it has
    hs.ABI = [e for e in hs.ABI if hasattr(probe, e[0])]
    hs.load_library()
    return pkg, hs


def make(pkg, hs, scene, config):
    import numpy as np
    nc, npt, cam, pt, obs, par = scene
    o = hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, min_num_iterations=0, max_num_iterations=500)
    bp = hs.BalProblem(o, nc, npt, cam, pt, obs)
    x0 = bp.state_from_bal(par)
    if config != "free":
        lo, hi = np.full(x0.size, -np.inf), np.full(x0.size, np.inf)
        f = 3 * npt + 9 * np.arange(nc) + 6
        a, b = (0.5, 2.0) if config == "far" else (0.9995, 1.0005)
        lo[f], hi[f] = np.minimum(a * x0[f], b * x0[f]), np.maximum(a * x0[f], b * x0[f])
        bp.set_bounds(lo, hi)
    return bp, x0


def timed(bp, x0, iterations, bounded):
    t0 = time.perf_counter()
    _, S = bp.minimize(x0, max_num_iterations=iterations)
    wall = time.perf_counter() - t0
    nit = S.num_successful_steps + S.num_unsuccessful_steps
    out = {"ms_per_lm_iteration": 1e3 * S.total_seconds / max(nit, 1), "lm_iterations": nit, "wall_ms": 1e3 * wall,
           "linear_solver_ms": 1e3 * S.linear_solver_seconds, "evaluation_ms": 1e3 * S.evaluation_seconds, "final_cost": S.final_cost}
    if bounded:
        st = bp.bounds_stats()
        out.update(line_search_ms=1e3 * st["line_search_seconds"], function_evaluations_per_iteration=st["num_function_evaluations"] / max(nit, 1),
                   gradient_evaluations_per_iteration=st["num_gradient_evaluations"] / max(nit, 1), num_projected=st["num_projected"],
                   searches=[int(v) for v in st["line_search_iterations"][:S.num_iterations_logged]])
    return out


def worker(workload):
    pkg, hs = load()
    scene = pkg.problems.bal_scene(workload, seed=38401)
    handles = {}
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd["cmd"] == "quit":
            break
        if cmd["cmd"] == "create":
            bp, x0 = make(pkg, hs, scene, cmd["config"])
            handles[cmd["name"]] = (bp, x0, cmd["config"] != "free")
            out = timed(*handles[cmd["name"]][:2], 1, cmd["config"] != "free")
        elif cmd["cmd"] == "time":
            bp, x0, bounded = handles[cmd["name"]]
            out = timed(bp, x0, cmd["iterations"], bounded)
        print("REPLY " + json.dumps(out), flush=True)
    for bp, _, _ in handles.values():
        bp.close()


class Worker:
    def __init__(self, workload, library=None):
        env = dict(os.environ)
        if library:
            env["CERES_HIP_LIBRARY"] = os.path.abspath(library)
        else:
            env.pop("CERES_HIP_LIBRARY", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--workload", workload], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)

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
    ap.add_argument("--workload", default="venice1778")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--single", default=None, choices=CONFIGS)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.workload)
    if a.single:
        pkg, hs = load()
        bp, x0 = make(pkg, hs, pkg.problems.bal_scene(a.workload, seed=38401), a.single)
        timed(bp, x0, 1, a.single != "free")
        for _ in range(3):
            print(json.dumps(timed(bp, x0, a.iterations, a.single != "free")), flush=True)
        bp.close()
        return 0
    workers = {"tree": Worker(a.workload)}
    configs = [("tree", c, c) for c in a.configs.split(",")]
    if a.parent_library:
        workers["parent"] = Worker(a.workload, a.parent_library)
        configs.insert(0, ("parent", "free_parent", "free"))
    result = {"workload": a.workload, "rounds": a.rounds, "iterations_per_call": a.iterations, "configs": {}}
    try:
        for w, name, config in configs:
            result["configs"][name] = {"setup": workers[w].call(cmd="create", name=name, config=config)}
        samples = {name: [] for _, name, _ in configs}
        for _ in range(a.rounds):   # alternating: one configuration at a time, round after round
            for w, name, _ in configs:
                r = workers[w].call(cmd="time", name=name, iterations=a.iterations)
                samples[name].append(r["ms_per_lm_iteration"])
                result["configs"][name]["last"] = r
        for name, v in samples.items():
            result["configs"][name]["ms_per_lm_iteration"] = {"median": round(median(v), 4), "spread": round((max(v) - min(v)) / median(v), 4),
                                                              "samples": [round(x, 4) for x in v]}
        print(json.dumps(result), flush=True)
    finally:
        for w in workers.values():
            w.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
