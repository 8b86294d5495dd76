#!/usr/bin/env python3
"""What constant parameter blocks cost in the trust-region loop on one MI355X (design/15_constant_blocks.md).

usage: constant_blocks_times.py [--workload venice1778] [--rounds 5] [--iterations 3] [--parent-library PATH] [--out FILE]
       constant_blocks_times.py --single free|camera0|points1pct [--iterations 3]      (one configuration alone in this process: the
                                                                                        thing to wrap in rocprofv3 --kernel-trace --stats)

Timed as tools/minimize_trace.py does, on the scene it uses: ceres_hip_bal_minimize, ITERATIVE_SCHUR + SCHUR_JACOBI, ms per LM iteration
= Summary total seconds / iterations.  Two resident worker processes, one per library — this tree's and (with --parent-library: a build
of the parent commit, selected through CERES_HIP_LIBRARY) the parent's — run their configurations ALTERNATING, `--rounds` times, one at
a time (the method of tools/cluster_jacobi_times.py): median, spread = (max - min) / median.

  free_parent   the parent commit's library, nothing constant (the old entry point)
  free          this tree, nothing constant, the old entry point            — expected equal to free_parent, accepted inside the spread
  camera0       this tree, camera 0 constant: the same rows, one camera less — accepted if not slower than `free` by more than the
                larger of the two spreads
  points1pct    this tree, every hundredth point constant: remainder rows, the two-pass evaluator — reported, no threshold
  free_cg5, camera0_cg5   the same two with exactly five CG iterations per solve (min = max = 5): fixing the gauge changes how many
                iterations CG takes to eta, which is the problem's conditioning and not the kernels'; these two do equal work

Also, as information: LM iterations and CG iterations to the default function tolerance, free against gauge-fixed (camera0)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("free", "camera0", "points1pct", "free_cg5", "camera0_cg5")


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


def make(pkg, hs, scene, config, generic=False):
    import numpy as np
    nc, npt, cam, pt, obs, par = scene
    cg5 = config.endswith("_cg5")
    config = config[:-4] if cg5 else config
    o = hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, min_num_iterations=5 if cg5 else 0,
                               max_num_iterations=5 if cg5 else 500, force_generic_path=generic)
    kw = {}
    if config == "camera0":
        kw["constant_cameras"] = [0]
    elif config == "points1pct":
        kw["constant_points"] = np.arange(0, npt, 100)
    bp = hs.BalProblem(o, nc, npt, cam, pt, obs, **kw)
    return bp, bp.state_from_bal(par)


def timed(bp, x0, iterations):
    t0 = time.perf_counter()
    _, S = bp.minimize(x0, max_num_iterations=iterations)
    wall = time.perf_counter() - t0
    nit = S.num_successful_steps + S.num_unsuccessful_steps
    return {"ms_per_lm_iteration": 1e3 * S.total_seconds / max(nit, 1), "lm_iterations": nit, "wall_ms": 1e3 * wall,
            "linear_solver_ms": 1e3 * S.linear_solver_seconds, "evaluation_ms": 1e3 * S.evaluation_seconds,
            "cg_iterations": [S.iterations[i].linear_solver_iterations for i in range(1, S.num_iterations_logged)], "final_cost": S.final_cost}


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
            bp.minimize(x0, max_num_iterations=1)
            handles[cmd["name"]] = (bp, x0)
            out = {"kernel_path": int(bp.solver_info().kernel_path)}
            if hasattr(bp, "reduced_sizes") and any(e[0] == "ceres_hip_bal_reduced_sizes" for e in hs.ABI):
                out["reduced_sizes"] = list(bp.reduced_sizes())
        elif cmd["cmd"] == "time":
            out = timed(*handles[cmd["name"]], cmd["iterations"])
        elif cmd["cmd"] == "converge":
            bp, x0 = handles[cmd["name"]]
            _, S = bp.minimize(x0, max_num_iterations=50)
            out = {"lm_iterations": S.num_successful_steps + S.num_unsuccessful_steps, "termination": S.message.decode(errors="replace"),
                   "cg_iterations_total": sum(S.iterations[i].linear_solver_iterations for i in range(1, S.num_iterations_logged)),
                   "initial_cost": S.initial_cost, "final_cost": S.final_cost}
        print("REPLY " + json.dumps(out), flush=True)
    for bp, _ in handles.values():
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--single", default=None, choices=CONFIGS)
    ap.add_argument("--generic", action="store_true", help="--single on the generic kernels (force_generic_path)")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.workload)
    if a.single:
        pkg, hs = load()
        bp, x0 = make(pkg, hs, pkg.problems.bal_scene(a.workload, seed=38401), a.single, generic=a.generic)
        bp.minimize(x0, max_num_iterations=1)
        for _ in range(3):
            print(json.dumps(timed(bp, x0, a.iterations)), flush=True)
        bp.close()
        return 0
    workers = {"tree": Worker(a.workload)}
    configs = [("tree", c, c) for c in CONFIGS]
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
            result["configs"][name].update(ms_per_lm_iteration_median=round(median(v), 4), spread=round((max(v) - min(v)) / median(v), 4),
                                           samples_ms=[round(x, 4) for x in v])
        C = result["configs"]

        def versus(x, y):
            d = C[x]["ms_per_lm_iteration_median"] - C[y]["ms_per_lm_iteration_median"]
            allow = max(C[x]["spread"], C[y]["spread"]) * C[y]["ms_per_lm_iteration_median"]
            return {"against": y, "difference_ms": round(d, 4), "allowance_ms": round(allow, 4), "not_slower_beyond_spread": bool(d <= allow),
                    "within_spread": bool(abs(d) <= allow)}
        if a.parent_library:
            C["free"]["versus"] = versus("free", "free_parent")
        C["camera0"]["versus"] = versus("camera0", "free")
        C["points1pct"]["versus"] = versus("points1pct", "free")
        C["camera0_cg5"]["versus"] = versus("camera0_cg5", "free_cg5")
        for name in ("free", "camera0"):
            C[name]["to_function_tolerance"] = workers["tree"].call(cmd="converge", name=name)
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
