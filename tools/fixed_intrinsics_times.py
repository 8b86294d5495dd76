#!/usr/bin/env python3
"""What fixed camera intrinsics cost and buy in the trust-region loop on one MI355X (design/22_fixed_intrinsics.md).

usage: fixed_intrinsics_times.py [--workload venice1778] [--rounds 5] [--iterations 3] [--parent-library PATH [--parent-last]] [--configs free,fixed] [--out FILE]
       fixed_intrinsics_times.py --single CONFIG [--iterations 3]      (one configuration alone in this process: the thing to wrap in
                                                                        rocprofv3 --kernel-trace --stats)

Timed as tools/constant_blocks_times.py does, on its scene: ceres_hip_bal_minimize, ITERATIVE_SCHUR + SCHUR_JACOBI, ms per LM iteration
= Summary total seconds / iterations; ms per CG iteration = linear solver seconds / CG iterations (one S x pass and its vector kernels).
Two resident worker processes — this tree's library and (with --parent-library) the parent commit's — run their configurations
ALTERNATING, `--rounds` times, one at a time: median, spread = (max - min) / median.

  free_parent   the parent commit's library through ceres_hip_bal_create (the tile-order evaluator)
  free          this tree, the same                                          — expected equal to free_parent, inside the spread
  free_rows     this tree, free intrinsics, CERES_HIP_EVAL_TILES=0: the row-order evaluator a handle with fixed intrinsics runs
  fixed         this tree, {f, k1, k2} fixed: <2,3,6>
  *_cg5         the same with exactly five CG iterations per solve (min = max = 5): fixing intrinsics changes how many iterations CG
                takes to eta, which is the problem's conditioning and not the kernels'; these do equal work per solve"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("free", "free_rows", "fixed", "free_cg5", "free_rows_cg5", "fixed_cg5")


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
    nc, npt, cam, pt, obs, par = scene
    cg5 = config.endswith("_cg5")
    config = config[:-4] if cg5 else config
    o = hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, min_num_iterations=5 if cg5 else 0,
                               max_num_iterations=5 if cg5 else 500)
    kw = {"constant_intrinsics": ["f", "k1", "k2"]} if config == "fixed" else {}
    bp = hs.BalProblem(o, nc, npt, cam, pt, obs, **kw)
    return bp, bp.state_from_bal(par), ("0" if config == "free_rows" else None)


def timed(bp, x0, tiles, iterations):
    if tiles is None:
        os.environ.pop("CERES_HIP_EVAL_TILES", None)
    else:
        os.environ["CERES_HIP_EVAL_TILES"] = tiles   # (read by every ceres_hip_bal_minimize call)
    t0 = time.perf_counter()
    _, S = bp.minimize(x0, max_num_iterations=iterations)
    wall = time.perf_counter() - t0
    os.environ.pop("CERES_HIP_EVAL_TILES", None)
    nit = S.num_successful_steps + S.num_unsuccessful_steps
    cg = [S.iterations[i].linear_solver_iterations for i in range(1, S.num_iterations_logged)]
    return {"ms_per_lm_iteration": 1e3 * S.total_seconds / max(nit, 1), "lm_iterations": nit, "wall_ms": 1e3 * wall,
            "linear_solver_ms": 1e3 * S.linear_solver_seconds, "evaluation_ms": 1e3 * S.evaluation_seconds, "cg_iterations": cg,
            "ms_per_cg_iteration": 1e3 * S.linear_solver_seconds / max(sum(cg), 1), "final_cost": S.final_cost}


def worker(workload):
    pkg, hs = load()
    scene = pkg.problems.bal_scene(workload, seed=38401)
    handles = {}
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd["cmd"] == "quit":
            break
        if cmd["cmd"] == "create":
            bp, x0, tiles = make(pkg, hs, scene, cmd["config"])
            timed(bp, x0, tiles, 1)
            handles[cmd["name"]] = (bp, x0, tiles)
            info = bp.solver_info()
            out = {"kernel_path": int(info.kernel_path), "f_block_size": int(info.f_block_size), "num_jacobian_values": int(bp.num_jacobian_values),
                   "num_effective_parameters": int(bp.num_effective_parameters)}
        elif cmd["cmd"] == "time":
            out = timed(*handles[cmd["name"]], cmd["iterations"])
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
    ap.add_argument("--parent-last", action="store_true", help="time the parent library after this tree's configurations in every round (default: before)")
    ap.add_argument("--configs", default=",".join(CONFIGS), help="this tree's configurations to time ('free' alone: two workers with one handle each)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--single", default=None, choices=CONFIGS)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.workload)
    if a.single:
        pkg, hs = load()
        bp, x0, tiles = make(pkg, hs, pkg.problems.bal_scene(a.workload, seed=38401), a.single)
        timed(bp, x0, tiles, 1)
        for _ in range(3):
            print(json.dumps(timed(bp, x0, tiles, a.iterations)), flush=True)
        bp.close()
        return 0
    workers = {"tree": Worker(a.workload)}
    configs = [("tree", c, c) for c in a.configs.split(",")]
    if a.parent_library:
        workers["parent"] = Worker(a.workload, a.parent_library)
        configs.insert(len(configs) if a.parent_last else 0, ("parent", "free_parent", "free"))
    result = {"workload": a.workload, "rounds": a.rounds, "iterations_per_call": a.iterations, "configs": {}}
    try:
        for w, name, config in configs:
            result["configs"][name] = {"setup": workers[w].call(cmd="create", name=name, config=config)}
        samples = {name: {"ms_per_lm_iteration": [], "ms_per_cg_iteration": []} for _, name, _ in configs}
        for _ in range(a.rounds):   # alternating: one configuration at a time, round after round
            for w, name, _ in configs:
                r = workers[w].call(cmd="time", name=name, iterations=a.iterations)
                for k in samples[name]:
                    samples[name][k].append(r[k])
                result["configs"][name]["last"] = r
        for name, per in samples.items():
            for k, v in per.items():
                result["configs"][name][k] = {"median": round(median(v), 4), "spread": round((max(v) - min(v)) / median(v), 4),
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
