#!/usr/bin/env python3
"""What shared camera intrinsics cost and buy in the trust-region loop on one MI355X (design/27_shared_intrinsics.md).

usage: shared_intrinsics_times.py [--workload venice1778] [--rounds 5] [--iterations 3] [--parent-library PATH [--parent-last]] [--configs ...] [--out FILE]
       shared_intrinsics_times.py --single CONFIG [--iterations 3]      (one configuration alone: the thing to wrap in rocprofv3
                                                                         --kernel-trace --stats)

tools/fixed_intrinsics_times.py with two more configurations — its method, its scene, its workers and its output:

  free, fixed, *_cg5   as there (the default handle with the tile-order evaluator; {f, k1, k2} fixed: <2,3,6>)
  shared               ONE group: every camera on one [f, k1, k2] block, <2,3,6> + the 4-scalar strip, the row-order evaluator of
                       csrc/kernels_shared.hip; the state's intrinsics are camera 0's in every camera (the pixels stay as generated:
                       what is timed is the work per iteration, not the trajectory)
  shared_cg5           the same with exactly five CG iterations per solve"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixed_intrinsics_times as T   # noqa: E402

CONFIGS = ("free", "fixed", "shared", "free_cg5", "fixed_cg5", "shared_cg5")
_make = T.make


def make(pkg, hs, scene, config):
    base = config[:-4] if config.endswith("_cg5") else config
    if base != "shared":
        return _make(pkg, hs, scene, config)
    import numpy as np
    nc, npt, cam, pt, obs, par = scene
    cg5 = config.endswith("_cg5")
    o = hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, min_num_iterations=5 if cg5 else 0,
                               max_num_iterations=5 if cg5 else 500)
    bp = hs.BalProblem(o, nc, npt, cam, pt, obs, camera_groups=np.zeros(nc, np.int32))
    x0 = bp.state_from_bal(par).copy()
    cams = x0[3 * npt:].reshape(nc, 9)
    cams[:, 6:] = cams[0, 6:]
    return bp, x0, None


class Worker(T.Worker):
    def __init__(self, workload, library=None):
        env = dict(os.environ)
        if library:
            env["CERES_HIP_LIBRARY"] = os.path.abspath(library)
        else:
            env.pop("CERES_HIP_LIBRARY", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--workload", workload], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, env=env, cwd=T.ROOT)


T.CONFIGS, T.make, T.Worker = CONFIGS, make, Worker

if __name__ == "__main__":
    sys.exit(T.main())
