#!/usr/bin/env python3
"""How far the device repeats ITSELF on each edge-scene case of tests/test_gpu_fixed_intrinsics.py (GPU box): three fresh handles, the
largest relative difference of any logged cost — the method of test_gpu_frontend_matrix.EDGE_DEVICE_UNREPEATABLE.  Prints one line per
case (with the iterations' accept / reject flags, and the difference over accepted iterations alone) and, at the end, that file's
EDGE_DEVICE_UNREPEATABLE: the cases whose difference exceeds a tenth of their cost tolerance.

    python tools/fixed_intrinsics_repeatability.py [substring of the case ids to run]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__ as entry  # noqa: E402
import test_gpu_fixed_intrinsics as T  # noqa: E402
from test_gpu_frontend_matrix import NAMES, edge_scene, tolerances  # noqa: E402


def main():
    oracle = entry.load_oracle()
    hip = entry.load_package().hip_solver
    hip.load_library()
    sc = edge_scene(oracle)
    only = sys.argv[1] if len(sys.argv) > 1 else ""
    out = {}
    for e in T.TABLE:
        if only not in T.fi_id(e) or not T.edge_values_compared(e):
            continue
        mask, constant, case = e
        c = dict(zip(NAMES, case))
        runs = []
        for _ in range(3):
            gp = T.device_problem(hip, sc, mask, constant, c["solver"], c["generic"])
            try:
                if T.loss_of(c):
                    gp.set_loss(*T.loss_of(c))
                if c["strategy"] != "lm":
                    gp.set_trust_region_strategy("dogleg", c["strategy"])
                _, S = gp.minimize(gp.state_from_bal(sc[-1]), eta=1e-12, max_num_iterations=8, jacobi_scaling=c["jacobi"])
                runs.append([(S.iterations[i].cost, S.iterations[i].step_is_successful) for i in range(S.num_iterations_logged)])
            finally:
                gp.close()
        n = min(len(r) for r in runs)
        diff = [max(r[i][0] for r in runs) / min(r[i][0] for r in runs) - 1.0 for i in range(n)]
        ok = [all(r[i][1] for r in runs) for i in range(n)]
        worst, worst_ok = max(diff), max([d for d, a in zip(diff, ok) if a] or [0.0])
        listed = 10.0 * worst > tolerances(case)[0]
        print(f"{T.fi_id(e)}: {worst:.1e} accepted_only={worst_ok:.1e} flags={''.join('a' if a else 'r' for a in ok)}{'  LISTED' if listed else ''}", flush=True)
        if listed:
            out[T.fi_id(e)] = worst
    print("EDGE_DEVICE_UNREPEATABLE = {")
    for k, v in sorted(out.items(), key=lambda kv: -kv[1]):
        print(f'    "{k}": {v:.1e},')
    print("}")


if __name__ == "__main__":
    main()
