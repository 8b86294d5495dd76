"""How well conditioned each case of tests/test_gpu_constant_blocks.py is on the edge scene: the restatement's own 8-iteration
trajectory under jacobian_noise=(1e-14, seed), seeds 1 and 2 (the method of test_gpu_frontend_matrix.EDGE_ILL_CONDITIONED).  No GPU.
Prints one line per case and, at the end, the entries of that file's EDGE_ILL_CONDITIONED: the cases whose largest relative cost
deviation exceeds a hundredth of their cost tolerance.

    python tools/constant_blocks_conditioning.py [substring of the case ids to run]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__ as entry  # noqa: E402
import frontend_reference as F  # noqa: E402
import test_gpu_constant_blocks as T  # noqa: E402
from test_gpu_frontend_matrix import NAMES, edge_scene, tolerances  # noqa: E402


def main():
    oracle = entry.load_oracle()
    hs = entry.load_package().hip_solver
    sc = edge_scene(oracle)
    nc, npts = sc[0], sc[1]
    only = sys.argv[1] if len(sys.argv) > 1 else ""
    out = {}
    for e in T.TABLE:
        if only not in T.cb_id(e):
            continue
        masks, case = e
        c = dict(zip(NAMES, case))
        w = T.reference(oracle, sc, masks, c["camera"], T.loss_of(c))
        par = sc[-1]
        cams, pts = par[:9 * nc], par[9 * nc:]
        if c["camera"] != "angle_axis":
            import numpy as np
            c9 = cams.reshape(-1, 9)
            cams = np.concatenate([hs.angle_axis_to_quaternion(c9[:, :3]), c9[:, 3:]], axis=1).reshape(-1)
        import numpy as np
        x0 = np.concatenate([pts, cams])
        inner = w.inner_ordering(c["inner"]) if c["inner"] else None
        opts = dict(max_num_iterations=8, jacobi_scaling=c["jacobi"])
        _, Sr = F.minimize(w, x0, c["strategy"], inner=inner, **opts)
        worst, flags = 0.0, 0
        for seed in (1, 2):
            _, Sn = F.minimize(w, x0, c["strategy"], inner=inner, jacobian_noise=(1e-14, seed), **opts)
            worst = max([worst] + [abs(a["cost"] - b["cost"]) / b["cost"] for a, b in zip(Sn["iterations"], Sr["iterations"])])
            flags += sum((a["step_is_successful"], a["step_is_valid"]) != (b["step_is_successful"], b["step_is_valid"])
                         for a, b in zip(Sn["iterations"], Sr["iterations"])) + abs(len(Sn["iterations"]) - len(Sr["iterations"]))
        excluded = 100.0 * worst > tolerances(case)[0]
        print(f"{T.cb_id(e)}: {worst:.1e} flags_changed={flags}{'  EXCLUDED' if excluded else ''}", flush=True)
        if excluded:
            out[T.cb_id(e)] = worst
    print("EDGE_ILL_CONDITIONED = {")
    for k, v in sorted(out.items(), key=lambda kv: -kv[1]):
        print(f'    "{k}": {v:.1e},')
    print("}")


if __name__ == "__main__":
    main()
