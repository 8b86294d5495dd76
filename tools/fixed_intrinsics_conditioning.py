"""How well conditioned the cases of tests/test_gpu_fixed_intrinsics.py are: the restatement's own 8-iteration trajectory under
jacobian_noise=(1e-14, seed), seeds 1 and 2 (the method of test_gpu_frontend_matrix.EDGE_ILL_CONDITIONED; as
tools/constant_blocks_conditioning.py).  No GPU.  Prints
  - the base table of design/22_fixed_intrinsics.md: scene x intrinsics mask x {LM, traditional dogleg}, the larger of the squared
    loss and Huber(2), with the free-intrinsics scene beside it;
  - one line per table case on the edge scene (and, with --clean, on the clean scene, where no case may be excused);
  - the entries of that file's EDGE_ILL_CONDITIONED: the cases whose largest relative cost deviation exceeds a hundredth of their cost
    tolerance.

    python tools/fixed_intrinsics_conditioning.py [--clean] [--no-base] [substring of the case ids to run]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__ as entry  # noqa: E402
import fixed_intrinsics_reference as FI  # noqa: E402
import frontend_reference as F  # noqa: E402
import test_gpu_fixed_intrinsics as T  # noqa: E402
from test_gpu_frontend_matrix import NAMES, clean_scene, edge_scene, tolerances  # noqa: E402

HUBER = ("huber", 2.0, 1.0, 1.0)


def state(sc):
    nc = sc[0]
    return np.concatenate([sc[-1][9 * nc:], sc[-1][:9 * nc]])


def base_table(oracle, scenes):
    for name, sc in scenes.items():
        nc, npts, cam, pt, obs, _ = sc
        order = np.argsort(pt, kind="stable")
        for mask in (None,) + T.MASKS:
            for strategy in ("lm", "traditional"):
                worst = 0.0
                for loss in (None, HUBER):
                    w = FI.Problem(F.problem(oracle.snavely_batch, 0, nc, npts, cam, pt, obs, order, loss), nc, npts, mask)
                    worst = max(worst, FI.conditioning(w, state(sc), strategy)[0])
                print(f"base {name} {{{mask or 'free'}}} {strategy}: {worst:.1e}", flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only = args[0] if args else ""
    oracle = entry.load_oracle()
    scenes = {"clean": clean_scene(oracle), "edge": edge_scene(oracle)}
    if "--no-base" not in sys.argv:
        base_table(oracle, scenes)
    out = {}
    for name in (("clean", "edge") if "--clean" in sys.argv else ("edge",)):
        sc = scenes[name]
        for e in T.TABLE:
            if only not in T.fi_id(e):
                continue
            mask, constant, case = e
            c = dict(zip(NAMES, case))
            w = T.Reference(oracle, sc, mask, constant, T.loss_of(c))
            worst, flags = FI.conditioning(w, state(sc), c["strategy"], jacobi_scaling=c["jacobi"])
            excluded = 100.0 * worst > tolerances(case)[0]
            print(f"{name} {T.fi_id(e)}: {worst:.1e} flags_changed={flags}{'  EXCLUDED' if excluded else ''}", flush=True)
            if excluded and name == "edge":
                out[T.fi_id(e)] = worst
            assert not (excluded and name == "clean"), "no case is excused on the clean scene"
    print("EDGE_ILL_CONDITIONED = {")
    for k, v in sorted(out.items(), key=lambda kv: -kv[1]):
        print(f'    "{k}": {v:.1e},')
    print("}")


if __name__ == "__main__":
    main()
