"""Stage times of ceres_hip_bal_covariance on one MI355X (design/17_covariance.md §17.5): a DENSE_SCHUR scene whose free cameras span
n = 8190 columns (912 cameras, two of them constant: the gauge), the median of 5 calls after 2 warm-up calls of the summary's five
stage times, with device_bytes and the pivots.  One JSON line.

--groups G (design/28_shared_covariance.md): the same cameras, points and observations on a handle with shared intrinsics, camera c in
group c % G, the poses of cameras 0 and 1 constant (n = 6 x 910 + 3 G), the state's intrinsics shared within each group.  The pair list
has the free handle's length; a quarter of its pose-pose cross pairs become pose-group pairs (the first G of them the groups' own
blocks), a quarter of its point-pose pairs point-group pairs and a quarter of its points' own blocks point-point pairs p != q — with one
group two such points meet through the group whether or not a camera sees both.

    python tools/covariance_times.py [--cameras 912] [--points 20000] [--observations 120000] [--calls 5] [--warmup 2] [--groups 0]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=912)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--observations", type=int, default=120000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--groups", type=int, default=0)
    a = ap.parse_args()
    pkg = entry.load_package()
    oracle = entry.load_oracle()
    hs = pkg.hip_solver
    op = oracle.BalProblem.generate(a.cameras, a.points, a.observations, seed=a.seed)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    x = op.state()
    o = hs.LinearSolverOptions(type=hs.DENSE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, max_num_iterations=1)
    groups = np.arange(a.cameras, dtype=np.int32) % a.groups if a.groups else None
    if a.groups:   # (the intrinsics of a group are those of its first camera, bit for bit)
        cams = x[3 * a.points:].reshape(a.cameras, 9)
        cams[:, 6:] = cams[groups, 6:]
    gp = hs.BalProblem(o, a.cameras, a.points, cam.astype(np.int32), pt.astype(np.int32), obs, constant_cameras=[0, 1], camera_groups=groups)
    # every camera's own block, its neighbour's cross block, and the own blocks and one cross block of a thousand points
    C = lambda c: a.points + c
    pairs = [(C(c), C(c)) for c in range(a.cameras)] + [(C(c), C(c + 1)) for c in range(a.cameras - 1)]
    pairs += [(q, q) for q in range(0, a.points, max(1, a.points // 1000))] + [(q, C(int(cam[np.flatnonzero(pt == q)[0]]))) for q in range(0, a.points, max(1, a.points // 1000))]
    if a.groups:
        G = lambda g: a.points + a.cameras + g
        step = max(1, a.points // 1000)
        for i, (p, q) in enumerate(pairs):
            if i % 4:
                continue
            if p >= a.points and q == p + 1:      # pose - next pose -> the groups' own blocks, then pose - group
                k = (i - a.cameras) // 4
                pairs[i] = (G(k), G(k)) if k < a.groups else (p, G(int(groups[p - a.points])))
            elif p < a.points and q >= a.points:  # point - pose -> point - group
                pairs[i] = (p, G(int(groups[q - a.points])))
            elif p < a.points and p == q:         # a point's own block -> point - point
                pairs[i] = (p, (p + step) % a.points)
    stages = ("evaluate_seconds", "eliminate_seconds", "factor_seconds", "inverse_seconds", "blocks_seconds")
    rows = []
    S = None
    for i in range(a.warmup + a.calls):
        _, S = gp.covariance(x, pairs)
        if i >= a.warmup:
            rows.append([getattr(S, f) for f in stages])
    med = np.median(np.array(rows), axis=0)
    n = 6 * (a.cameras - 2) + 3 * a.groups if a.groups else 9 * (a.cameras - 2)
    out = {"cameras": a.cameras, "constant_cameras": 2, "n": n, "points": a.points, "observations": int(cam.shape[0]), "pairs": len(pairs),
           "calls": a.calls, "warmup": a.warmup}
    if a.groups:
        kind = lambda b: "point" if b < a.points else "pose" if b < a.points + a.cameras else "group"
        out["groups"] = a.groups
        out["pair_kinds"] = {k: sum(1 for p, q in pairs if kind(p) + "-" + kind(q) == k) for k in sorted({kind(p) + "-" + kind(q) for p, q in pairs})}
    out.update({f.replace("_seconds", "_ms"): round(1e3 * float(v), 3) for f, v in zip(stages, med)})
    out.update({"inverse_over_factor": round(float(med[3] / med[2]), 2), "inverse_tflops": round(2.0 * n ** 3 / 3.0 / float(med[3]) / 1e12, 2),
                "device_bytes": int(S.device_bytes), "min_point_pivot": float(S.min_point_pivot), "min_schur_pivot": float(S.min_schur_pivot)})
    gp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
