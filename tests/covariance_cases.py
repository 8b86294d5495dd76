"""The scenes and pair lists of tests/test_covariance_cpu.py and tests/test_gpu_covariance.py.  The shapes are chosen for the kernels'
boundaries (the factorisation's 128-column panels and 256-column panel pairs, the inversion's 32-column blocks, the blocks pass's
64-lane rounds), not for any workload; every scene runs in seconds.

  A   8 cameras, cameras 0 and 1 constant: n_f = 54, less than one panel; EVERY pair is requested (the whole matrix comes back)
  B   32 cameras: n_f = 270, two panels and a remainder, across the 256-column panel pair — cameras 0 and 1 constant; camera 0 and
      point 0 constant (n_f = 279); cameras 0 and 1 and three more points constant, one of them seen by a constant camera (rows
      without an E cell and removed rows)
  C   test_gpu_frontend_matrix.edge_scene(lonely=False) without its point of one observation: 66 cameras, tracks of 32, 33, 64 and
      65 observations, one point cut down to 2; the quaternion manifold (n_f = 576) and angle-axis with a Huber loss (576); the
      Euclidean quaternion camera (640, exactly five panels) only fails: QuaternionRotatePoint normalises, every camera has a null
      direction
  failures: only camera 0 constant and nothing constant on scene A (the gauge is free), the Euclidean quaternion handle of scene C,
  and scene C with its single-observation point kept (the point factorisation)."""
import functools

import numpy as np

import constant_blocks_reference as CB
import covariance_reference as CR
from test_gpu_frontend_matrix import LOSS_PARAMS, MODELS, edge_scene

HUBER = ("huber",) + LOSS_PARAMS["huber"] + (1.0,)


class Case:
    def __init__(self, name, scene, camera, constant_cameras, constant_points, loss, pairs, succeeds, stage=None):
        self.name, self.scene, self.camera, self.loss, self.succeeds, self.stage = name, scene, camera, loss, succeeds, stage
        self.nc, self.npts = scene[0], scene[1]
        self.cc, self.cp = CB.mask(constant_cameras, self.nc), CB.mask(constant_points, self.npts)
        self.pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)

    def state(self, hs):
        """The state [3 per point | cameras] of the scene's BAL-order parameters, as BalProblem.state_from_bal converts them."""
        par = np.asarray(self.scene[5], dtype=np.float64)
        cams = par[:9 * self.nc]
        if MODELS[self.camera]:
            c9 = cams.reshape(-1, 9)
            cams = np.concatenate([hs.angle_axis_to_quaternion(c9[:, :3]), c9[:, 3:]], axis=1).reshape(-1)
        return np.concatenate([par[9 * self.nc:], cams])

    def device_problem(self, hip, solver_type=None):
        nc, npts, cam, pt, obs, _ = self.scene
        o = hip.LinearSolverOptions(type=hip.DENSE_SCHUR if solver_type is None else solver_type, preconditioner_type=hip.SCHUR_JACOBI,
                                    min_num_iterations=0, max_num_iterations=100)
        gp = hip.BalProblem(o, nc, npts, cam, pt, obs, camera_model=self.camera, constant_cameras=self.cc, constant_points=self.cp)
        if self.loss:
            gp.set_loss(*self.loss)
        return gp

    def reference(self, oracle, hs, apply_loss_function=True):
        """(layout, J): the dense Jacobian of the reduced program at the case's state, loss-corrected unless switched off."""
        nc, npts, cam, pt, obs, _ = self.scene
        ref = CB.Problem(oracle.snavely_batch, MODELS[self.camera], nc, npts, cam, pt, obs, np.flatnonzero(self.cc), np.flatnonzero(self.cp),
                         self.loss if apply_loss_function else None)
        _, _, vals, _ = ref.evaluate(self.state(hs))
        return CR.Layout(npts, nc, ref.pcol, ref.ccol, ref.cw), ref.dense_jacobian(vals)


def generated(oracle, nc, npts, nobs, seed):
    op = oracle.BalProblem.generate(nc, npts, nobs, seed=seed)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    x = op.state()
    return nc, npts, cam.astype(np.int32), pt.astype(np.int32), obs, np.concatenate([x[3 * npts:], x[:3 * npts]])


TWO_OBSERVATION_POINT = 10   # of scene C (after its first point is dropped)


def scene_c(oracle, keep_single=False):
    """edge_scene(lonely=False); its point 0 (one observation) dropped and the points renumbered unless keep_single; one more point cut
    down to its first two observations."""
    nc, npts, cam, pt, obs, par = edge_scene(oracle, lonely=False)
    cams, pts = par[:9 * nc], par[9 * nc:].reshape(-1, 3)
    if not keep_single:
        keep = pt != 0
        cam, pt, obs, pts, npts = cam[keep], pt[keep] - 1, obs[keep], pts[1:], npts - 1
    two = TWO_OBSERVATION_POINT + (1 if keep_single else 0)
    rows = np.flatnonzero(pt == two)
    keep = np.ones(cam.shape[0], bool)
    keep[rows[2:]] = False
    cam, pt, obs = cam[keep], pt[keep], obs[keep]
    assert np.bincount(cam, minlength=nc).min() >= 5
    return nc, npts, cam.astype(np.int32), pt.astype(np.int32), obs, np.concatenate([cams, pts.reshape(-1)])


def all_pairs(scene):
    n = scene[0] + scene[1]
    return [(a, b) for a in range(n) for b in range(n)]


def sampled_pairs(scene, constant_cameras, constant_points, points_of_interest=()):
    """Every camera's own block; ten camera-camera pairs (neighbours and far apart: across the factorisation's panels and the inversion's
    levels); own blocks of the points of interest and a few more; point-camera pairs seen and unseen; point-point pairs p != q; the
    transposed order of some; a repeated pair; pairs with a constant block."""
    nc, npts, cam, pt = scene[0], scene[1], scene[2], scene[3]
    C = lambda c: npts + c
    free_c = [c for c in range(nc) if c not in set(constant_cameras)]
    free_p = [q for q in range(npts) if q not in set(constant_points)]
    pairs = [(C(c), C(c)) for c in range(nc)]
    f = free_c
    cc_pairs = [(f[0], f[1]), (f[0], f[-1]), (f[1], f[len(f) // 2]), (f[len(f) // 2], f[-1]), (f[2], f[3]), (f[3], f[len(f) // 3]),
                (f[len(f) // 4], f[3 * len(f) // 4]), (f[-2], f[-1]), (f[len(f) // 3], f[2 * len(f) // 3]), (f[5], f[-3])]
    pairs += [(C(a), C(b)) for a, b in cc_pairs]
    pairs += [(C(b), C(a)) for a, b in cc_pairs[:4]]                      # transposed
    pts = list(points_of_interest) + [q for q in (free_p[0], free_p[len(free_p) // 2], free_p[-1]) if q not in points_of_interest]
    pairs += [(q, q) for q in pts]
    for q in pts:
        seen = sorted(set(cam[pt == q].tolist()) - set(constant_cameras))
        unseen = [c for c in free_c if c not in seen]
        if seen:
            pairs += [(q, C(seen[0])), (C(seen[0]), q), (q, C(seen[-1]))]
        if unseen:
            pairs += [(q, C(unseen[0])), (C(unseen[-1]), q)]
    pairs += [(pts[i], pts[j]) for i in range(len(pts)) for j in range(len(pts)) if i < j][:12]
    pairs += [(pts[1], pts[0]), (pts[2], pts[0]), (pts[-1], pts[1])]       # transposed
    pairs += [pairs[len(pairs) // 2], pairs[-5], (C(f[0]), C(f[1]))]       # repeated
    for c in list(constant_cameras)[:2]:
        pairs += [(C(c), C(f[0])), (C(f[0]), C(c)), (pts[0], C(c)), (C(c), pts[0])]
    for q in list(constant_points)[:3]:
        pairs += [(q, q), (q, pts[0]), (pts[0], q), (q, C(f[0])), (C(f[0]), q)]
    return pairs


@functools.lru_cache(maxsize=None)
def _cases(oracle):
    A = generated(oracle, 8, 40, 240, seed=101)
    B = generated(oracle, 32, 110, 1300, seed=202)
    Cs = scene_c(oracle)
    Cl = scene_c(oracle, keep_single=True)
    b_cam = B[2]
    b_pt = B[3]
    # three more constant points of scene B: one seen by a constant camera (its row with that camera is removed), two others
    seen_by_const = sorted(set(b_pt[(b_cam == 0) | (b_cam == 1)].tolist()))
    b_points = [seen_by_const[0]] + [q for q in (50, 51, 52) if q != seen_by_const[0]][:2]
    tracks = [0, 1, 2, 3, TWO_OBSERVATION_POINT]   # 32, 33, 64, 65 and 2 observations
    cases = [
        Case("A-cameras01", A, "angle_axis", [0, 1], [], None, all_pairs(A), True),
        Case("B-cameras01", B, "angle_axis", [0, 1], [], None, sampled_pairs(B, [0, 1], []), True),
        Case("B-camera0-point0", B, "angle_axis", [0], [0], None, sampled_pairs(B, [0], [0]), True),
        Case("B-cameras01-points3", B, "angle_axis", [0, 1], b_points, None, sampled_pairs(B, [0, 1], b_points), True),
        Case("C-manifold", Cs, "quaternion_manifold", [0, 1], [], None, sampled_pairs(Cs, [0, 1], [], tracks), True),
        Case("C-angle_axis-huber", Cs, "angle_axis", [0, 1], [], HUBER, sampled_pairs(Cs, [0, 1], [], tracks), True),
        Case("A-camera0-only", A, "angle_axis", [0], [], None, all_pairs(A)[:40], False, "Schur"),
        Case("A-no-masks", A, "angle_axis", [], [], None, all_pairs(A)[:40], False, "Schur"),
        Case("C-quaternion", Cs, "quaternion", [0, 1], [], None, sampled_pairs(Cs, [0, 1], [], tracks)[:40], False, "Schur"),
        Case("C-single-observation-point", Cl, "angle_axis", [0, 1], [], None, [(0, 0), (1, 1)], False, "point"),
    ]
    return cases


def cases(oracle):
    return list(_cases(oracle))


def case(oracle, name):
    return {c.name: c for c in _cases(oracle)}[name]


SUCCESS = ("A-cameras01", "B-cameras01", "B-camera0-point0", "B-cameras01-points3", "C-manifold", "C-angle_axis-huber")
FAILURE = ("A-camera0-only", "A-no-masks", "C-quaternion", "C-single-observation-point")


@functools.lru_cache(maxsize=None)
def reference_results(oracle, hs, name, apply_loss_function=True):
    """What the restatement says of a case, computed once: layout, J, route (a) (None where J^T J cannot be inverted), route (b)."""
    c = case(oracle, name)
    layout, J = c.reference(oracle, hs, apply_loss_function)
    b = CR.schur_covariance(J, layout.e_sizes())
    a = CR.dense_covariance(J) if c.succeeds else None
    return layout, J, a, b


@functools.lru_cache(maxsize=None)
def yardstick(oracle, hs):
    """y of the parity tests: over every success case, the larger of the restatement's route (a) against route (b) deviation and route
    (a)'s deviation when every Jacobian value is multiplied by 1 + 1e-15 N(0, 1) (seeds 1 and 2), in the correlation scale over the
    requested blocks.  Returns (y, per-case dict of (route deviation, perturbation deviation))."""
    per = {}
    for name in SUCCESS:
        c = case(oracle, name)
        layout, J, a, b = reference_results(oracle, hs, name)
        scales = layout.scales(np.diag(a), c.pairs)
        ra = layout.blocks(a, c.pairs)
        route = CR.correlation_deviation(layout.blocks(b["cov"], c.pairs), ra, scales)
        noise = max(CR.correlation_deviation(layout.blocks(CR.dense_covariance(CR.perturbed(J, seed)), c.pairs), ra, scales) for seed in (1, 2))
        per[name] = (route, noise)
    return max(max(v) for v in per.values()), per
