"""The scenes, pair lists and reference layout of tests/test_shared_covariance_cpu.py and tests/test_gpu_shared_covariance.py:
ceres_hip_bal_covariance on handles with shared intrinsics (design/28_shared_covariance.md).  The scenes are those of
tests/covariance_cases.py (`generated`, `scene_c`: shapes for the kernels' edges, not workloads), their pixels as generated, their state
with every group's intrinsics shared (shared_intrinsics_reference.share).  The reference is the shared-intrinsics restatement's dense
Jacobian (shared_intrinsics_reference.Problem.dense_jacobian) through covariance_reference's two routes.

  A-one          8 cameras, 40 points, one group, poses 0 and 1 constant: n = 39; EVERY pair, the group included (the whole matrix)
  A-two_single   camera 1 alone in group 1, poses 0 and 2 constant: n = 42 — a group of one camera
  B-each         32 cameras, a group per camera, poses 0 and 1 constant: n = 276, across the 256-column panel pair; groups 0 and 1 have
                 constant poses only — their rows carry a group cell and no pose cell
  B-three        three groups, the first two poses of group 0 constant: n = 189 — the handle runs the generic kernels
  C-two-huber    covariance_cases.scene_c (66 cameras; tracks of 32, 33, 64, 65 and 2 observations), two groups, the first two poses
                 of group 0 constant, Huber: n = 390; 65^2 row pairs are 67 rounds of 64 lanes, 64^2 exactly 64 rounds
  failures       scene A, one group, only pose 0 constant (the scale is free) and nothing constant: the Schur stage fails"""
import functools

import numpy as np

import covariance_cases as CC
import covariance_reference as CR
import frontend_reference as F
import shared_intrinsics_reference as SI


class Layout(CR.Layout):
    """Blocks (point q is q, the pose of camera c is num_points + c, group g is num_points + num_cameras + g) -> their columns in the
    program [points | poses of the free cameras | groups]; a constant pose has none.  covariance_reference.Layout knows one camera
    width: this one has three block kinds and takes its `blocks` and `scales`."""

    def __init__(self, num_points, num_cameras, num_groups, camera_column):
        self.np_, self.nc, self.ng = int(num_points), int(num_cameras), int(num_groups)
        self.ccol = np.asarray(camera_column)
        self.pcol = np.arange(self.np_)
        self.nfp = self.np_
        self.nfc = int(np.sum(self.ccol >= 0))
        self.n_f = 6 * self.nfc + 3 * self.ng
        self.n = 3 * self.nfp + self.n_f
        self.num_blocks = self.np_ + self.nc + self.ng

    def size(self, block):
        return 6 if self.np_ <= block < self.np_ + self.nc else 3

    def columns(self, block):
        if block < self.np_:
            return np.arange(3 * block, 3 * block + 3)
        if block < self.np_ + self.nc:
            c = int(self.ccol[block - self.np_])
            return None if c < 0 else 3 * self.nfp + np.arange(6 * c, 6 * c + 6)
        g = block - self.np_ - self.nc
        assert 0 <= g < self.ng, block
        return 3 * self.nfp + 6 * self.nfc + np.arange(3 * g, 3 * g + 3)


class Case:
    def __init__(self, name, scene, layout, constant, loss, pairs, succeeds, stage=None):
        self.name, self.scene, self.layout, self.loss, self.succeeds, self.stage = name, scene, layout, loss, succeeds, stage
        self.nc, self.npts = scene[0], scene[1]
        self.groups = SI.layout(layout, self.nc)
        self.constant = np.asarray(constant, dtype=np.int64)
        self.pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)

    def state(self):
        """The ambient state [3 per point | 9 per camera] with every group's intrinsics those of its first camera."""
        par = np.asarray(self.scene[5], dtype=np.float64)
        return SI.share(np.concatenate([par[9 * self.nc:], par[:9 * self.nc]]), self.nc, self.npts, self.groups)

    def device_problem(self, hip, solver_type=None, loss="case", generic=False):
        nc, npts, cam, pt, obs, _ = self.scene
        o = hip.LinearSolverOptions(type=hip.DENSE_SCHUR if solver_type is None else solver_type, preconditioner_type=hip.SCHUR_JACOBI,
                                    min_num_iterations=0, max_num_iterations=100, force_generic_path=generic)
        mask = np.zeros(nc, bool)
        mask[self.constant] = True
        gp = hip.BalProblem(o, nc, npts, cam, pt, obs, constant_cameras=mask if mask.any() else None, camera_groups=self.groups)
        loss = self.loss if loss == "case" else loss
        if loss:
            gp.set_loss(*loss)
        return gp

    def restatement(self, oracle, apply_loss_function=True):
        nc, npts, cam, pt, obs, _ = self.scene
        inner = F.problem(oracle.snavely_batch, 0, nc, npts, cam, pt, obs, np.argsort(pt, kind="stable"), self.loss if apply_loss_function else None)
        return SI.Problem(inner, nc, npts, self.groups, self.constant, self.state())

    def reference(self, oracle, apply_loss_function=True):
        """(layout, J): the dense Jacobian of the program at the case's state, loss-corrected unless switched off."""
        w = self.restatement(oracle, apply_loss_function)
        _, _, vals, _ = w.evaluate(w.compact(self.state()))
        return Layout(self.npts, self.nc, w.ng, w.ccol), w.dense_jacobian(vals)


def all_pairs(scene, groups):
    n = scene[0] + scene[1] + int(np.max(groups)) + 1
    return [(a, b) for a in range(n) for b in range(n)]


def points_through_the_group(scene, groups, constant=()):
    """Two points no camera sees both of, with a camera of one and a camera of the other in one group: in S their rows meet in that
    group's columns only.  None if the scene has no such pair."""
    npts, cam, pt = scene[1], scene[2], scene[3]
    groups = np.asarray(groups)
    seen = [set(cam[pt == q].tolist()) for q in range(npts)]
    for p in range(npts):
        for q in range(p + 1, npts):
            if not (seen[p] & seen[q]) and set(groups[list(seen[p])].tolist()) & set(groups[list(seen[q])].tolist()):
                return p, q
    return None


def sampled_pairs(scene, groups, constant, points_of_interest=()):
    """covariance_cases.sampled_pairs for three block kinds: every group's and every pose's own block; group-group cross pairs; ten
    pose-pose pairs (neighbours and far apart); pose-group pairs with the pose in and out of the group; point-group pairs; point-pose
    pairs seen and unseen; point-point pairs p != q, two points whose only common ground is a group among them; a point seen by a
    constant pose; the transposed order of some; repeated pairs; pairs with a constant pose."""
    nc, npts, cam, pt = scene[0], scene[1], scene[2], scene[3]
    groups = np.asarray(groups)
    ng = int(groups.max()) + 1
    C = lambda c: npts + c
    G = lambda g: npts + nc + g
    const = [int(c) for c in constant]
    f = [c for c in range(nc) if c not in set(const)]
    pairs = [(G(g), G(g)) for g in range(ng)] + [(C(c), C(c)) for c in range(nc)]
    if ng > 1:
        gg = [(0, 1), (0, ng - 1), (ng // 2, ng - 1), (1, ng // 2)]
        pairs += [(G(a), G(b)) for a, b in gg] + [(G(b), G(a)) for a, b in gg[:2]]
    cc_pairs = [(f[0], f[1]), (f[0], f[-1]), (f[1], f[len(f) // 2]), (f[len(f) // 2], f[-1]), (f[2], f[3]), (f[3], f[len(f) // 3]),
                (f[len(f) // 4], f[3 * len(f) // 4]), (f[-2], f[-1]), (f[len(f) // 3], f[2 * len(f) // 3]), (f[5], f[-3])]
    pairs += [(C(a), C(b)) for a, b in cc_pairs]
    pairs += [(C(b), C(a)) for a, b in cc_pairs[:4]]                      # transposed
    for c in (f[0], f[len(f) // 2], f[-1]):                                # pose - group, the pose in the group and out of it
        own = int(groups[c])
        pairs += [(C(c), G(own)), (G(own), C(c))]
        if ng > 1:
            other = (own + 1) % ng
            pairs += [(C(c), G(other)), (G(other), C(c))]
    by_const = sorted(set(pt[np.isin(cam, const)].tolist())) if const else []
    pts = list(points_of_interest) + [q for q in (0, npts // 2, npts - 1) + tuple(by_const[:1]) if q not in points_of_interest]
    through = points_through_the_group(scene, groups)
    if through is not None:
        pts += [q for q in through if q not in pts]
    pairs += [(q, q) for q in pts]
    for q in pts:
        cams_q = sorted(set(cam[pt == q].tolist()))
        seen = [c for c in cams_q if c not in const]
        unseen = [c for c in f if c not in seen]
        if seen:
            pairs += [(q, C(seen[0])), (C(seen[0]), q), (q, C(seen[-1]))]
        if unseen:
            pairs += [(q, C(unseen[0])), (C(unseen[-1]), q)]
        gs = sorted(set(groups[cams_q].tolist()))
        not_gs = [g for g in range(ng) if g not in gs]
        pairs += [(q, G(gs[0])), (G(gs[0]), q), (q, G(gs[-1]))]
        if not_gs:
            pairs += [(q, G(not_gs[0])), (G(not_gs[-1]), q)]
    pairs += [(pts[i], pts[j]) for i in range(len(pts)) for j in range(len(pts)) if i < j][:12]
    poi = list(points_of_interest)
    pairs += [(poi[i], poi[i + 1]) for i in range(len(poi) - 1)]           # (scene C: the long tracks against each other)
    pairs += [(pts[1], pts[0]), (pts[2], pts[0]), (pts[-1], pts[1])]       # transposed
    if through is not None:
        pairs += [through, through[::-1]]
    point_group = next(pr for pr in pairs if pr[0] < npts and pr[1] >= G(0))
    pairs += [pairs[len(pairs) // 2], pairs[-5], (C(f[0]), C(f[1])), (G(0), G(0)), point_group]   # repeated
    for c in const[:2]:
        g = int(groups[c])
        pairs += [(C(c), C(f[0])), (C(f[0]), C(c)), (pts[0], C(c)), (C(c), pts[0]), (C(c), G(g)), (G(g), C(c))]
    return pairs


TRACKS = [0, 1, 2, 3, CC.TWO_OBSERVATION_POINT]   # of scene C: 32, 33, 64, 65 and 2 observations


@functools.lru_cache(maxsize=None)
def _cases(oracle):
    A = CC.generated(oracle, 8, 40, 240, seed=101)
    B = CC.generated(oracle, 32, 110, 1300, seed=202)
    Cs = CC.scene_c(oracle)
    lay = lambda name, sc: SI.layout(name, sc[0])
    two = lambda name, sc: SI.constant_cameras("two", lay(name, sc)).tolist()
    cases = [
        Case("A-one", A, "one", [0, 1], None, all_pairs(A, lay("one", A)), True),
        Case("A-two_single", A, "two_single", [0, 2], None, sampled_pairs(A, lay("two_single", A), [0, 2]), True),
        Case("B-each", B, "each", [0, 1], None, sampled_pairs(B, lay("each", B), [0, 1]), True),
        Case("B-three", B, "three", two("three", B), None, sampled_pairs(B, lay("three", B), two("three", B)), True),
        Case("C-two-huber", Cs, "two", two("two", Cs), CC.HUBER, sampled_pairs(Cs, lay("two", Cs), two("two", Cs), TRACKS), True),
        Case("A-one-pose0-only", A, "one", [0], None, all_pairs(A, lay("one", A))[:60], False, "Schur"),
        Case("A-one-nothing-constant", A, "one", [], None, all_pairs(A, lay("one", A))[:60], False, "Schur"),
    ]
    return cases


def cases(oracle):
    return list(_cases(oracle))


def case(oracle, name):
    return {c.name: c for c in _cases(oracle)}[name]


SUCCESS = ("A-one", "A-two_single", "B-each", "B-three", "C-two-huber")
FAILURE = ("A-one-pose0-only", "A-one-nothing-constant")
SIZES = {"A-one": 39, "A-two_single": 42, "B-each": 276, "B-three": 189, "C-two-huber": 390}   # n = 6 (free cameras) + 3 (groups)


@functools.lru_cache(maxsize=None)
def reference_results(oracle, name, apply_loss_function=True):
    """What the restatement says of a case, computed once: layout, J, route (a) (None for a failure case), route (b)."""
    c = case(oracle, name)
    layout, J = c.reference(oracle, apply_loss_function)
    b = CR.schur_covariance(J, layout.e_sizes())
    a = CR.dense_covariance(J) if c.succeeds else None
    return layout, J, a, b


@functools.lru_cache(maxsize=None)
def yardstick(oracle):
    """covariance_cases.yardstick over these cases: y = the larger, over every success case, of route (a) against route (b) and of route
    (a)'s move when every Jacobian value is multiplied by 1 + 1e-15 N(0, 1) (seeds 1 and 2), in the correlation scale over the requested
    blocks.  Returns (y, per-case dict of (route deviation, perturbation deviation))."""
    per = {}
    for name in SUCCESS:
        c = case(oracle, name)
        layout, J, a, b = reference_results(oracle, name)
        scales = layout.scales(np.diag(a), c.pairs)
        ra = layout.blocks(a, c.pairs)
        route = CR.correlation_deviation(layout.blocks(b["cov"], c.pairs), ra, scales)
        noise = max(CR.correlation_deviation(layout.blocks(CR.dense_covariance(CR.perturbed(J, seed)), c.pairs), ra, scales) for seed in (1, 2))
        per[name] = (route, noise)
    return max(max(v) for v in per.values()), per
