"""A numpy restatement of constant parameter blocks in the BAL front end (ceres_hip_bal_create_with_constant_blocks):
Problem::SetParameterBlockConstant, Program::RemoveFixedBlocks and the Schur ordering of what is left.

  reduce               the reduction: kept rows in order, the columns of the free blocks (csrc/constant_blocks.inc)
  Problem              frontend_reference.Problem's interface (n, evaluate, cost, dense_jacobian, plus, gradient_max_norm) around the
                       existing evaluators, so that frontend_reference.minimize runs on it unchanged: the state is full, the tangent
                       side is the reduced program's
  fixed_cost           the removed rows' cost (Solver::Summary::fixed_cost)
  inner_ordering       inner_reference.ordering on the reduced program; Problem.ev (what frontend_reference.minimize hands to
                       inner_reference.one_pass) sees ALL observations, so a free block's loop keeps its rows against constant blocks

It copies none of the evaluators, the minimizer or the inner iterations; tests/test_constant_blocks_cpu.py holds it to things that do
not depend on it."""
import numpy as np

import frontend_reference as F
import inner_reference as IR
import robust_reference as R


def mask(which, n):
    """None, an index array or a boolean mask -> a boolean mask of length n."""
    m = np.zeros(n, bool)
    if which is None:
        return m
    a = np.asarray(which)
    if a.dtype == np.bool_:
        assert a.shape == (n,)
        return a.copy()
    if a.size:
        m[a.astype(np.int64)] = True
    return m


def reduce(num_cameras, num_points, camera_index, point_index, constant_cameras=None, constant_points=None):
    """(row_observation, num_rows_e, camera_column, point_column, removed observations).  A residual block whose blocks are both
    constant is removed; the others are grouped by point, stable in observation order, the rows of constant points (no E cell)
    behind every row that has one, stable in observation order; columns: index among the free blocks, -1 for a constant one."""
    cam, pt = np.asarray(camera_index, dtype=np.int64), np.asarray(point_index, dtype=np.int64)
    cc, pc = mask(constant_cameras, num_cameras), mask(constant_points, num_points)
    obs = np.arange(cam.shape[0])
    with_e = obs[~pc[pt]]
    with_e = with_e[np.argsort(pt[with_e], kind="stable")]
    tail = obs[pc[pt] & ~cc[cam]]
    removed = obs[pc[pt] & cc[cam]]
    ccol = np.where(cc, -1, np.cumsum(~cc) - 1)
    pcol = np.where(pc, -1, np.cumsum(~pc) - 1)
    return np.concatenate([with_e, tail]).astype(np.int32), int(with_e.size), ccol.astype(np.int32), pcol.astype(np.int32), removed


class Problem:
    """The reduced program of a BAL problem with constant blocks behind frontend_reference.Problem's interface.  `full` is the
    frontend_reference.Problem of the KEPT rows in the reduced program's row order, with every block's columns; this class deletes the
    constant blocks' columns and cells and scatters tangent vectors back."""

    def __init__(self, snavely_batch, model, num_cameras, num_points, camera_index, point_index, observations, constant_cameras=None,
                 constant_points=None, loss=None):
        self.model, self.nc, self.np_, self.loss = model, int(num_cameras), int(num_points), loss
        self.cam, self.pt = np.asarray(camera_index), np.asarray(point_index)
        self.obs = np.asarray(observations, dtype=np.float64).reshape(-1, 2)
        self.row_order, self.n_rows_e, self.ccol, self.pcol, self.removed = reduce(num_cameras, num_points, camera_index, point_index,
                                                                                   constant_cameras, constant_points)
        self.snavely = snavely_batch
        self.full = F.problem(snavely_batch, model, num_cameras, num_points, camera_index, point_index, observations, self.row_order, loss)
        self.quaternion = self.full.quaternion
        self.cs = 10 if model else 9
        self.cw = 10 if model == 1 else 9
        nr = self.row_order.shape[0]
        self.n_rows = nr
        self.row_has_e = self.pcol[self.pt[self.row_order]] >= 0
        self.row_has_f = self.ccol[self.cam[self.row_order]] >= 0
        assert np.all(self.row_has_e[:self.n_rows_e]) and not np.any(self.row_has_e[self.n_rows_e:])
        # the free blocks' columns of the full tangent vector, free points then free cameras, ascending; and their doubles in the state
        fp, fc = np.flatnonzero(self.pcol >= 0), np.flatnonzero(self.ccol >= 0)
        self.free_cols = np.concatenate([(3 * fp[:, None] + np.arange(3)).reshape(-1),
                                         (3 * self.np_ + self.cw * fc[:, None] + np.arange(self.cw)).reshape(-1)]).astype(np.int64)
        kp, kc = np.flatnonzero(self.pcol < 0), np.flatnonzero(self.ccol < 0)
        self.constant_state = np.concatenate([(3 * kp[:, None] + np.arange(3)).reshape(-1),
                                              (3 * self.np_ + self.cs * kc[:, None] + np.arange(self.cs)).reshape(-1)]).astype(np.int64)
        self.n_full = self.full.n
        self.n = int(self.free_cols.size)
        # positions of the kept cells in the full value layout [E cells 6 per row | F cells 2 cw per row]
        e_rows, f_rows = np.flatnonzero(self.row_has_e), np.flatnonzero(self.row_has_f)
        self.value_index = np.concatenate([(6 * e_rows[:, None] + np.arange(6)).reshape(-1),
                                           (6 * nr + 2 * self.cw * f_rows[:, None] + np.arange(2 * self.cw)).reshape(-1)]).astype(np.int64)
        self.n_values_full = (6 + 2 * self.cw) * nr
        # what inner_reference.one_pass runs on (frontend_reference.minimize passes ev.ev): every observation, the caller's order
        self.ev = R.Evaluator(snavely_batch, num_cameras, num_points, camera_index, point_index, observations,
                              np.arange(self.cam.shape[0]), loss) if model == 0 and self.removed.size else self.full.ev

    def _scatter(self, v):
        out = np.zeros(self.n_full)
        out[self.free_cols] = v
        return out

    def evaluate(self, x):
        cost, r, vals, g = self.full.evaluate(x)
        return cost, r, vals[self.value_index], g[self.free_cols]

    def cost(self, x):
        return self.full.cost(x)

    def dense_jacobian(self, vals):
        v = np.zeros(self.n_values_full)
        v[self.value_index] = vals
        return np.ascontiguousarray(self.full.dense_jacobian(v)[:, self.free_cols])   # (row-major, as the unwrapped problem's)

    def plus(self, x, delta):
        out = self.full.plus(x, self._scatter(delta))
        out[self.constant_state] = np.asarray(x)[self.constant_state]   # read, never written
        return out

    def gradient_max_norm(self, x, g):
        return self.full.gradient_max_norm(x, self._scatter(g))

    def fixed_cost(self, x):
        """1/2 sum rho over the removed rows, by the unwrapped evaluator."""
        if self.removed.size == 0:
            return 0.0
        return F.problem(self.snavely, self.model, self.nc, self.np_, self.cam, self.pt, self.obs, self.removed, self.loss).cost(x)

    def inner_ordering(self, blocks):
        """(group per block in state order, groups) of the reduced program: the graph of the free blocks (residual blocks that join two
        of them), constant blocks in no group."""
        both = (self.ccol[self.cam] >= 0) & (self.pcol[self.pt] >= 0)
        group, ng = IR.ordering(self.nc, self.np_, self.cam[both], self.pt[both], blocks)
        group = np.array(group)
        group[:self.np_][self.pcol < 0] = -1
        group[self.np_:][self.ccol < 0] = -1
        return group, ng


MASK_SETS = ("camera0", "cameras01_points3", "camera_of_constant_points", "point_of_constant_cameras", "both_constant", "points_only",
             "none")


def mask_set(name, num_cameras, num_points, camera_index, point_index):
    """(constant cameras, constant points) of the tests' mask sets on a scene: (a) camera 0; (b) cameras {0, 1} and three points;
    (c) a camera all of whose points are constant (the camera with the fewest observations: all its rows lose their E cell); (d) a
    point seen only by constant cameras (the point with the fewest observations: its rows keep an E cell alone); (e) an observation
    with both blocks constant (a removed row); (f) constant points only; (g) nothing constant."""
    cam, pt = np.asarray(camera_index), np.asarray(point_index)
    if not isinstance(name, str):   # (constant cameras, constant points) given outright (tools/fuzz_frontend.py --masks)
        return list(name[0]), list(name[1])
    if name == "camera0":
        return [0], []
    if name == "cameras01_points3":
        return [0, 1], [3, 7, 50]
    if name == "camera_of_constant_points":
        c = int(np.argmin(np.bincount(cam, minlength=num_cameras)))
        return [], sorted(set(pt[cam == c].tolist()))
    if name == "point_of_constant_cameras":
        q = int(np.argmin(np.bincount(pt, minlength=num_points)))
        return sorted(set(cam[pt == q].tolist())), []
    if name == "both_constant":
        return [int(cam[0])], [int(pt[0])]
    if name == "points_only":
        return [], list(range(10, 40))
    assert name == "none", name
    return [], []
