"""A numpy restatement of fixed camera intrinsics in the BAL front end (ceres_hip_bal_create_with_fixed_intrinsics): SubsetManifold(9,
marked coordinates) on every angle-axis camera block.  PlusJacobian of a SubsetManifold is a selection, so the local Jacobian is the
ambient one with the marked columns deleted, and Plus adds the tangent step to the free coordinates.

  Problem     frontend_reference.Problem's interface (n, evaluate, cost, dense_jacobian, plus, gradient_max_norm, ev, quaternion) around
              a frontend_reference.Problem of camera model 0 or a constant_blocks_reference.Problem: it deletes the marked columns of
              every free camera and scatters tangent vectors back, so that frontend_reference.minimize runs on it unchanged

It copies no evaluator and no minimizer; tests/test_fixed_intrinsics_cpu.py holds it to the wrapped problems."""
import numpy as np

import constant_blocks_reference as CB

INTRINSICS = {"f": 6, "k1": 7, "k2": 8}
# the masks under test: name -> marked coordinates (camera widths 6, 7, 8)
MASKS = {"f,k1,k2": (6, 7, 8), "k1,k2": (7, 8), "f": (6,)}


def marked(mask):
    """Names, indices or a boolean mask of nine -> the sorted marked coordinates."""
    if mask is None:
        return ()
    if isinstance(mask, str):
        mask = MASKS[mask] if mask in MASKS else [mask]
    a = list(mask)
    if len(a) == 9 and all(isinstance(v, (bool, np.bool_)) for v in a):
        return tuple(int(j) for j in np.flatnonzero(a))
    return tuple(sorted({INTRINSICS[v] if isinstance(v, str) else int(v) for v in a}))


class Problem:
    """`inner` with the marked coordinates of every free camera held fixed.  inner: a frontend_reference.Problem of angle-axis cameras
    (every block free) or a constant_blocks_reference.Problem of camera model 0 (the mask applies to its free cameras)."""

    def __init__(self, inner, num_cameras, num_points, mask):
        assert not inner.quaternion, "fixed intrinsics: angle-axis cameras only"
        self.inner, self.quaternion, self.ev = inner, False, inner.ev
        self.nc, self.np_ = int(num_cameras), int(num_points)
        self.marked = marked(mask)
        assert all(6 <= j <= 8 for j in self.marked), self.marked
        self.free = np.array([j for j in range(9) if j not in self.marked], dtype=np.int64)
        self.cw = int(self.free.size)
        reduced = isinstance(inner, CB.Problem)
        self.reduced = reduced
        if reduced:
            assert inner.model == 0
            nfp, nfc = int(np.count_nonzero(inner.pcol >= 0)), int(np.count_nonzero(inner.ccol >= 0))
            n_e, n_f = int(np.count_nonzero(inner.row_has_e)), int(np.count_nonzero(inner.row_has_f))
        else:   # (the unwrapped evaluator: one row with both cells per observation)
            nfp, nfc = self.np_, self.nc
            n_e = n_f = int(inner.ev.n_rows)
        self.nfp, self.nfc = nfp, nfc
        assert inner.n == 3 * nfp + 9 * nfc
        # the tangent columns kept: every point column, the free coordinates of every free camera, ascending
        self.keep_cols = np.concatenate([np.arange(3 * nfp), (3 * nfp + 9 * np.arange(nfc)[:, None] + self.free).reshape(-1)]).astype(np.int64)
        # the Jacobian values kept: every E cell, the free columns of both rows of every F cell (2 x 9 row-major -> 2 x cw row-major)
        cell = np.concatenate([self.free, 9 + self.free])
        self.n_values_inner = 6 * n_e + 18 * n_f
        self.keep_vals = np.concatenate([np.arange(6 * n_e), (6 * n_e + 18 * np.arange(n_f)[:, None] + cell).reshape(-1)]).astype(np.int64)
        self.n = int(self.keep_cols.size)
        # the marked doubles of the state, of every camera: read, never written
        self.marked_state = (3 * self.np_ + 9 * np.arange(self.nc)[:, None] + np.array(self.marked, dtype=np.int64)).reshape(-1)

    # what the reduced program's tests ask of constant_blocks_reference.Problem, passed on (the identity reduction otherwise)
    def __getattr__(self, name):
        if name in ("row_order", "n_rows", "n_rows_e", "removed", "ccol", "pcol", "constant_state", "fixed_cost") and self.__dict__.get("reduced"):
            return getattr(self.inner, name)
        raise AttributeError(name)

    def _scatter(self, v):
        out = np.zeros(self.inner.n)
        out[self.keep_cols] = v
        return out

    def evaluate(self, x):
        cost, r, vals, g = self.inner.evaluate(x)
        assert vals.size == self.n_values_inner
        return cost, r, vals[self.keep_vals], g[self.keep_cols]

    def cost(self, x):
        return self.inner.cost(x)

    def dense_jacobian(self, vals):
        v = np.zeros(self.n_values_inner)
        v[self.keep_vals] = vals
        return np.ascontiguousarray(self.inner.dense_jacobian(v)[:, self.keep_cols])   # (row-major, as the wrapped problem's)

    def plus(self, x, delta):
        out = self.inner.plus(x, self._scatter(delta))
        out[self.marked_state] = np.asarray(x)[self.marked_state]   # read, never written (x + 0.0 would turn a -0.0 into 0.0)
        return out

    def gradient_max_norm(self, x, g):
        return self.inner.gradient_max_norm(x, self._scatter(g))


def conditioning(problem, x0, strategy, max_num_iterations=8, **opts):
    """How far the restatement's own trajectory moves when every Jacobian value is multiplied by 1 + 1e-14 N(0, 1), seeds 1 and 2
    (test_gpu_frontend_matrix.EDGE_ILL_CONDITIONED's method): (the largest relative cost deviation, flags changed)."""
    import frontend_reference as F
    _, Sr = F.minimize(problem, x0, strategy, max_num_iterations=max_num_iterations, **opts)
    worst, flags = 0.0, 0
    for seed in (1, 2):
        _, Sn = F.minimize(problem, x0, strategy, jacobian_noise=(1e-14, seed), max_num_iterations=max_num_iterations, **opts)
        worst = max([worst] + [abs(a["cost"] - b["cost"]) / b["cost"] for a, b in zip(Sn["iterations"], Sr["iterations"])])
        flags += sum((a["step_is_successful"], a["step_is_valid"]) != (b["step_is_successful"], b["step_is_valid"])
                     for a, b in zip(Sn["iterations"], Sr["iterations"])) + abs(len(Sn["iterations"]) - len(Sr["iterations"]))
    return worst, flags
