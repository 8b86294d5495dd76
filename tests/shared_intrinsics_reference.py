"""A numpy restatement of shared camera intrinsics in the BAL front end (ceres_hip_bal_create_with_shared_intrinsics): one 3-wide
parameter block [f, k1, k2] per group of cameras beside a 6-wide pose block per camera, as examples/libmv_bundle_adjuster.cc adds its
residual blocks; a constant camera is a constant pose block.

  Problem     frontend_reference.Problem's interface (n, evaluate, cost, dense_jacobian, plus, gradient_max_norm, ev, quaternion) around
              a frontend_reference.Problem of camera model 0.  Its state is Ceres' compact one, [points | poses of the free cameras |
              groups]; `expand` builds the ambient state the wrapped problem (and the device) takes, `compact` goes back.  evaluate
              calls the wrapped problem and regroups: values into [E cells, 6 per row | per row: pose cell 12, group cell 6], the
              gradient by P^T, where P is the 0/1 matrix that sends a free camera's pose columns and a group's columns to the ambient
              columns of its cameras.  dense_jacobian is J_ambient P; plus is x + delta.  frontend_reference.minimize runs on it
              unchanged — its norm(x) counts a group once and a constant pose not at all because the compact state does.

It copies no evaluator and no minimizer; tests/test_shared_intrinsics_cpu.py holds it to the wrapped problem."""
import numpy as np

# grouping layouts under test: name -> camera -> group
LAYOUTS = {
    "one": lambda nc: np.zeros(nc, np.int32),
    "two": lambda nc: (np.arange(nc) % 2).astype(np.int32),
    "two_single": lambda nc: (np.arange(nc) == 1).astype(np.int32),    # group 1 is camera 1 alone
    "three": lambda nc: (np.arange(nc) % 3).astype(np.int32),
    "each": lambda nc: np.arange(nc, dtype=np.int32),                  # num_groups == num_cameras
}
# constant-camera sets: name -> (groups) -> camera indices; "two": the first two cameras of group 0 (cameras 0 and 1 where they share
# a group; with every camera in a group of its own, cameras 0 and 1 — groups all of whose cameras are constant, which stay free)
CONSTANT_SETS = ("none", "camera0", "two")


def layout(name, nc):
    return LAYOUTS[name](int(nc))


def constant_cameras(name, groups):
    groups = np.asarray(groups)
    if name == "none":
        return np.zeros(0, np.int64)
    if name == "camera0":
        return np.array([0], np.int64)
    assert name == "two", name
    first = np.flatnonzero(groups == groups[0])
    return first[:2].astype(np.int64) if first.size >= 2 else np.array([0, 1], np.int64)


def share(x_ambient, num_cameras, num_points, groups):
    """The ambient state with every camera's intrinsics replaced by those of the first camera of its group (bit-identical)."""
    x = np.array(x_ambient, dtype=np.float64)
    cams = x[3 * num_points:].reshape(num_cameras, 9)
    groups = np.asarray(groups)
    for g in range(int(groups.max()) + 1):
        members = np.flatnonzero(groups == g)
        cams[members, 6:] = cams[members[0], 6:]
    return x


class Problem:
    """`inner` (a frontend_reference.Problem of angle-axis cameras, rows with both cells) with the intrinsics of every group of cameras
    one parameter block.  x_ambient: where the constant cameras' poses are read from (never written)."""

    def __init__(self, inner, num_cameras, num_points, groups, constant=(), x_ambient=None):
        assert not inner.quaternion, "shared intrinsics: angle-axis cameras only"
        self.inner, self.quaternion, self.ev = inner, False, inner.ev
        nc, npts = int(num_cameras), int(num_points)
        self.nc, self.np_ = nc, npts
        self.groups = np.asarray(groups, dtype=np.int64)
        assert self.groups.shape == (nc,) and self.groups.min() >= 0
        self.ng = int(self.groups.max()) + 1
        assert np.array_equal(np.unique(self.groups), np.arange(self.ng)), "every group id is used"
        self.first = np.array([np.flatnonzero(self.groups == g)[0] for g in range(self.ng)], dtype=np.int64)
        is_const = np.zeros(nc, bool)
        is_const[np.asarray(constant, dtype=np.int64)] = True
        self.free_cams = np.flatnonzero(~is_const)
        self.ccol = np.full(nc, -1, np.int64)
        self.ccol[self.free_cams] = np.arange(self.free_cams.size)
        self.nfc = int(self.free_cams.size)
        assert inner.n == 3 * npts + 9 * nc
        self.n = 3 * npts + 6 * self.nfc + 3 * self.ng
        self.template = None if x_ambient is None else np.array(x_ambient, dtype=np.float64)
        assert self.nfc == nc or self.template is not None, "constant poses are read from x_ambient"
        # compact column of every ambient column, -1: the pose of a constant camera
        amb = np.full(inner.n, -1, np.int64)
        amb[:3 * npts] = np.arange(3 * npts)
        for c in range(nc):
            a = 3 * npts + 9 * c
            if self.ccol[c] >= 0:
                amb[a:a + 6] = 3 * npts + 6 * self.ccol[c] + np.arange(6)
            amb[a + 6:a + 9] = 3 * npts + 6 * self.nfc + 3 * self.groups[c] + np.arange(3)
        self.amb_col = amb
        self.kept = np.flatnonzero(amb >= 0)   # P as an index map: ambient column kept[i] goes to compact column amb[kept[i]]
        # the ambient doubles the program never writes: the constant cameras' poses
        self.constant_state = np.flatnonzero(amb < 0)
        # the rows: one per observation, in the wrapped evaluator's order; the values' regrouping
        self.row_cam = np.asarray(self.ev.cam, dtype=np.int64)
        n = int(self.ev.n_rows)
        self.n_rows = n
        has_pose = self.ccol[self.row_cam] >= 0
        self.row_has_pose = has_pose
        width = np.where(has_pose, 18, 6).astype(np.int64)
        start = 6 * n + np.concatenate([[0], np.cumsum(width)[:-1]])
        self.n_values = int(6 * n + width.sum())
        self.row_start = start
        # inner F cell (2 x 9 row-major at 6 n + 18 r) -> [pose cell 2 x 6 row-major | group cell 2 x 3 row-major]
        pose_src = np.concatenate([np.arange(6), 9 + np.arange(6)])
        grp_src = np.concatenate([6 + np.arange(3), 15 + np.arange(3)])
        f = 6 * n + 18 * np.arange(n, dtype=np.int64)
        rows_p = np.flatnonzero(has_pose)
        src = [np.arange(6 * n), (f[rows_p][:, None] + pose_src).reshape(-1), (f[:, None] + grp_src).reshape(-1)]
        dst = [np.arange(6 * n), (start[rows_p][:, None] + np.arange(12)).reshape(-1), ((start + 12 * has_pose)[:, None] + np.arange(6)).reshape(-1)]
        self.val_src, self.val_dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
        assert self.val_dst.size == self.n_values and np.array_equal(np.bincount(self.val_dst, minlength=self.n_values), np.ones(self.n_values, np.int64))

    def structure(self):
        """(column block sizes, rows) of the program as the header states it — points (3), the free cameras' poses (6), groups (3); a
        row is (2, [(column block, value position), ...]): its E cell, its pose cell unless the camera is constant, its group cell —
        the arguments of BlockStructure.from_rows."""
        npts, nfc = self.np_, self.nfc
        sizes = [3] * npts + [6] * nfc + [3] * self.ng
        pt = np.asarray(self.ev.pt, dtype=np.int64)
        rows = []
        for r in range(self.n_rows):
            c = self.row_cam[r]
            cells = [(int(pt[r]), 6 * r)]
            at = int(self.row_start[r])
            if self.row_has_pose[r]:
                cells.append((npts + int(self.ccol[c]), at))
                at += 12
            cells.append((npts + nfc + int(self.groups[c]), at))
            rows.append((2, cells))
        return sizes, rows

    def expand(self, xc):
        """The ambient state [points | nine per camera] of a compact one."""
        xc = np.asarray(xc, dtype=np.float64)
        npts, nc = self.np_, self.nc
        x = np.zeros(self.inner.n) if self.template is None else self.template.copy()
        x[:3 * npts] = xc[:3 * npts]
        cams = x[3 * npts:].reshape(nc, 9)
        cams[self.free_cams, :6] = xc[3 * npts:3 * npts + 6 * self.nfc].reshape(-1, 6)
        cams[:, 6:] = xc[3 * npts + 6 * self.nfc:].reshape(-1, 3)[self.groups]
        return x

    def compact(self, x):
        """The compact state of an ambient one (a group's intrinsics from its first camera)."""
        x = np.asarray(x, dtype=np.float64)
        cams = x[3 * self.np_:].reshape(self.nc, 9)
        return np.concatenate([x[:3 * self.np_], cams[self.free_cams, :6].reshape(-1), cams[self.first, 6:].reshape(-1)])

    def groups_identical(self, x):
        """Whether every camera of an ambient state holds its group's bits."""
        cams = np.asarray(x)[3 * self.np_:].reshape(self.nc, 9)[:, 6:].view(np.int64)
        return bool(np.array_equal(cams, cams[self.first][self.groups]))

    def project(self, g):
        """P^T g: an ambient gradient's entries added into the compact columns (a group's from all its cameras, in camera order)."""
        return np.bincount(self.amb_col[self.kept], weights=np.asarray(g)[self.kept], minlength=self.n)

    def evaluate(self, xc):
        cost, r, vals, g = self.inner.evaluate(self.expand(xc))
        out = np.empty(self.n_values)
        out[self.val_dst] = vals[self.val_src]
        return cost, r, out, self.project(g)

    def cost(self, xc):
        return self.inner.cost(self.expand(xc))

    def dense_jacobian(self, vals):
        v = np.zeros(6 * self.n_rows + 18 * self.n_rows)   # (a constant camera's pose cell: zeros, its columns are deleted by P)
        v[self.val_src] = np.asarray(vals)[self.val_dst]
        J = self.inner.dense_jacobian(v)
        out = np.zeros((self.n, J.shape[0]))
        np.add.at(out, self.amb_col[self.kept], J.T[self.kept])   # J P: a group's column is the sum of its cameras' columns
        return np.ascontiguousarray(out.T)

    def plus(self, xc, delta):
        return xc + delta

    def gradient_max_norm(self, xc, g):
        return float(np.max(np.abs(g)))
