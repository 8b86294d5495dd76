"""A numpy restatement of ceres_hip_bal_covariance (ceres::Covariance for the BAL front end): float64, from a dense Jacobian.  The
Jacobian comes from constant_blocks_reference.Problem.evaluate / dense_jacobian (every camera model, the losses, the masks); nothing of
those is copied here.  Two routes to the same matrix:

  dense_covariance     (a) np.linalg.inv(J^T J)
  schur_covariance     (b) the Schur form the device runs — C_p = E_p^T E_p, W_p = E_p^T F, Y_p = C_p^-1 W_p,
                       S = F^T F - sum_p W_p^T C_p^-1 W_p; camera-camera S^-1, point-camera -Y_p S^-1, point-point
                       delta_pq C_p^-1 + Y_p S^-1 Y_q^T — with the unit-diagonal scaling of every C_p and of S before their unpivoted
                       Cholesky factorisations, and the smallest pivots of both

tests/test_covariance_cpu.py holds both to the reference's known answers (tests/golden/covariance_known_answers.json) and to each other."""
import numpy as np


def dense_covariance(J):
    return np.linalg.inv(J.T @ J)


def scaled_cholesky(A):
    """Unpivoted Cholesky of Lambda A Lambda, Lambda = diag(A)^-1/2.  Returns (lam, G, smallest pivot, its column); G is None when the
    factorisation stops: a diagonal entry of A that is not positive (pivot 0) or a pivot that is not positive (that pivot)."""
    n = A.shape[0]
    d = np.diag(A)
    if not np.all(np.isfinite(d)) or np.any(d <= 0.0):
        return None, None, 0.0, int(np.argmax(~(d > 0.0)))
    lam = 1.0 / np.sqrt(d)
    T = A * lam[:, None] * lam[None, :]
    G = np.zeros((n, n))
    smallest, at = np.inf, -1
    for j in range(n):
        piv = T[j, j] - G[j, :j] @ G[j, :j]
        if piv < smallest:
            smallest, at = float(piv), j
        if not piv > 0.0:
            return lam, None, smallest, at
        G[j, j] = np.sqrt(piv)
        G[j + 1:, j] = (T[j + 1:, j] - G[j + 1:, :j] @ G[j, :j]) / G[j, j]
    return lam, G, smallest, at


def inverse_from_scaled_factor(lam, G):
    X = np.linalg.inv(G)   # (lower triangular)
    return (X.T @ X) * lam[:, None] * lam[None, :]


def schur_covariance(J, e_sizes):
    """Route (b).  J: dense, columns [E blocks of the sizes e_sizes | F]; E^T E is taken block-diagonal (only the diagonal blocks are
    read, as the eliminator reads them).  Returns a dict: cov (None when a factorisation failed), min_point_pivot, point_at (the E
    block), min_schur_pivot (-1.0 when the point stage already failed), schur_at."""
    ne = int(np.sum(e_sizes))
    E, F = J[:, :ne], J[:, ne:]
    out = {"cov": None, "min_point_pivot": np.inf, "point_at": -1, "min_schur_pivot": -1.0, "schur_at": -1}
    Cinv = np.zeros((ne, ne))
    ok, at = True, 0
    for p, sz in enumerate(e_sizes):
        Ep = E[:, at:at + sz]
        lam, G, piv, _ = scaled_cholesky(Ep.T @ Ep)
        if piv < out["min_point_pivot"]:
            out["min_point_pivot"], out["point_at"] = piv, p
        if G is None:
            ok = False
        else:
            Cinv[at:at + sz, at:at + sz] = inverse_from_scaled_factor(lam, G)
        at += sz
    if not e_sizes:
        out["min_point_pivot"] = 1.0
    if not ok:
        return out
    W = E.T @ F
    Y = Cinv @ W
    S = F.T @ F - W.T @ Y
    lam, G, piv, where = scaled_cholesky(S)
    out["min_schur_pivot"], out["schur_at"] = piv, where
    if G is None:
        return out
    Sinv = inverse_from_scaled_factor(lam, G)
    n = J.shape[1]
    cov = np.zeros((n, n))
    cov[ne:, ne:] = Sinv
    cov[:ne, ne:] = -Y @ Sinv
    cov[ne:, :ne] = cov[:ne, ne:].T
    cov[:ne, :ne] = Cinv + Y @ Sinv @ Y.T
    out["cov"] = cov
    return out


class Layout:
    """Blocks in state order (point q is q, camera c is num_points + c) -> their columns in the reduced program [free points | free
    cameras]; a constant block has none."""

    def __init__(self, num_points, num_cameras, point_column, camera_column, cw):
        self.np_, self.nc, self.cw = int(num_points), int(num_cameras), int(cw)
        self.pcol, self.ccol = np.asarray(point_column), np.asarray(camera_column)
        self.nfp = int(np.sum(self.pcol >= 0))
        self.nfc = int(np.sum(self.ccol >= 0))
        self.n = 3 * self.nfp + self.cw * self.nfc

    def size(self, block):
        return 3 if block < self.np_ else self.cw

    def columns(self, block):
        """The block's columns (an index array), or None for a constant block."""
        if block < self.np_:
            q = int(self.pcol[block])
            return None if q < 0 else np.arange(3 * q, 3 * q + 3)
        c = int(self.ccol[block - self.np_])
        return None if c < 0 else 3 * self.nfp + np.arange(self.cw * c, self.cw * c + self.cw)

    def e_sizes(self):
        return [3] * self.nfp

    def blocks(self, cov, pairs):
        """The requested blocks of a full matrix; a pair with a constant block is zeros (covariance_impl.cc:143-165)."""
        out = []
        for a, b in np.asarray(pairs).reshape(-1, 2):
            ra, rb = self.columns(int(a)), self.columns(int(b))
            if ra is None or rb is None:
                out.append(np.zeros((self.size(int(a)), self.size(int(b)))))
            else:
                out.append(cov[np.ix_(ra, rb)].copy())
        return out

    def scales(self, diag, pairs):
        """sqrt(Cov_ii Cov_jj) for every entry of every requested block (1 for a pair with a constant block: its entries are exact zeros)."""
        out = []
        for a, b in np.asarray(pairs).reshape(-1, 2):
            ra, rb = self.columns(int(a)), self.columns(int(b))
            if ra is None or rb is None:
                out.append(np.ones((self.size(int(a)), self.size(int(b)))))
            else:
                out.append(np.sqrt(np.outer(diag[ra], diag[rb])))
        return out


def correlation_deviation(blocks, reference_blocks, scales):
    """max |Delta_ij| / sqrt(Cov_ii Cov_jj) over every entry of every block."""
    worst = 0.0
    for b, r, s in zip(blocks, reference_blocks, scales):
        assert b.shape == r.shape == s.shape, (b.shape, r.shape, s.shape)
        worst = max(worst, float(np.max(np.abs(b - r) / s)))
    return worst


def perturbed(J, seed, sigma=1e-15):
    """Every Jacobian value times 1 + sigma N(0, 1): the method of test_gpu_frontend_matrix.EDGE_ILL_CONDITIONED."""
    rng = np.random.default_rng(seed)
    return J * (1.0 + sigma * rng.standard_normal(J.shape))
