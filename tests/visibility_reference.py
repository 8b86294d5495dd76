"""The host analysis of the CLUSTER_JACOBI preconditioner restated in Python, and the preconditioner itself in float64 numpy.

Restates ComputeVisibility / CreateSchurComplementGraph (internal/ceres/visibility.cc), ComputeCanonicalViewsClustering
(internal/ceres/canonical_views_clustering.cc), ComputeSingleLinkageClustering (internal/ceres/single_linkage_clustering.cc) and
VisibilityBasedPreconditioner::ClusterCameras / FlattenMembershipMap / ComputeBlockPairsInPreconditioner
(internal/ceres/visibility_based_preconditioner.cc) from the block structure alone.  Python floats are IEEE doubles and math.sqrt is
correctly rounded, so the same operations in the same order give the same bits as csrc/visibility.cc.

What the reference leaves to the iteration order of its hash sets is pinned as include/ceres_hip.h states it: candidates are scanned and
a candidate's neighbours summed in ascending index, a strictly greater score replaces the best (the lowest index wins a tie), and
clusters are numbered by ascending first member.  `ties` counts the comparisons in which a candidate scored exactly the running best.
"""
import math

import numpy as np

CANONICAL_VIEWS, SINGLE_LINKAGE = 0, 1
SIZE_PENALTY, SIMILARITY_PENALTY, MIN_VIEWS, VIEW_SCORE_WEIGHT = 3.0, 0.0, 3, 0.0   # visibility_based_preconditioner.cc:65-66, the options' defaults
SINGLE_LINKAGE_MIN_SIMILARITY = 0.9


def visibility(bs, nelim):
    """Per F block: the set of E blocks of the rows (first cell an E cell) it has a cell in."""
    nf = int(bs.num_col_blocks) - nelim
    vis = [set() for _ in range(nf)]
    ptr, col = bs.row_cell_ptr, bs.cell_col_block
    for r in range(int(bs.num_row_blocks)):
        a, b = int(ptr[r]), int(ptr[r + 1])
        if a == b:
            continue
        e = int(col[a])
        if e >= nelim:
            continue
        for k in range(a + 1, b):
            vis[int(col[k]) - nelim].add(e)
    return vis


def schur_complement_graph(vis):
    """neighbours[v] = {u: weight}, self edges of weight 1; (i, j) = shared / sqrt(|vis i| |vis j|), the product formed in integers."""
    n = len(vis)
    inverse = {}
    for c, s in enumerate(vis):
        for pt in s:
            inverse.setdefault(pt, []).append(c)
    count = {}
    for cams in inverse.values():
        cams = sorted(cams)
        for i in range(len(cams)):
            for j in range(i + 1, len(cams)):
                count[(cams[i], cams[j])] = count.get((cams[i], cams[j]), 0) + 1
    nb = [{i: 1.0} for i in range(n)]
    for (i, j), c in count.items():
        w = float(c) / math.sqrt(float(len(vis[i]) * len(vis[j])))
        nb[i][j] = w
        nb[j][i] = w
    return nb


def graph_from_edges(num_vertices, edges, self_edges=False):
    """A graph given as data (tests/golden/visibility_known_answers.json): edges = [[u, v, weight], ...]."""
    nb = [dict() for _ in range(num_vertices)]
    if self_edges:
        for i in range(num_vertices):
            nb[i][i] = 1.0
    for u, v, w in edges:
        nb[int(u)][int(v)] = float(w)
        nb[int(v)][int(u)] = float(w)
    return nb


def canonical_views(nb, size_penalty=SIZE_PENALTY, similarity_penalty=SIMILARITY_PENALTY, min_views=MIN_VIEWS,
                    view_score_weight=VIEW_SCORE_WEIGHT, vertex_weights=None):
    """(centers in the order chosen, {view: index of its centre}, ties)."""
    n = len(nb)
    weight = [1.0] * n if vertex_weights is None else [float(w) for w in vertex_weights]
    valid = [not math.isnan(w) for w in weight]
    centers, to_center, similarity, ties = [], {}, {}, 0
    order = [sorted(d.items()) for d in nb]
    while any(valid):
        best, best_view = -1.7976931348623157e308, 0   # -std::numeric_limits<double>::max()
        for v in range(n):
            if not valid[v]:
                continue
            d = view_score_weight * weight[v]
            for u, w in order[v]:
                old = similarity.get(u, 0.0)
                if w > old:
                    d += w - old
            d -= size_penalty
            for c in centers:
                d -= similarity_penalty * nb[c].get(v, 0.0)
            if d > best:
                best, best_view = d, v
            elif d == best:
                ties += 1
        if best <= 0 and len(centers) >= min_views:
            break
        cid = len(centers)
        centers.append(best_view)
        valid[best_view] = False
        for u, w in order[best_view]:
            if w > similarity.get(u, 0.0):
                to_center[u] = cid
                similarity[u] = w
    return centers, to_center, ties


def single_linkage(nb, min_similarity=SINGLE_LINKAGE_MIN_SIMILARITY):
    """Root (smallest member) of every vertex's component over the edges of at least min_similarity."""
    n = len(nb)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in range(n):
        for j, w in sorted(nb[i].items()):
            if i > j or w < min_similarity:
                continue
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return [find(i) for i in range(n)]


def renumber(raw):
    """Cluster ids by ascending first member."""
    ids, out = {}, []
    for m in raw:
        if m not in ids:
            ids[m] = len(ids)
        out.append(ids[m])
    return np.array(out, dtype=np.int32), len(ids)


def cluster_cameras(bs, nelim, clustering_type, return_ties=False):
    """(membership of every F block, number of clusters) — what ceres_hip_debug_cluster_cameras returns."""
    nb = schur_complement_graph(visibility(bs, nelim))
    ties = 0
    if clustering_type == CANONICAL_VIEWS:
        centers, to_center, ties = canonical_views(nb)
        raw = [to_center[v] if v in to_center else v % len(centers) for v in range(len(nb))]   # FlattenMembershipMap
    elif clustering_type == SINGLE_LINKAGE:
        raw = single_linkage(nb)
    else:
        raise ValueError(clustering_type)
    membership, n = renumber(raw)
    return (membership, n, ties) if return_ties else (membership, n)


def block_pairs(bs, nelim, membership):
    """ComputeBlockPairsInPreconditioner: the sorted pairs (i <= j) of F blocks that share a chunk or an E-free row and a cluster; every
    (i, i)."""
    nf = int(bs.num_col_blocks) - nelim
    pairs = {(i, i) for i in range(nf)}
    ptr, col = bs.row_cell_ptr, bs.cell_col_block
    chunks = {}
    for r in range(int(bs.num_row_blocks)):
        a, b = int(ptr[r]), int(ptr[r + 1])
        if a == b:
            continue
        e = int(col[a])
        if e < nelim:
            chunks.setdefault(e, set()).update(int(col[k]) - nelim for k in range(a + 1, b))
        else:
            fs = [int(col[k]) - nelim for k in range(a, b)]
            for i in fs:
                for j in fs:
                    if i <= j and membership[i] == membership[j]:
                        pairs.add((i, j))
    for fs in chunks.values():
        fs = sorted(fs)
        for x in range(len(fs)):
            for y in range(x + 1, len(fs)):
                if membership[fs[x]] == membership[fs[y]]:
                    pairs.add((fs[x], fs[y]))
    return sorted(pairs)


def cluster_matrices(ref, membership):
    """[(scalar indices into F space, dense M_k)] per cluster: S restricted to the cluster's F blocks, from SchurReference's ftf, ef and
    ete_inv (no dense E) plus the off-diagonal F_i^T F_j of rows that hold both blocks."""
    bs, nelim = ref.bs, ref.nelim
    membership = np.asarray(membership)
    nf_blocks = len(ref.f_sizes)
    clusters = [np.flatnonzero(membership == k) for k in range(int(membership.max()) + 1)] if nf_blocks else []
    loc = np.zeros(nf_blocks, dtype=np.int64)
    mats, idx = [], []
    for members in clusters:
        o = 0
        ii = []
        for f in members:
            loc[f] = o
            o += int(ref.f_sizes[f])
            ii.append(np.arange(int(ref.f_pos[f]), int(ref.f_pos[f]) + int(ref.f_sizes[f])))
        M = np.zeros((o, o))
        for f in members:
            n = int(ref.f_sizes[f])
            M[loc[f]:loc[f] + n, loc[f]:loc[f] + n] = ref.ftf[f]
        mats.append(M)
        idx.append(np.concatenate(ii) if ii else np.zeros(0, np.int64))
    # rows holding two F blocks of one cluster: F_i^T F_j off the diagonal
    ptr, col = bs.row_cell_ptr, bs.cell_col_block
    for r in range(int(bs.num_row_blocks)):
        a, b = int(ptr[r]), int(ptr[r + 1])
        rs = int(bs.row_block_size[r])
        cells = []
        for k in range(a, b):
            c = int(col[k])
            if c >= nelim:
                n = int(ref.f_sizes[c - nelim])
                vp = int(bs.cell_value_pos[k])
                cells.append((c - nelim, ref.values[vp:vp + rs * n].reshape(rs, n)))
        for x in range(len(cells)):
            for y in range(len(cells)):
                i, Bi = cells[x]
                j, Bj = cells[y]
                if i == j or membership[i] != membership[j]:
                    continue
                M = mats[membership[i]]
                M[loc[i]:loc[i] + Bi.shape[1], loc[j]:loc[j] + Bj.shape[1]] += Bi.T @ Bj
    # minus sum over points of (E_p^T F_i)^T M_p^-1 (E_p^T F_j)
    by_point = {}
    for (pt, c), W in ref.ef.items():
        by_point.setdefault(pt, []).append((c, W))
    for pt, lst in by_point.items():
        inv = ref.ete_inv[pt]
        for i, Wi in lst:
            for j, Wj in lst:
                if membership[i] != membership[j]:
                    continue
                M = mats[membership[i]]
                M[loc[i]:loc[i] + Wi.shape[1], loc[j]:loc[j] + Wj.shape[1]] -= Wi.T @ inv @ Wj
    return list(zip(idx, mats))


def cluster_jacobi(ref, membership):
    """A callable r -> M^-1 r (numpy's Cholesky per cluster), with .clusters = [(indices, M_k)] and .apply_M(z) = M z."""
    clusters = cluster_matrices(ref, membership)
    factors = [np.linalg.cholesky(0.5 * (M + M.T)) for _, M in clusters]

    def apply(r):
        z = np.zeros_like(r)
        for (ii, _), L in zip(clusters, factors):
            y = np.linalg.solve(L, r[ii])
            z[ii] = np.linalg.solve(L.T, y)
        return z

    def apply_M(z):
        out = np.zeros_like(z)
        for ii, M in clusters:
            out[ii] = 0.5 * (M + M.T) @ z[ii]
        return out
    apply.clusters = clusters
    apply.apply_M = apply_M
    return apply
