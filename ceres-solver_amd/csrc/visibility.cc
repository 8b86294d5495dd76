// visibility.cc — host analysis of the CLUSTER_JACOBI preconditioner (no HIP): the visibility graph of the F blocks, canonical-views
// and single-linkage clustering, the flattened membership, the scalar layout of the cluster factors.  See common.h for what is
// restated and for the order this file pins where the reference walks hash sets.
//
// The CPU tests compare the clustering bit-for-bit with a Python restatement that performs the same IEEE operations in the same
// order: this file is compiled without floating-point contraction (build.py), and nothing here may be re-associated.
#include <algorithm>
#include <cmath>
#include <limits>

#include "common.h"

namespace chip {

// ComputeVisibility + CreateSchurComplementGraph, I/visibility.cc:49-145.  Visibility of F block f: the E blocks of the rows whose
// first cell is an E cell and that hold a cell of f.  Edge (i, j) = shared E blocks / sqrt(|vis i| |vis j|), the product formed in
// integers and converted once, as the reference does; self edges weigh 1.
void BuildVisibilityGraph(const HostStructure& h, VisibilityGraph* g) {
  const int nf = h.ncb - h.nelim;
  // camera -> sorted, distinct E blocks
  std::vector<std::vector<int32_t>> vis(nf);
  for (int i = 0; i < h.nrb; ++i) {
    const int e = h.row_e_block[i];
    if (e < 0) continue;
    for (int k = h.rptr[i] + 1; k < h.rptr[i + 1]; ++k) vis[h.ccol[k] - h.nelim].push_back(e);
  }
  for (auto& v : vis) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
  }
  // E block -> cameras, ascending
  std::vector<int64_t> iptr(size_t(h.nelim) + 1, 0);
  for (int c = 0; c < nf; ++c) for (int e : vis[c]) ++iptr[e + 1];
  for (int e = 0; e < h.nelim; ++e) iptr[e + 1] += iptr[e];
  std::vector<int32_t> icam(static_cast<size_t>(iptr[h.nelim]), 0);
  {
    std::vector<int64_t> cur(iptr.begin(), iptr.end() - 1);
    for (int c = 0; c < nf; ++c) for (int e : vis[c]) icam[cur[e]++] = c;
  }
  // shared counts per camera i with the cameras j > i, through a dense counter
  std::vector<std::vector<std::pair<int32_t, double>>> upper(nf);   // (j, weight), j > i
  std::vector<int32_t> count(nf, 0), touched;
  for (int i = 0; i < nf; ++i) {
    touched.clear();
    for (int e : vis[i])
      for (int64_t q = iptr[e]; q < iptr[e + 1]; ++q) {
        const int j = icam[q];
        if (j <= i) continue;
        if (count[j]++ == 0) touched.push_back(j);
      }
    std::sort(touched.begin(), touched.end());
    for (int j : touched) {
      const double w = static_cast<double>(count[j]) / std::sqrt(static_cast<double>(vis[i].size() * vis[j].size()));
      upper[i].push_back({j, w});
      count[j] = 0;
    }
  }
  // symmetric adjacency, ascending neighbours, self edge included
  std::vector<int64_t> deg(size_t(nf) + 1, 0);
  for (int i = 0; i < nf; ++i) {
    deg[i + 1] += 1 + int64_t(upper[i].size());
    for (auto& jw : upper[i]) ++deg[jw.first + 1];
  }
  g->ptr.assign(size_t(nf) + 1, 0);
  for (int i = 0; i < nf; ++i) g->ptr[i + 1] = g->ptr[i] + deg[i + 1];
  g->nbr.assign(size_t(g->ptr[nf]), 0);
  g->weight.assign(size_t(g->ptr[nf]), 0.0);
  std::vector<int64_t> cur(g->ptr.begin(), g->ptr.end() - 1);
  // rows are filled in ascending i: the entries (j < i) of row i arrive first and in ascending j, then the self edge, then j > i
  for (int i = 0; i < nf; ++i) {
    g->nbr[cur[i]] = i; g->weight[cur[i]] = 1.0; ++cur[i];
    for (auto& jw : upper[i]) {
      g->nbr[cur[i]] = jw.first; g->weight[cur[i]] = jw.second; ++cur[i];
      g->nbr[cur[jw.first]] = i; g->weight[cur[jw.first]] = jw.second; ++cur[jw.first];
    }
  }
}

// CanonicalViewsClustering::ComputeClustering, I/canonical_views_clustering.cc:94-196.  A vertex whose weight is NaN is not a valid
// view (FindValidViews).  The score of a candidate is accumulated in the reference's order: view score, the gains over its neighbours
// (ascending index here), minus the size penalty, minus the similarity terms of the centres in the order they were chosen.
void CanonicalViews(const VisibilityGraph& g, const CanonicalViewsOptions& o, const double* vertex_weight, std::vector<int32_t>* centers,
                    std::vector<int32_t>* view_center) {
  const int n = int(g.ptr.size()) - 1;
  centers->clear();
  view_center->assign(n, -1);
  std::vector<double> similarity(n, 0.0);   // view_to_canonical_view_similarity_, default 0
  std::vector<char> valid(n, 1);
  int num_valid = 0;
  for (int v = 0; v < n; ++v) {
    const double w = vertex_weight ? vertex_weight[v] : 1.0;
    valid[v] = !(w != w);
    num_valid += valid[v];
  }
  auto edge_weight = [&](int a, int b) {
    const int32_t* first = g.nbr.data() + g.ptr[a];
    const int32_t* last = g.nbr.data() + g.ptr[a + 1];
    const int32_t* it = std::lower_bound(first, last, b);
    return (it != last && *it == b) ? g.weight[it - g.nbr.data()] : 0.0;
  };
  while (num_valid > 0) {
    double best_difference = -std::numeric_limits<double>::max();
    int best_view = 0;
    for (int v = 0; v < n; ++v) {
      if (!valid[v]) continue;
      double difference = o.view_score_weight * (vertex_weight ? vertex_weight[v] : 1.0);
      for (int64_t q = g.ptr[v]; q < g.ptr[v + 1]; ++q) {
        const double old_similarity = similarity[g.nbr[q]];
        const double new_similarity = g.weight[q];
        if (new_similarity > old_similarity) difference += new_similarity - old_similarity;
      }
      difference -= o.size_penalty_weight;
      for (int c : *centers) {
        const double term = o.similarity_penalty_weight * edge_weight(c, v);
        difference -= term;
      }
      if (difference > best_difference) { best_difference = difference; best_view = v; }
    }
    if (best_difference <= 0 && int(centers->size()) >= o.min_views) break;
    const int id = int(centers->size());
    centers->push_back(best_view);
    valid[best_view] = 0;
    --num_valid;
    for (int64_t q = g.ptr[best_view]; q < g.ptr[best_view + 1]; ++q) {   // UpdateCanonicalViewAssignments
      const int u = g.nbr[q];
      if (g.weight[q] > similarity[u]) { (*view_center)[u] = id; similarity[u] = g.weight[q]; }
    }
  }
}

namespace {
// clusters numbered by ascending first member; returns their number
int RenumberByFirstMember(std::vector<int32_t>* membership) {
  std::vector<int32_t> id;
  int next = 0;
  for (int32_t& m : *membership) {
    if (m >= int(id.size())) id.resize(size_t(m) + 1, -1);
    if (id[m] < 0) id[m] = next++;
    m = id[m];
  }
  return next;
}
}  // namespace

std::string ClusterCameras(const HostStructure& h, int clustering_type, std::vector<int32_t>* membership, int* num_clusters) {
  const int nf = h.ncb - h.nelim;
  if (nf <= 0) return "CLUSTER_JACOBI needs at least one F block";
  if (clustering_type != CERES_HIP_CANONICAL_VIEWS && clustering_type != CERES_HIP_SINGLE_LINKAGE)
    return "visibility_clustering_type must be CANONICAL_VIEWS (0) or SINGLE_LINKAGE (1)";
  VisibilityGraph g;
  BuildVisibilityGraph(h, &g);
  membership->assign(nf, 0);
  if (clustering_type == CERES_HIP_CANONICAL_VIEWS) {
    std::vector<int32_t> centers, view_center;
    CanonicalViews(g, CanonicalViewsOptions(), nullptr, &centers, &view_center);
    const int nc = int(centers.size());   // > 0: the first round always takes a centre (min_views = 3)
    // FlattenMembershipMap (I/visibility_based_preconditioner.cc:540-576): a view no centre claimed goes to camera % num_clusters
    for (int v = 0; v < nf; ++v) (*membership)[v] = view_center[v] >= 0 ? view_center[v] : v % nc;
  } else {
    // ComputeSingleLinkageClustering (I/single_linkage_clustering.cc:41-91): union-find over the edges of at least 0.9, the smaller
    // root wins — the components do not depend on the order the edges are met in
    constexpr double kMinSimilarity = 0.9;
    std::vector<int32_t> parent(nf);
    for (int v = 0; v < nf; ++v) parent[v] = v;
    auto find = [&](int v) {
      int r = v;
      while (parent[r] != r) r = parent[r];
      while (parent[v] != r) { const int nx = parent[v]; parent[v] = r; v = nx; }
      return r;
    };
    for (int v1 = 0; v1 < nf; ++v1)
      for (int64_t q = g.ptr[v1]; q < g.ptr[v1 + 1]; ++q) {
        const int v2 = g.nbr[q];
        if (v1 > v2 || g.weight[q] < kMinSimilarity) continue;
        const int c1 = find(v1), c2 = find(v2);
        if (c1 == c2) continue;
        if (c1 < c2) parent[c2] = c1; else parent[c1] = c2;
      }
    for (int v = 0; v < nf; ++v) (*membership)[v] = find(v);
  }
  *num_clusters = RenumberByFirstMember(membership);
  return "";
}

void BuildClusterLayout(const HostStructure& h, const std::vector<int32_t>& membership, int num_clusters, ClusterLayoutHost* out) {
  ClusterLayoutHost& L = *out;
  L = ClusterLayoutHost();
  const int nf = h.ncb - h.nelim;
  L.num_clusters = num_clusters;
  L.block_cluster = membership;
  L.block_loc.assign(nf, 0);
  std::vector<int32_t> dim(num_clusters, 0);
  for (int f = 0; f < nf; ++f) { L.block_loc[f] = dim[membership[f]]; dim[membership[f]] += h.csz[h.nelim + f]; }
  L.cl_off.assign(size_t(num_clusters) + 1, 0);
  L.mat_off.assign(size_t(num_clusters) + 1, 0);
  for (int k = 0; k < num_clusters; ++k) {
    L.cl_off[k + 1] = L.cl_off[k] + dim[k];
    L.mat_off[k + 1] = L.mat_off[k] + int64_t(dim[k]) * dim[k];
    L.largest = std::max(L.largest, int(dim[k]));
  }
  L.perm.assign(size_t(h.num_cols_f), 0);
  for (int f = 0; f < nf; ++f) {
    const int j = h.nelim + f;
    for (int a = 0; a < h.csz[j]; ++a) L.perm[L.cl_off[membership[f]] + L.block_loc[f] + a] = h.cpos[j] - h.num_cols_e + a;
  }
}

}  // namespace chip
