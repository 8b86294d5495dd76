// bal_layout.h — the host-side index work of a BAL front-end handle (design/28_bal_layout.md): which rows the program keeps and in what
// order, where every Jacobian cell, step and state entry of a row lies, the flat block structure, and the lists cut from them: where every
// kernel of the front end reads and writes.  No HIP in it, the standard library alone (tests/test_bal_layout_cpu.py runs it under g++'s sanitizers).
#ifndef CERES_HIP_BAL_LAYOUT_H_
#define CERES_HIP_BAL_LAYOUT_H_

#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

namespace chip {

enum : int { kBalAngleAxis = 0, kBalQuaternion = 1, kBalQuaternionManifold = 2 };   // CERES_HIP_CAMERA_* (asserted in bal_frontend.inc)
inline bool bal_camera_model_known(int32_t m) { return m >= kBalAngleAxis && m <= kBalQuaternionManifold; }

// ---- one stable grouping of a list by key: a counting sort.  Keys lie in [0, n); an item with a negative key is in no group (place -1).
struct BalGrouping { std::vector<int32_t> ptr, perm, place; };   // group g: the items perm[ptr[g] .. ptr[g + 1]) in list order; place: perm's inverse
template <class Key>
BalGrouping bal_group_by(int64_t count, int32_t n, Key key) {
  BalGrouping G;
  G.ptr.assign(size_t(n) + 1, 0);
  for (int64_t i = 0; i < count; ++i) { const int32_t k = key(i); if (k >= 0) ++G.ptr[size_t(k) + 1]; }
  for (int32_t g = 0; g < n; ++g) G.ptr[size_t(g) + 1] += G.ptr[g];
  G.perm.resize(size_t(G.ptr[n])); G.place.assign(size_t(count), -1);
  std::vector<int32_t> fill(G.ptr.begin(), G.ptr.end() - 1);
  for (int64_t i = 0; i < count; ++i) { const int32_t k = key(i); if (k >= 0) G.perm[size_t(G.place[i] = fill[k]++)] = int32_t(i); }
  return G;
}
// out[e] = src[perm[e]], for records of `width` entries (2: pixels): through a permutation, or through a grouping — read in the list's order, one
// write stream per group; through perm the 5 M rows of Venice miss the cache at every item, +50 ms (profiles/bal_layout_gather_first_call.json)
template <class T>
std::vector<T> bal_gather(const std::vector<int32_t>& perm, const T* src, int width = 1) {
  std::vector<T> out(perm.size() * size_t(width));
  for (size_t e = 0; e < perm.size(); ++e)
    for (int j = 0; j < width; ++j) out[width * e + j] = src[size_t(width) * perm[e] + j];
  return out;
}
template <class T>
std::vector<T> bal_gather(const BalGrouping& G, const T* src, int width = 1) {
  std::vector<T> out(G.perm.size() * size_t(width));
  for (size_t i = 0; i < G.place.size(); ++i)
    for (int j = 0; j < width && G.place[i] >= 0; ++j) out[size_t(width) * G.place[i] + j] = src[width * i + j];
  return out;
}

// ---- Constant parameter blocks: SetParameterBlockConstant, and what Program::RemoveFixedBlocks (I/program.cc:309-410) and the Schur ordering
// (I/reorder_program.cc:278-340) make of the problem.
struct BalReduction {
  int32_t num_free_cameras = 0, num_free_points = 0;
  int64_t num_rows_e = 0;                    // rows with an E cell (a free point): they come first
  std::vector<int32_t> row_obs;              // kept row -> observation
  std::vector<int32_t> removed_obs;          // observations whose camera and point are both constant, in observation order
  std::vector<int32_t> camera_column, point_column;   // index among the free blocks, -1: constant
};

// "" or why the problem is refused.  A residual block whose parameter blocks are all constant is removed; the others keep the project's
// order — grouped by point, stable in observation order — with the rows of constant points behind all rows that have an E cell.
inline std::string bal_reduce(int32_t num_cameras, int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                              const int32_t* point_index, const uint8_t* camera_is_constant, const uint8_t* point_is_constant, BalReduction& R) {
  if (num_cameras <= 0 || num_points <= 0 || num_observations <= 0 || !camera_index || !point_index) return "bad arguments";
  if (num_observations > int64_t(INT32_MAX)) return "more than 2^31 observations";
  for (int64_t i = 0; i < num_observations; ++i)
    if (camera_index[i] < 0 || camera_index[i] >= num_cameras || point_index[i] < 0 || point_index[i] >= num_points)
      return "observation index out of range";
  R.camera_column.assign(size_t(num_cameras), -1);
  R.point_column.assign(size_t(num_points), -1);
  R.num_free_cameras = R.num_free_points = 0;
  for (int c = 0; c < num_cameras; ++c) if (!(camera_is_constant && camera_is_constant[c])) R.camera_column[c] = R.num_free_cameras++;
  for (int q = 0; q < num_points; ++q) if (!(point_is_constant && point_is_constant[q])) R.point_column[q] = R.num_free_points++;
  if (R.num_free_cameras == 0)
    return "every camera is constant: no F block is left (Ceres switches the linear solver there, LinearSolverForZeroEBlocks and its "
           "kin; this front end does not)";
  if (R.num_free_points == 0)
    return "every point is constant: no E block is left (Ceres switches the linear solver there, LinearSolverForZeroEBlocks; this front "
           "end does not)";
  R.row_obs.clear(); R.removed_obs.clear();
  std::vector<int32_t> tail;
  for (int64_t i = 0; i < num_observations; ++i) {
    const bool cf = R.camera_column[camera_index[i]] >= 0, pf = R.point_column[point_index[i]] >= 0;
    if (pf) R.row_obs.push_back(int32_t(i));
    else if (cf) tail.push_back(int32_t(i));
    else R.removed_obs.push_back(int32_t(i));
  }
  std::stable_sort(R.row_obs.begin(), R.row_obs.end(), [&](int32_t a, int32_t b) { return point_index[a] < point_index[b]; });
  R.num_rows_e = int64_t(R.row_obs.size());
  R.row_obs.insert(R.row_obs.end(), tail.begin(), tail.end());
  if (R.row_obs.empty()) return "no residual block is left: every observation has a constant camera and a constant point";
  return "";
}

// State offsets of the free blocks, points then cameras (BalFreeBlocks::block).  Empty column maps: every block is free.
inline std::vector<int64_t> bal_free_block_offsets(int32_t num_cameras, int32_t num_points, int cs, const std::vector<int32_t>& camera_column,
                                                   const std::vector<int32_t>& point_column) {
  std::vector<int64_t> fb;
  fb.reserve(size_t(num_points) + size_t(num_cameras));
  for (int q = 0; q < num_points; ++q) if (point_column.empty() || point_column[q] >= 0) fb.push_back(3 * int64_t(q));
  for (int c = 0; c < num_cameras; ++c) if (camera_column.empty() || camera_column[c] >= 0) fb.push_back(3 * int64_t(num_points) + cs * int64_t(c));
  return fb;
}

// ---- The layout of a handle: everything ceres_hip_bal_create* computes on the host before its uploads.
//   state (ambient)   [points 3 | cameras cs], n_a doubles: the caller's, whatever is constant
//   step (tangent)    [free points 3 | free cameras cw | groups 3], n_t doubles
//   Jacobian values   [E cells 6, of the rows with a free point: these rows come first | per row with a free camera an F cell 2 x cw];
//                     with shared intrinsics behind the E cells per row [pose cell 2 x 6, free cameras only | group cell 2 x 3]
struct BalLayout {
  int32_t camera_model = kBalAngleAxis, nc = 0, np = 0;
  int cs = 9, cw = 9;                         // state doubles / Jacobian columns per camera
  int intrinsics_mask = 0, n_groups = 0;      // bit k: coordinate 6 + k of every camera is constant; shared intrinsics: the groups, else 0
  std::vector<int32_t> group_first;           // a group's first camera
  bool has_const = false;                     // some camera or point is constant
  BalReduction red;                           // kept rows, removed observations, free columns (nfc, nfp, n_rows_e)
  int64_t n_a = 0, n_t = 0, n_rows = 0, n_rows_e = 0, n_rows_f = 0, n_values = 0;
  // per kept row: camera, point, pixel; value position of its F (pose) and group cell, -1: none; step offset of its camera, point, group, -1: constant; removed rows
  std::vector<int32_t> row_cam, row_pt, row_fpos, row_scam, row_spt, row_gpos, row_sgrp, rm_cam, rm_pt;
  std::vector<double> row_pixel, rm_pixel;
  std::vector<int32_t> f_row;                 // F cell (in row order) -> row
  // the flat ceres_hip_block_structure: column blocks are the free points, the free cameras (their poses), the groups
  std::vector<int32_t> row_size, row_pos, col_size, col_pos, row_ptr, cell_col, cell_pos;
  std::vector<int64_t> free_block;            // bal_free_block_offsets
  std::vector<int32_t> cam_pose, cam_group, cam_first;   // shared intrinsics, per camera: step offset of its pose (-1: constant) and group, first of its group?
  int nfc() const { return red.num_free_cameras; }   // free cameras / points
  int nfp() const { return red.num_free_points; }
};

// "" or the refusal (the text behind the entry point's name), checks in the entry points' old order.  The masks and camera_group may be NULL.
inline std::string bal_layout(int32_t camera_model, int32_t num_cameras, int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                              const int32_t* point_index, const double* observations, const uint8_t* camera_is_constant,
                              const uint8_t* point_is_constant, const uint8_t* camera_coordinate_is_constant, const int32_t* camera_group,
                              int32_t num_groups, BalLayout& L) {
  using std::to_string;
  if (!bal_camera_model_known(camera_model)) return "unknown camera_model " + to_string(camera_model);
  if (num_cameras <= 0 || num_points <= 0 || num_observations <= 0 || !camera_index || !point_index || !observations) return "bad arguments";
  L = BalLayout{};
  L.camera_model = camera_model; L.nc = num_cameras; L.np = num_points;
  const int cs = L.cs = camera_model == kBalAngleAxis ? 9 : 10;
  // Shared intrinsics (camera_group != NULL): every camera in exactly one group, every group id used; angle-axis cameras only
  const int ng = L.n_groups = camera_group ? num_groups : 0;
  if (camera_group) {
    if (camera_model != kBalAngleAxis) return "shared intrinsics are supported for the angle-axis camera only (camera_model " + to_string(camera_model) + ")";
    if (num_groups <= 0 || num_groups > num_cameras) return "num_groups " + to_string(num_groups) + " is not in [1, num_cameras = " + to_string(num_cameras) + "]";
    L.group_first.assign(size_t(num_groups), -1);
    for (int c = 0; c < num_cameras; ++c) {
      if (camera_group[c] < 0 || camera_group[c] >= num_groups)
        return "camera " + to_string(c) + " has group " + to_string(camera_group[c]) + ", not in [0, " + to_string(num_groups) + ")";
      if (L.group_first[camera_group[c]] < 0) L.group_first[camera_group[c]] = c;
    }
    for (int g = 0; g < num_groups; ++g)
      if (L.group_first[g] < 0) return "group " + to_string(g) + " has no camera (every id in [0, num_groups) must be used)";
  }
  // SubsetManifold on every camera (one mask of cs entries; NULL: none): the intrinsics f, k1, k2 of the angle-axis camera alone
  for (int j = 0; camera_coordinate_is_constant && j < cs; ++j) {
    if (!camera_coordinate_is_constant[j]) continue;
    if (camera_model != kBalAngleAxis) return "constant camera coordinates are supported for the angle-axis camera only (camera_model " + to_string(camera_model) + ")";
    if (j >= 6) { L.intrinsics_mask |= 1 << (j - 6); continue; }
    bool all = true;
    for (int k = 0; k < cs; ++k) all = all && camera_coordinate_is_constant[k] != 0;
    return all ? "every camera coordinate is constant: use constant cameras (camera_is_constant)"
               : "camera coordinate " + to_string(j) + " cannot be constant: only the intrinsics, coordinates 6 .. 8 (f, k1, k2)";
  }
  const int mask = L.intrinsics_mask, cw = L.cw = ng ? 6 : (camera_model == kBalQuaternion ? 10 : 9) - ((mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1));
  const int64_t per_obs = 6 + 2 * cw + (ng ? 6 : 0);   // Jacobian values per observation: 24, 26; 18 .. 22 with fixed intrinsics, 24 with shared ones
  if (num_observations * per_obs > int64_t(INT32_MAX))   // cell.position is an int in the reference too (I/block_structure.h:64)
    return "more than " + to_string(int64_t(INT32_MAX) / per_obs / 1000000) + " M observations do not fit 32-bit value positions";
  for (int c = 0; camera_is_constant && c < num_cameras; ++c) L.has_const = L.has_const || camera_is_constant[c] != 0;
  for (int q = 0; point_is_constant && q < num_points; ++q) L.has_const = L.has_const || point_is_constant[q] != 0;
  // RemoveFixedBlocks and the Schur ordering, behind the index-range check.  Nothing constant: rows by point, stable in observation order, every block free
  const BalReduction& R = L.red;
  const std::string why = bal_reduce(num_cameras, num_points, num_observations, camera_index, point_index, L.has_const ? camera_is_constant : nullptr,
                                     L.has_const ? point_is_constant : nullptr, L.red);
  if (!why.empty()) return why;
  const int nfc = L.nfc(), nfp = L.nfp();
  L.n_a = 3 * int64_t(num_points) + cs * int64_t(num_cameras);
  if ((L.has_const || ng || mask) && L.n_a > int64_t(INT32_MAX))   // (row_scam / row_spt / row_sgrp, the free blocks' users: 32-bit state offsets)
    return std::string("more than 2^31 state doubles with ") + (L.has_const ? "constant blocks" : ng ? "shared intrinsics" : "fixed intrinsics");
  L.n_t = 3 * int64_t(nfp) + cw * int64_t(nfc) + 3 * int64_t(ng);
  const int64_t no = L.n_rows = int64_t(R.row_obs.size()), ne = L.n_rows_e = R.num_rows_e;
  const int ncb = nfp + nfc + ng;
  L.col_size.resize(size_t(ncb)); L.col_pos.resize(size_t(ncb));
  for (int q = 0; q < nfp; ++q) { L.col_size[q] = 3; L.col_pos[q] = 3 * q; }
  for (int c = 0; c < nfc; ++c) { L.col_size[nfp + c] = cw; L.col_pos[nfp + c] = 3 * nfp + cw * c; }
  for (int g = 0; g < ng; ++g) { L.col_size[nfp + nfc + g] = 3; L.col_pos[nfp + nfc + g] = 3 * nfp + cw * nfc + 3 * g; }
  // step offsets of a camera's own columns (-1: constant) and of its group's
  auto cam_step = [&](int c) { const int cc = R.camera_column[c]; return cc >= 0 ? 3 * nfp + cw * cc : -1; };
  auto group_step = [&](int c) { return 3 * nfp + cw * nfc + 3 * camera_group[c]; };
  L.row_cam = bal_gather(R.row_obs, camera_index); L.row_pt = bal_gather(R.row_obs, point_index); L.row_pixel = bal_gather(R.row_obs, observations, 2);
  L.rm_cam = bal_gather(R.removed_obs, camera_index); L.rm_pt = bal_gather(R.removed_obs, point_index); L.rm_pixel = bal_gather(R.removed_obs, observations, 2);
  for (int64_t r = 0; r < no; ++r) if (R.camera_column[L.row_cam[r]] >= 0) L.f_row.push_back(int32_t(r));
  const int64_t nf = L.n_rows_f = int64_t(L.f_row.size());
  L.n_values = 6 * ne + 2 * cw * nf + (ng ? 6 * no : 0);
  L.row_size.assign(size_t(no), 2); L.row_ptr.resize(size_t(no) + 1);
  for (auto* v : {&L.row_pos, &L.row_fpos, &L.row_scam, &L.row_spt}) v->resize(size_t(no));
  L.row_gpos.resize(ng ? size_t(no) : 0); L.row_sgrp.resize(ng ? size_t(no) : 0);
  L.cell_col.reserve(size_t(ng ? 3 : 2) * size_t(no)); L.cell_pos.reserve(size_t(ng ? 3 : 2) * size_t(no));
  auto cell = [&](int col, int64_t pos) { L.cell_col.push_back(col); L.cell_pos.push_back(int32_t(pos)); return int32_t(pos); };
  int64_t next = 6 * ne;   // (shared intrinsics: a row's pose cell and group cell back to back, in column order)
  for (int64_t r = 0, f = 0; r < no; ++r) {
    const int cam = L.row_cam[r], pc = R.point_column[L.row_pt[r]], cc = R.camera_column[cam];
    L.row_pos[r] = int32_t(2 * r); L.row_ptr[r] = int32_t(L.cell_col.size());
    L.row_spt[r] = pc >= 0 ? 3 * pc : -1; L.row_scam[r] = cam_step(cam); L.row_fpos[r] = -1;
    if (pc >= 0) cell(pc, 6 * r);   // E cell (rows with one come first)
    if (ng) {
      if (cc >= 0) { L.row_fpos[r] = cell(nfp + cc, next); next += 12; }                  // pose cell
      L.row_gpos[r] = cell(nfp + nfc + camera_group[cam], next); next += 6;               // group cell
      L.row_sgrp[r] = group_step(cam);
    } else if (cc >= 0) {
      L.row_fpos[r] = cell(nfp + cc, 6 * ne + 2 * cw * f++);                              // F cell
    }
  }
  L.row_ptr[no] = int32_t(L.cell_col.size());
  L.free_block = bal_free_block_offsets(num_cameras, num_points, cs, R.camera_column, R.point_column);
  for (int c = 0; ng && c < num_cameras; ++c) {   // Plus' per-camera records (kernels_shared.hip)
    L.cam_pose.push_back(cam_step(c)); L.cam_group.push_back(group_step(c)); L.cam_first.push_back(L.group_first[camera_group[c]] == c);
  }
  return "";
}

// ---- The records cut from the solver's plan (plan.cc): the rows' camera / point / pixel in SLOT order — the tile-order evaluator's and the evaluating
// camera-major pass's.  Angle-axis cameras nine columns wide only; of constant blocks cameras alone (every row then has its E cell and lies in the tiles).
struct BalRecords {
  bool slots = false, camera_major = false;   // the slot-order lists exist; the plan's camera-major list covers the rows with an F cell
  std::vector<int32_t> slot_cam, slot_pt;     // per slot: its camera's RECORD, its point; 0 in the slots without a row
  // camera records: the free cameras in the solver's order, the constant ones behind them; per record its camera and its scale's step offset, -1: constant
  std::vector<int32_t> pack_cam, pack_scale;
  std::vector<int32_t> cm_pt;                 // point (and pixel) of every entry of the camera-major list
  std::vector<double> slot_pixel, cm_pixel;
};
inline BalRecords bal_records(const BalLayout& L, const std::vector<int32_t>& slot_bpos, const std::vector<int32_t>& cam_ptr,
                              const std::vector<int32_t>& cam_fpos) {
  BalRecords K;
  const int nfc = L.nfc();
  if (slot_bpos.empty() || L.camera_model != kBalAngleAxis || L.nfp() != L.np || L.intrinsics_mask || L.n_groups) return K;
  K.slots = true;
  std::vector<int32_t> rec_of(size_t(L.nc));
  K.pack_cam.resize(size_t(L.nc)); K.pack_scale.resize(size_t(L.nc));
  for (int c = 0, k = nfc; c < L.nc; ++c) {
    const int cc = L.red.camera_column[c];
    rec_of[c] = cc >= 0 ? cc : k++;
    K.pack_cam[rec_of[c]] = c;
    K.pack_scale[rec_of[c]] = cc >= 0 ? 3 * L.nfp() + 9 * cc : -1;
  }
  const size_t ns = slot_bpos.size();
  K.slot_cam.assign(ns, 0); K.slot_pt.assign(ns, 0); K.slot_pixel.assign(2 * ns, 0.0);
  for (size_t q = 0; q < ns; ++q) {
    if (slot_bpos[q] < 0) continue;
    const int64_t r = slot_bpos[q] >> 1;
    K.slot_cam[q] = rec_of[L.row_cam[r]]; K.slot_pt[q] = L.row_pt[r];
    K.slot_pixel[2 * q] = L.row_pixel[2 * r]; K.slot_pixel[2 * q + 1] = L.row_pixel[2 * r + 1];
  }
  // camera-major entry -> its row (through the F cell's position) -> point, pixel: the lists of the free cameras
  const int64_t nf = L.n_rows_f;
  if (cam_ptr.size() != size_t(nfc) + 1 || cam_ptr[nfc] != nf || (L.has_const ? cam_fpos.size() < size_t(nf) : cam_fpos.size() != size_t(L.n_rows))) return K;
  K.camera_major = true;
  std::vector<int32_t> rows(static_cast<size_t>(nf));
  for (int64_t q = 0; q < nf; ++q) rows[q] = L.f_row[(int64_t(cam_fpos[q]) - 6 * L.n_rows_e) / 18];
  K.cm_pt = bal_gather(rows, L.row_pt.data()); K.cm_pixel = bal_gather(rows, L.row_pixel.data(), 2);
  return K;
}

}  // namespace chip

#endif  // CERES_HIP_BAL_LAYOUT_H_
