"""The host-side layout of a BAL front-end handle (ceres-solver_amd/csrc/bal_layout.h, design/28_bal_layout.md): which rows are kept and in
what order, where every cell, step and state entry lies, the block structure, the records cut from the plan, the grouping — and every
refusal with its text.  The header has no HIP in it: it is compiled with g++ into a stand-alone program and run, once plainly and once
with the address and undefined-behaviour sanitizers (nothing is preloaded: the program has its own main).

One scene, the smallest that separates the cases: 3 cameras, 4 points, 7 observations.  The expected values are literals, derived by hand
from the rules the header states."""
import os
import subprocess
import textwrap

import pytest

from conftest import ROOT

CHECK = r"""
    #include <cstdio>
    #include <initializer_list>
    #include "bal_layout.h"

    using namespace chip;
    #define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

    template <class T>
    bool eq(const std::vector<T>& v, std::initializer_list<T> want) { return v == std::vector<T>(want); }
    typedef std::vector<int32_t> Ints;

    const int32_t kCam[7] = {0, 1, 2, 0, 1, 2, 1}, kPt[7] = {2, 0, 2, 1, 3, 0, 2};
    const double kPixel[14] = {0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5, 10.5, 11.5, 12.5, 13.5};   // observation i: (2 i + .5, 2 i + 1.5)

    // the scene with these masks / groups, the camera and point counts its own unless given
    std::string lay(BalLayout& L, int32_t model, const uint8_t* cam_const = nullptr, const uint8_t* pt_const = nullptr, const uint8_t* coord_const = nullptr,
                    const int32_t* group = nullptr, int32_t num_groups = 0, int32_t nc = 3, int32_t np = 4) {
      return bal_layout(model, nc, np, 7, kCam, kPt, kPixel, cam_const, pt_const, coord_const, group, num_groups, L);
    }

    int main() {
      BalLayout L;
      // ---- plain angle-axis: rows grouped by point, stable in observation order
      EXPECT(lay(L, kBalAngleAxis) == "");
      EXPECT(eq(L.red.row_obs, {1, 5, 3, 0, 2, 6, 4}) && L.red.removed_obs.empty() && !L.has_const);
      EXPECT(L.cs == 9 && L.cw == 9 && L.intrinsics_mask == 0 && L.n_groups == 0 && L.nfc() == 3 && L.nfp() == 4);
      EXPECT(L.n_rows == 7 && L.n_rows_e == 7 && L.n_rows_f == 7 && L.n_a == 39 && L.n_t == 39 && L.n_values == 168);
      EXPECT(eq(L.row_cam, {1, 2, 0, 0, 2, 1, 1}) && eq(L.row_pt, {0, 0, 1, 2, 2, 2, 3}));
      for (int r = 0; r < 7; ++r) {
        EXPECT(L.row_pixel[2 * r] == 2 * L.red.row_obs[r] + .5 && L.row_pixel[2 * r + 1] == 2 * L.red.row_obs[r] + 1.5);
        EXPECT(L.row_fpos[r] == 42 + 18 * r && L.f_row[r] == r && L.row_spt[r] == 3 * L.row_pt[r] && L.row_scam[r] == 12 + 9 * L.row_cam[r]);
        EXPECT(L.row_size[r] == 2 && L.row_pos[r] == 2 * r && L.row_ptr[r] == 2 * r);   // 2 cells per row: E at 6 r, F at 42 + 18 r
        EXPECT(L.cell_col[2 * r] == L.row_pt[r] && L.cell_pos[2 * r] == 6 * r && L.cell_col[2 * r + 1] == 4 + L.row_cam[r] && L.cell_pos[2 * r + 1] == 42 + 18 * r);
      }
      EXPECT(L.row_ptr[7] == 14 && L.row_gpos.empty() && L.row_sgrp.empty() && L.rm_cam.empty() && L.cam_pose.empty());
      EXPECT(eq(L.col_size, {3, 3, 3, 3, 9, 9, 9}) && eq(L.col_pos, {0, 3, 6, 9, 12, 21, 30}));   // 7 column blocks
      EXPECT(eq<int64_t>(L.free_block, {0, 3, 6, 9, 12, 21, 30}));
      EXPECT(eq<int64_t>(bal_free_block_offsets(3, 4, 9, Ints(), Ints()), {0, 3, 6, 9, 12, 21, 30}));   // no maps: every block
      {   // the records: slots in any order with padding; the camera-major list in the plan's order (camera 0: rows 2 3, 1: 0 5 6, 2: 1 4)
        const BalRecords K = bal_records(L, Ints{12, -1, 0, 2, 4, 6, 8, 10}, Ints{0, 2, 5, 7}, Ints{78, 96, 42, 132, 150, 60, 114});
        EXPECT(K.slots && eq(K.slot_cam, {1, 0, 1, 2, 0, 0, 2, 1}) && eq(K.slot_pt, {3, 0, 0, 0, 1, 2, 2, 2}));
        EXPECT(K.slot_pixel[0] == 8.5 && K.slot_pixel[1] == 9.5 && K.slot_pixel[2] == 0.0 && K.slot_pixel[3] == 0.0 && K.slot_pixel[4] == 2.5);
        EXPECT(eq(K.pack_cam, {0, 1, 2}) && eq(K.pack_scale, {12, 21, 30}));   // the identity without constants
        EXPECT(K.camera_major && eq(K.cm_pt, {1, 2, 0, 2, 3, 0, 2}) && K.cm_pixel[0] == 6.5 && K.cm_pixel[13] == 5.5);
        EXPECT(!bal_records(L, Ints(), Ints{0, 2, 5, 7}, Ints(7, 42)).slots);                     // no plan, no records
        EXPECT(!bal_records(L, Ints{0}, Ints{0, 2, 5, 7}, Ints(6, 42)).camera_major);             // a camera-major list that is not the rows'
        EXPECT(!bal_records(L, Ints{0}, Ints{0, 2, 5, 6}, Ints(7, 42)).camera_major);
      }
      // ---- the quaternion cameras: ten state doubles; ten columns (Euclidean) or nine (manifold)
      EXPECT(lay(L, kBalQuaternion) == "");
      EXPECT(L.cs == 10 && L.cw == 10 && L.n_a == 42 && L.n_t == 42 && L.n_values == 182 && L.row_fpos[6] == 42 + 20 * 6);
      EXPECT(!bal_records(L, Ints{0}, Ints{0, 2, 5, 7}, Ints(7, 42)).slots);   // the tile evaluator is angle-axis
      EXPECT(lay(L, kBalQuaternionManifold) == "");
      EXPECT(L.cs == 10 && L.cw == 9 && L.n_a == 42 && L.n_t == 39 && L.n_values == 168);
      // ---- camera 0 and point 2 constant: observation 0 is removed, the two rows of the constant point trail
      const uint8_t cam0[3] = {1, 0, 0}, pt2[4] = {0, 0, 1, 0};
      EXPECT(lay(L, kBalAngleAxis, cam0, pt2) == "");
      EXPECT(L.has_const && eq(L.red.row_obs, {1, 5, 3, 4, 2, 6}) && eq(L.red.removed_obs, {0}));
      EXPECT(eq(L.red.camera_column, {-1, 0, 1}) && eq(L.red.point_column, {0, 1, -1, 2}));
      EXPECT(L.nfc() == 2 && L.nfp() == 3 && L.n_rows == 6 && L.n_rows_e == 4 && L.n_rows_f == 5 && L.n_a == 39 && L.n_t == 27 && L.n_values == 114);
      EXPECT(eq(L.row_cam, {1, 2, 0, 1, 2, 1}) && eq(L.row_pt, {0, 0, 1, 3, 2, 2}));
      EXPECT(eq(L.row_fpos, {24, 42, -1, 60, 78, 96}) && eq(L.f_row, {0, 1, 3, 4, 5}));
      EXPECT(eq(L.row_spt, {0, 0, 3, 6, -1, -1}) && eq(L.row_scam, {9, 18, -1, 9, 18, 9}));
      EXPECT(eq<int64_t>(L.free_block, {0, 3, 9, 21, 30}));
      EXPECT(eq<int64_t>(bal_free_block_offsets(3, 4, 9, L.red.camera_column, L.red.point_column), {0, 3, 9, 21, 30}));
      EXPECT(eq(L.rm_cam, {0}) && eq(L.rm_pt, {2}) && L.rm_pixel.size() == 2 && L.rm_pixel[0] == 0.5 && L.rm_pixel[1] == 1.5);
      EXPECT(eq(L.col_size, {3, 3, 3, 9, 9}) && eq(L.col_pos, {0, 3, 6, 9, 18}));
      EXPECT(eq(L.row_ptr, {0, 2, 4, 5, 7, 8, 9}));   // E + F, E + F, E, E + F, F, F
      EXPECT(eq(L.cell_col, {0, 3, 0, 4, 1, 2, 3, 4, 3}) && eq(L.cell_pos, {0, 24, 6, 42, 12, 18, 60, 78, 96}));
      // (a constant point leaves rows outside the tiles: no records, whatever the plan)
      EXPECT(!bal_records(L, Ints{0, 2, 4, 6}, Ints{0, 3, 5}, Ints{24, 60, 96, 42, 78}).slots);
      // ---- camera 0 constant alone: the records exist — cameras 1, 2 first, camera 0 behind them, without a scale
      EXPECT(lay(L, kBalAngleAxis, cam0) == "");
      EXPECT(L.has_const && L.n_rows == 7 && L.n_rows_e == 7 && L.n_rows_f == 5 && L.n_t == 30 && L.n_values == 132);
      EXPECT(eq(L.row_fpos, {42, 60, -1, -1, 78, 96, 114}) && eq(L.f_row, {0, 1, 4, 5, 6}));
      {
        const BalRecords K = bal_records(L, Ints{0, 2, -1, 4, 6, 8, 10, 12}, Ints{0, 3, 5}, Ints{42, 96, 114, 60, 78});
        EXPECT(K.slots && eq(K.pack_cam, {1, 2, 0}) && eq(K.pack_scale, {12, 21, -1}));
        EXPECT(eq(K.slot_cam, {0, 1, 0, 2, 2, 1, 0, 0}) && eq(K.slot_pt, {0, 0, 0, 1, 2, 2, 2, 3}));
        EXPECT(K.camera_major && eq(K.cm_pt, {0, 2, 3, 0, 2}) && K.cm_pixel[2] == 12.5 && K.cm_pixel[9] == 5.5);
      }
      // ---- coordinates 6 and 8 of every camera constant: the mask is 5, seven columns
      const uint8_t c68[9] = {0, 0, 0, 0, 0, 0, 1, 0, 1};
      EXPECT(lay(L, kBalAngleAxis, nullptr, nullptr, c68) == "");
      EXPECT(L.intrinsics_mask == 5 && L.cs == 9 && L.cw == 7 && !L.has_const && L.n_a == 39 && L.n_t == 33 && L.n_values == 140);
      for (int r = 0; r < 7; ++r) EXPECT(L.row_fpos[r] == 42 + 14 * r && L.row_scam[r] == 12 + 7 * L.row_cam[r] && L.row_spt[r] == 3 * L.row_pt[r]);
      EXPECT(eq(L.col_size, {3, 3, 3, 3, 7, 7, 7}) && !bal_records(L, Ints{0}, Ints{0, 2, 5, 7}, Ints(7, 42)).slots);
      // ---- groups [0, 1, 0] with camera 1 constant: every row an E cell and a group cell, the rows of cameras 0 and 2 a pose cell in front
      const int32_t grp[3] = {0, 1, 0};
      const uint8_t cam1[3] = {0, 1, 0};
      EXPECT(lay(L, kBalAngleAxis, cam1, nullptr, nullptr, grp, 2) == "");
      EXPECT(L.n_groups == 2 && eq(L.group_first, {0, 1}) && L.cw == 6 && L.nfc() == 2 && L.nfp() == 4 && L.n_t == 30 && L.n_values == 132);
      EXPECT(L.n_rows == 7 && L.n_rows_e == 7 && L.n_rows_f == 4);
      EXPECT(eq(L.row_fpos, {-1, 48, 66, 84, 102, -1, -1}) && eq(L.row_gpos, {42, 60, 78, 96, 114, 120, 126}));
      EXPECT(eq(L.row_scam, {-1, 18, 12, 12, 18, -1, -1}) && eq(L.row_sgrp, {27, 24, 24, 24, 24, 27, 27}));
      EXPECT(eq(L.cam_pose, {12, -1, 18}) && eq(L.cam_group, {24, 27, 24}) && eq(L.cam_first, {1, 1, 0}));
      EXPECT(eq(L.col_size, {3, 3, 3, 3, 6, 6, 3, 3}) && eq(L.col_pos, {0, 3, 6, 9, 12, 18, 24, 27}));
      EXPECT(eq(L.row_ptr, {0, 2, 5, 8, 11, 14, 16, 18}));
      EXPECT(eq(L.cell_col, {0, 7, 0, 5, 6, 1, 4, 6, 2, 4, 6, 2, 5, 6, 2, 7, 3, 7}));
      EXPECT(eq(L.cell_pos, {0, 42, 6, 48, 60, 12, 66, 78, 18, 84, 96, 24, 102, 114, 30, 120, 36, 126}));
      EXPECT(!bal_records(L, Ints{0}, Ints{0, 2, 4}, Ints(7, 42)).slots);
      // ---- refusals, each with the entry points' text
      const uint8_t all3[5] = {1, 1, 1, 0, 0}, all4[5] = {1, 1, 1, 1, 0};
      EXPECT(lay(L, kBalAngleAxis, all3) == "every camera is constant: no F block is left (Ceres switches the linear solver there, "
                                            "LinearSolverForZeroEBlocks and its kin; this front end does not)");
      EXPECT(lay(L, kBalAngleAxis, nullptr, all4) == "every point is constant: no E block is left (Ceres switches the linear solver there, "
                                                     "LinearSolverForZeroEBlocks; this front end does not)");
      // (a free camera and a free point that nothing observes: every observation is removed)
      EXPECT(lay(L, kBalAngleAxis, all3, all4, nullptr, nullptr, 0, 4, 5) == "no residual block is left: every observation has a constant camera and a constant point");
      const int32_t grp_far[3] = {0, 2, 0}, grp_one[3] = {0, 0, 0};
      EXPECT(lay(L, kBalAngleAxis, nullptr, nullptr, nullptr, grp_far, 2) == "camera 1 has group 2, not in [0, 2)");
      EXPECT(lay(L, kBalAngleAxis, nullptr, nullptr, nullptr, grp_one, 2) == "group 1 has no camera (every id in [0, num_groups) must be used)");
      EXPECT(lay(L, kBalAngleAxis, nullptr, nullptr, nullptr, grp, 4) == "num_groups 4 is not in [1, num_cameras = 3]");
      EXPECT(lay(L, kBalAngleAxis, nullptr, nullptr, nullptr, grp, 0) == "num_groups 0 is not in [1, num_cameras = 3]");
      const uint8_t c2[10] = {0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, c_all[10] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 0}, c6[10] = {0, 0, 0, 0, 0, 0, 1, 0, 0, 0};
      EXPECT(lay(L, kBalAngleAxis, nullptr, nullptr, c2) == "camera coordinate 2 cannot be constant: only the intrinsics, coordinates 6 .. 8 (f, k1, k2)");
      EXPECT(lay(L, kBalAngleAxis, nullptr, nullptr, c_all) == "every camera coordinate is constant: use constant cameras (camera_is_constant)");
      EXPECT(lay(L, kBalQuaternion, nullptr, nullptr, c6) == "constant camera coordinates are supported for the angle-axis camera only (camera_model 1)");
      EXPECT(lay(L, kBalQuaternionManifold, nullptr, nullptr, nullptr, grp, 2) == "shared intrinsics are supported for the angle-axis camera only (camera_model 2)");
      EXPECT(lay(L, kBalAngleAxis, nullptr, nullptr, nullptr, nullptr, 0, 2) == "observation index out of range");   // (camera 2 of 2)
      EXPECT(lay(L, kBalAngleAxis, nullptr, nullptr, nullptr, nullptr, 0, 3, 3) == "observation index out of range");   // (point 3 of 3)
      EXPECT(lay(L, 3) == "unknown camera_model 3" && lay(L, -1) == "unknown camera_model -1");
      EXPECT(bal_layout(kBalAngleAxis, 3, 4, 7, nullptr, kPt, kPixel, nullptr, nullptr, nullptr, nullptr, 0, L) == "bad arguments");
      EXPECT(bal_layout(kBalAngleAxis, 3, 4, 0, kCam, kPt, kPixel, nullptr, nullptr, nullptr, nullptr, 0, L) == "bad arguments");
      // more observations than 32-bit value positions hold (24 values each: 89 478 485 fit): refused before any array is read — they are
      // seven entries long here — and before anything of that size is allocated.  (NULL arrays are "bad arguments", an earlier check.)
      EXPECT(bal_layout(kBalAngleAxis, 3, 4, 89478485 + 1, kCam, kPt, kPixel, nullptr, nullptr, nullptr, nullptr, 0, L) ==
             "more than 89 M observations do not fit 32-bit value positions");
      EXPECT(bal_layout(kBalQuaternion, 3, 4, int64_t(1) << 40, kCam, kPt, kPixel, nullptr, nullptr, nullptr, nullptr, 0, L) ==
             "more than 82 M observations do not fit 32-bit value positions");
      // ---- the grouping: stable, the negative key skipped, two groups empty
      const int32_t keys[5] = {2, -1, 0, 2, 0};
      const BalGrouping G = bal_group_by(5, 4, [&](int64_t i) { return keys[i]; });
      EXPECT(eq(G.ptr, {0, 2, 2, 4, 4}) && eq(G.perm, {2, 4, 0, 3}) && eq(G.place, {2, -1, 0, 3, 1}));
      const double two[10] = {0, 1, 10, 11, 20, 21, 30, 31, 40, 41};
      EXPECT(eq(bal_gather(G.perm, keys), {0, 0, 2, 2}) && eq<double>(bal_gather(G.perm, two, 2), {20, 21, 40, 41, 0, 1, 30, 31}));
      EXPECT(eq(bal_gather(G, keys), {0, 0, 2, 2}) && eq<double>(bal_gather(G, two, 2), {20, 21, 40, 41, 0, 1, 30, 31}));   // (the same through the grouping)
      const BalGrouping none = bal_group_by(0, 2, [&](int64_t) { return 0; });
      EXPECT(eq(none.ptr, {0, 0, 0}) && none.perm.empty() && none.place.empty());
      std::printf("bal layout ok\n");
      return 0;
    }
"""


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_bal_layout(tmp_path, flags):
    src = tmp_path / "bal_layout_check.cc"
    src.write_text(textwrap.dedent(CHECK))
    exe = tmp_path / "bal_layout_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags + [
        "-I", os.path.join(ROOT, "ceres-solver_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "bal layout ok" in r.stdout, r.stdout + r.stderr
