"""INTEGRATION.md's structure flattening: the code the adapter runs (ceres-solver_amd/host/flatten_block_structure.h,
a template on the structure type) is compiled with g++ and run on a hand-built structure, flattened and compared.

* Always: on the dependency-free CompressedRowBlockStructure of the C++ mirror (ceres-solver_amd/host/hip_linear_solver.h), the type
  the host driver flattens.
* With CERES_SOURCE_DIR=<a Ceres source tree>, in the same test: also on Ceres' REAL internal/ceres/block_structure.h (field names
  and types checked by the compiler).  That header needs <vector>, <cstdint> and "ceres/internal/export.h" — a file Ceres' CMake
  GENERATES (visibility macros only); the test writes an empty-macro one into a temporary directory.  Nothing of Ceres is copied."""
import os
import subprocess
import textwrap

from conftest import ROOT

CERES_SOURCE_DIR = os.environ.get("CERES_SOURCE_DIR", "")

CHECK = """
    int main() {
      // two 3-wide points, two 9-wide cameras, three 2-high observation rows, E|F-split values
      CompressedRowBlockStructure bs;
      bs.cols = {Block(3, 0), Block(3, 3), Block(9, 6), Block(9, 15)};
      const int pt[3] = {0, 0, 1}, cam[3] = {2, 3, 2};
      for (int r = 0; r < 3; ++r) {
        CompressedRow row;
        row.cells.resize(2);
        row.block = Block(2, 2 * r);
        row.cells[0] = Cell(pt[r], 6 * r);
        row.cells[1] = Cell(cam[r], 18 + 18 * r);
        bs.rows.push_back(row);
      }
      const ceres_hip::FlatBlockStructure f = ceres_hip::FlattenBlockStructure(bs);
      const ceres_hip_block_structure v = f.view();
      bool ok = v.num_row_blocks == 3 && v.num_col_blocks == 4;
      const int want_ptr[4] = {0, 2, 4, 6}, want_col[6] = {0, 2, 0, 3, 1, 2}, want_val[6] = {0, 18, 6, 36, 12, 54};
      for (int i = 0; i < 4; ++i) ok = ok && v.row_cell_ptr[i] == want_ptr[i];
      for (int i = 0; i < 6; ++i) ok = ok && v.cell_col_block[i] == want_col[i] && v.cell_value_pos[i] == want_val[i];
      for (int r = 0; r < 3; ++r) ok = ok && v.row_block_size[r] == 2 && v.row_block_pos[r] == 2 * r;
      ok = ok && v.col_block_size[2] == 9 && v.col_block_pos[3] == 15;
      std::printf(ok ? "flatten ok\\n" : "flatten MISMATCH\\n");
      return ok ? 0 : 1;
    }
"""


def compile_and_run(tmp_path, prelude, include_dirs):
    tmp_path.mkdir(parents=True, exist_ok=True)
    src = tmp_path / "flatten_check.cc"
    src.write_text(textwrap.dedent(prelude) + textwrap.dedent(CHECK))
    exe = tmp_path / "flatten_check"
    cmd = ["g++", "-std=c++17", "-O1"] + [a for d in include_dirs for a in ("-I", str(d))] + [
        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ceres-solver_amd", "host"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "flatten ok" in r.stdout, r.stdout + r.stderr


def test_flattening_compiles_and_runs_on_the_mirror_block_structure(tmp_path):
    compile_and_run(tmp_path / "mirror", """
        #include <cstdio>
        #include "hip_linear_solver.h"              // the mirror's structure types; includes flatten_block_structure.h
        using ceres_hip::Block;
        using ceres_hip::Cell;
        using ceres_hip::CompressedRow;
        using ceres_hip::CompressedRowBlockStructure;
        """, [])
    if not CERES_SOURCE_DIR:
        return
    assert os.path.exists(os.path.join(CERES_SOURCE_DIR, "internal", "ceres", "block_structure.h")), \
        f"CERES_SOURCE_DIR={CERES_SOURCE_DIR} is not a Ceres source tree"
    inc = tmp_path / "gen" / "ceres" / "internal"
    inc.mkdir(parents=True)
    (inc / "export.h").write_text("#ifndef CERES_EXPORT\n#define CERES_EXPORT\n#define CERES_NO_EXPORT\n#endif\n")
    compile_and_run(tmp_path / "ceres", """
        #include <cstdio>
        #include "ceres/block_structure.h"          // Ceres' own header
        #include "flatten_block_structure.h"        // what the adapter runs
        using ceres::internal::Block;
        using ceres::internal::Cell;
        using ceres::internal::CompressedRow;
        using ceres::internal::CompressedRowBlockStructure;
        """, [os.path.join(CERES_SOURCE_DIR, "internal"), tmp_path / "gen"])
