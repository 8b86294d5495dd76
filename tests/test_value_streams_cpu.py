"""The plan of the streamed upload (csrc/plan.cc, PlanValueStreams, through ceres_hip_debug_value_streams) against its restatement in
numpy (tests/streamed_upload_reference.py): how many value streams a layout has, and that the range a run of row blocks owns in each
stream is exactly the bytes of the run's cells — for every run of 1, 2, 3 and 5 rows of every layout below, none of which has more than
400 row blocks.  The stream counts are pinned (design/26_streamed_upload_tests.md): Ceres' Schur layout with camera priors has NO
stream today, and a change of that is to be a visible decision.

The planner is also compiled on its own (plan.cc, nothing else) into a stand-alone program with the address and undefined-behaviour
sanitizers and run on three hand-made structures; nothing is preloaded, the program has its own main."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

import streamed_upload_reference as ref
from conftest import ROOT, pkg

problems = pkg.problems
BlockStructure = pkg.BlockStructure


def drop_camera_cells(p, rows):
    """A Schur-layout scene whose row blocks `rows` lost their camera cell (a locked camera, examples/libmv_bundle_adjuster.cc:725-728):
    the E cells stay where they are, the remaining F cells are laid out back to back behind them, in row order."""
    bs = p.bs
    ptr = bs.row_cell_ptr.astype(np.int64)
    lose = np.zeros(bs.num_row_blocks, dtype=bool)
    lose[np.asarray(rows, dtype=np.int64)] = True
    new_rows, pos_f = [], None
    e_end = 0
    for r in range(bs.num_row_blocks):
        c = int(ptr[r])
        e_end = max(e_end, int(bs.cell_value_pos[c]) + int(bs.row_block_size[r]) * int(bs.col_block_size[bs.cell_col_block[c]]))
    pos_f = e_end
    for r in range(bs.num_row_blocks):
        c0, c1 = int(ptr[r]), int(ptr[r + 1])
        cells = [(int(bs.cell_col_block[c0]), int(bs.cell_value_pos[c0]))]
        if not lose[r]:
            for c in range(c0 + 1, c1):
                cells.append((int(bs.cell_col_block[c]), pos_f))
                pos_f += int(bs.row_block_size[r]) * int(bs.col_block_size[bs.cell_col_block[c]])
        new_rows.append((int(bs.row_block_size[r]), cells))
    return BlockStructure.from_rows(bs.col_block_size, new_rows)


def _schur():
    return problems.synthetic_bal(None, layout="schur", num_cameras=7, num_points=60, num_observations=300, seed=4)


def _cgnr():
    return problems.synthetic_bal(None, layout="cgnr", num_cameras=7, num_points=60, num_observations=300, seed=4)


def _shuffled(p, seed):
    return problems.permute_rows(p, np.random.default_rng(seed).permutation(p.bs.num_row_blocks))


def _lost(which):
    p = _schur()
    n = p.bs.num_row_blocks
    rows = {"leading": np.arange(0, 9), "trailing": np.arange(n - 11, n), "random": np.flatnonzero(np.random.default_rng(6).random(n) < 0.3),
            "mixed": np.concatenate([np.arange(0, 4), np.arange(50, 53), np.arange(n - 2, n)]), "all": np.arange(n)}[which]
    return drop_camera_cells(p, rows)


# name -> (structure, value streams of the table in design/26_streamed_upload_tests.md)
LAYOUTS = {
    "schur": (lambda: _schur().bs, 2),
    "cgnr": (lambda: _cgnr().bs, 1),
    "schur+camera rows": (lambda: problems.add_camera_rows(_schur(), 40, seed=1, pair_fraction=0.4).bs, 0),
    "cgnr+camera rows": (lambda: problems.add_camera_rows(_cgnr(), 40, seed=1, pair_fraction=0.4).bs, 1),
    "schur permuted": (lambda: _shuffled(_schur(), 2).bs, 0),
    "cgnr permuted": (lambda: _shuffled(_cgnr(), 2).bs, 0),
    "schur+camera rows permuted": (lambda: _shuffled(problems.add_camera_rows(_schur(), 40, seed=1, pair_fraction=0.4), 3).bs, 0),
    "cgnr+camera rows permuted": (lambda: _shuffled(problems.add_camera_rows(_cgnr(), 40, seed=1, pair_fraction=0.4), 3).bs, 0),
    "random schur, row-sequential values": (lambda: problems.random_schur_problem(num_e_blocks=40, num_f_blocks=9, seed=8, shuffle_values=False).bs, 1),
    "random schur, shuffled values": (lambda: problems.random_schur_problem(num_e_blocks=40, num_f_blocks=9, seed=8, shuffle_values=True).bs, 0),
    "random block sparse": (lambda: problems.random_block_sparse(num_row_blocks=120, num_col_blocks=15, seed=3).bs, 1),
    "libmv structured": (lambda: _libmv().bs, 2),
    "synthetic structured, strip": (lambda: problems.synthetic_structured(7, 60, 300, camera_width=6, shared_widths=(3,), seed=5).bs, 2),
    "synthetic structured, strip, cgnr": (lambda: problems.synthetic_structured(7, 60, 300, camera_width=6, shared_widths=(3,), layout="cgnr", seed=5).bs, 1),
    "schur, leading rows without a camera cell": (lambda: _lost("leading"), 2),
    "schur, trailing rows without a camera cell": (lambda: _lost("trailing"), 2),
    "schur, random rows without a camera cell": (lambda: _lost("random"), 2),
    "schur, mixed rows without a camera cell": (lambda: _lost("mixed"), 2),
    "schur, no row with a camera cell": (lambda: _lost("all"), 1),
    "one row block": (lambda: BlockStructure.from_rows([3, 9], [(2, [(0, 0), (1, 6)])]), 1),
    "a gap between two cells": (lambda: BlockStructure.from_rows([3], [(2, [(0, 0)]), (2, [(0, 8)])]), 0),
}


def _libmv():
    """libmv's structure (every row on the shared intrinsics block, the first camera locked) on the first 400 rows' worth of a real
    visibility graph: whole points, observations sorted by point."""
    n_c, n_p, cam_of, pt_of = problems.libmv_visibility(2)
    order = np.lexsort((cam_of, pt_of))
    cam_of, pt_of = cam_of[order], pt_of[order]
    n_pts = int(pt_of[399])   # the points below the one row 399 belongs to are whole
    keep = pt_of < n_pts
    return problems.structured_bal(n_c, n_pts, pt_of[keep], cam_of[keep], 6, (8,), True, (0,), None, "schur", 7, with_values=False)


@pytest.fixture(scope="module", params=list(LAYOUTS), ids=[k.replace(" ", "_").replace(",", "") for k in LAYOUTS])
def layout(request):
    make, streams = LAYOUTS[request.param]
    bs = make()
    assert 1 <= bs.num_row_blocks <= 400, bs.num_row_blocks
    k, lo, hi = pkg.hip_solver.debug_value_streams(bs)
    return request.param, bs, streams, k, lo, hi


def test_stream_count(layout):
    name, bs, streams, k, lo, hi = layout
    assert k == ref.value_streams(bs) == streams, (name, k, ref.value_streams(bs), streams)
    if k == 0:
        assert not lo.any() and not hi.any()


def test_every_run_owns_exactly_its_cells(layout):
    name, bs, streams, k, lo, hi = layout
    nrb = bs.num_row_blocks
    per_row = [[ref.class_bytes(bs, r, r + 1, c, k) for r in range(nrb)] for c in range(k)]
    for n in (1, 2, 3, 5):
        for r0 in range(0, nrb - n + 1):
            r1 = r0 + n
            sent = []
            for c in range(k):
                a, b = int(lo[c, r0]), int(hi[c, r1 - 1])
                assert a <= b, (name, n, r0, c, a, b)
                own = np.sort(np.concatenate(per_row[c][r0:r1]))
                assert np.array_equal(np.arange(a, b), own), (name, n, r0, c, a, b)
                sent.append(np.arange(a, b))
            if k > 0:
                want, _ = ref.run_bytes(bs, r0, r1)
                assert np.array_equal(np.sort(np.concatenate(sent)), want), (name, n, r0)


def test_single_rows_partition_the_cell_bytes(layout):
    name, bs, streams, k, lo, hi = layout
    if k == 0:
        return   # nothing goes up by rows: ceres_hip_values_end sends the whole array
    extent = bs.values_extent()
    count = np.zeros(extent, dtype=np.int64)
    for c in range(k):
        for r in range(bs.num_row_blocks):
            assert 0 <= lo[c, r] <= hi[c, r] <= extent
            count[lo[c, r]:hi[c, r]] += 1
    assert np.array_equal(count, ref.cell_mask(bs, extent).astype(np.int64)), name


CHECK = """
    #include <cstdio>
    #include <vector>
    #include "common.h"

    #define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\\n", __LINE__, #cond); return 1; } } while (0)

    struct Rows {
      std::vector<int32_t> rsz, rpos, csz, cpos, rptr{0}, ccol, cval;
      void col(int size) { cpos.push_back(cpos.empty() ? 0 : cpos.back() + csz.back()); csz.push_back(size); }
      void row(int size) { rpos.push_back(rpos.empty() ? 0 : rpos.back() + rsz.back()); rsz.push_back(size); rptr.push_back(rptr.back()); }
      void cell(int block, int pos) { ccol.push_back(block); cval.push_back(pos); ++rptr.back(); }
    };

    // every double of a cell in exactly one row's range of exactly one class, no other double in any
    static int check(const Rows& R, int want_streams) {
      ceres_hip_block_structure bs;
      bs.num_row_blocks = int32_t(R.rsz.size()); bs.num_col_blocks = int32_t(R.csz.size());
      bs.row_block_size = R.rsz.data(); bs.row_block_pos = R.rpos.data(); bs.col_block_size = R.csz.data(); bs.col_block_pos = R.cpos.data();
      bs.row_cell_ptr = R.rptr.data(); bs.cell_col_block = R.ccol.data(); bs.cell_value_pos = R.cval.data();
      chip::HostStructure h;
      EXPECT(chip::AnalyzeStructure(bs, 0, &h).empty());
      chip::ValueStreamPlan P;
      chip::PlanValueStreams(h, &P);
      EXPECT(P.streams == want_streams);
      std::vector<int> owned(size_t(h.values_extent), 0), cell(size_t(h.values_extent), 0);
      for (int r = 0; r < h.nrb; ++r)
        for (int c = h.rptr[r]; c < h.rptr[r + 1]; ++c)
          for (int64_t i = h.cval[c]; i < h.cval[c] + int64_t(h.rsz[r]) * h.csz[h.ccol[c]]; ++i) ++cell[size_t(i)];
      for (int k = 0; k < P.streams; ++k) {
        EXPECT(int(P.lo[k].size()) == h.nrb && int(P.hi[k].size()) == h.nrb);
        for (int r = 0; r < h.nrb; ++r) {
          EXPECT(0 <= P.lo[k][size_t(r)] && P.lo[k][size_t(r)] <= P.hi[k][size_t(r)] && P.hi[k][size_t(r)] <= h.values_extent);
          if (r > 0) EXPECT(P.lo[k][size_t(r)] == P.hi[k][size_t(r - 1)]);   // a run [r0, r1) owns [lo[r0], hi[r1 - 1]): no hole, no overlap
          for (int64_t i = P.lo[k][size_t(r)]; i < P.hi[k][size_t(r)]; ++i) ++owned[size_t(i)];
        }
      }
      for (size_t i = 0; i < owned.size(); ++i) EXPECT(owned[i] == cell[i] && cell[i] <= 1);
      return 0;
    }

    int main() {
      {   // two streams: three E cells (2 x 3), then the F cells (2 x 9) of the rows
        Rows R; R.col(3); R.col(3); R.col(9); R.col(9);
        R.row(2); R.cell(0, 0); R.cell(2, 18);
        R.row(2); R.cell(0, 6); R.cell(3, 36);
        R.row(2); R.cell(1, 12); R.cell(2, 54);
        if (check(R, 2)) return 1;
      }
      {   // one stream: row-sequential values, rows of different heights, a row with one cell
        Rows R; R.col(3); R.col(9); R.col(2);
        R.row(2); R.cell(0, 0); R.cell(1, 6);
        R.row(1); R.cell(2, 24);
        R.row(3); R.cell(0, 26); R.cell(1, 35); R.cell(2, 62);
        if (check(R, 1)) return 1;
      }
      {   // the leading rows (and one in the middle, and the last) have no class-1 cell: they own the empty range where the stream stands
        Rows R; R.col(3); R.col(3); R.col(9);
        R.row(2); R.cell(0, 0);
        R.row(2); R.cell(0, 6);
        R.row(2); R.cell(1, 12); R.cell(2, 36);
        R.row(2); R.cell(1, 18);
        R.row(2); R.cell(1, 24); R.cell(2, 54);
        R.row(2); R.cell(0, 30);
        if (check(R, 2)) return 1;
      }
      std::printf("value streams ok\\n");
      return 0;
    }
"""


def test_planner_alone_under_the_sanitizers(tmp_path):
    src = tmp_path / "value_streams_check.cc"
    src.write_text(textwrap.dedent(CHECK))
    exe = tmp_path / "value_streams_check"
    csrc = os.path.join(ROOT, "ceres-solver_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, str(src),
           os.path.join(csrc, "plan.cc"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "value streams ok" in r.stdout, r.stdout + r.stderr
