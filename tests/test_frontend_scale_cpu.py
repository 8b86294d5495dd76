"""The wide scene of tests/frontend_scale_cases.py without a device: it exceeds every grid cap of the front end's kernels (read from
csrc/device.h) by a real second trip, its long points, multi-chunk cameras and chunk-crossing runs lie IN the second trip, the
row-range evaluator the references run through is the plain one, and the line search restatement's runs on it are non-degenerate
(as tests/test_line_search_cpu.py holds the small scenes' runs to be): tests/test_gpu_frontend_scale.py compares the device with them."""
import numpy as np
import pytest

import frontend_scale_cases as F
import line_search_cases as C

CONFIGS = [(camera, masks) for camera in C.MODELS for masks in F.MASKS]


@pytest.fixture(scope="module")
def hs():
    from conftest import pkg
    pkg.hip_solver.load_library()
    return pkg.hip_solver


def test_caps_are_the_named_constants_of_device_h():
    k = F.caps()["constants"]
    print("constants:", {n: k[n] for n in ("kVecBlock", "kMaxVecGrid", "kMaxEvalGrid", "kMaxLsCameraGrid")})
    assert F.caps()["rows"] == k["kMaxEvalGrid"] * 256 and F.caps()["vector"] == k["kMaxVecGrid"] * 256
    # the launchers use the names: no literal grid cap is left in them
    import os
    import re
    for name in ("kernels_evaluator.hip", "kernels_quaternion.hip", "kernels_line_search.hip", "kernels_line_search_quat.hip"):
        with open(os.path.join(os.path.dirname(F.DEVICE_H), name)) as f:
            text = f.read()
        assert not re.search(r"(>|min<int64_t>\()\s*(2048|4096)\b", text), name


def test_scene_has_the_prescribed_long_points_and_cameras(oracle):
    nc, npts, cam, pt, obs, _ = F.scene(oracle)
    track, degree = np.bincount(pt, minlength=npts), np.bincount(cam, minlength=nc)
    assert {q: int(track[q]) for q in F.LONG_POINT_ROWS} == F.LONG_POINT_ROWS
    assert {c: int(degree[c]) for c in F.HEAVY_CAMERA_ROWS} == F.HEAVY_CAMERA_ROWS
    ordinary_p, ordinary_c = np.delete(track, list(F.LONG_POINT_ROWS)), np.delete(degree, list(F.HEAVY_CAMERA_ROWS))
    print("observations", cam.shape[0], "longest ordinary track", ordinary_p.max(), "largest ordinary camera", ordinary_c.max())
    assert ordinary_p.max() <= 64 and ordinary_c.max() <= 64 and ordinary_p.min() >= 2 and ordinary_c.min() >= 1
    assert np.any(np.diff(pt) < 0)   # not grouped by point as given: the device sorts
    assert np.unique(np.stack([cam, pt]), axis=1).shape[1] == cam.shape[0]   # one residual block per (camera, point) pair


def test_tiles_exceed_the_tile_evaluators_grid(oracle, hs):
    op = F.oracle_problem(oracle)
    plan = hs.debug_plan(op.bs, op.nelim)
    assert plan["eligible"]
    print("tiles", plan["n_tiles"], "cap", F.caps()["tiles"])
    assert plan["n_tiles"] > F.caps()["tiles"] + 64
    # the long points' tiles are walked in the second trip
    long_tiles = np.flatnonzero(np.isin(plan["slot_pt"].reshape(-1, 64), list(F.LONG_POINT_ROWS)).any(axis=1) & (plan["valid"].reshape(-1, 64).any(axis=1)))
    assert long_tiles.size and long_tiles.min() >= F.caps()["tiles"]


@pytest.mark.parametrize("camera,masks", CONFIGS)
def test_every_program_takes_a_second_trip_with_its_edges_in_it(oracle, camera, masks):
    """Rows, camera chunks, free blocks and tangent size of the (reduced) program against the caps, and where the long points, the
    chunk-crossing runs and the multi-chunk cameras lie — in the device's row order (constant_blocks_reference.reduce) and its
    camera-major chunk list (bal_ls_prepare: the free cameras ascending, ceil(rows / 64) chunks each)."""
    cap = F.caps()
    w = F.reference_problem(oracle, camera, None, masks)
    rows = w.n_rows
    rpt, rcam = w.pt[w.row_order], w.cam[w.row_order]
    nfp, nfc = int(np.count_nonzero(w.pcol >= 0)), int(np.count_nonzero(w.ccol >= 0))
    degree = np.bincount(w.ccol[rcam][w.ccol[rcam] >= 0], minlength=nfc)
    first_chunk, n_chunks = F.chunks(degree)
    print(camera, masks, "rows", rows, "cap", cap["rows"], "| camera chunks", int(n_chunks.sum()), "cap", cap["camera_chunks"],
          "| free blocks", nfp + nfc, "tangent", w.n, "cap", cap["vector"])
    assert rows >= cap["rows"] + 4096
    assert n_chunks.sum() > cap["camera_chunks"] + 64
    assert nfp + nfc > cap["vector"] + 1024 and w.n > cap["vector"] + 1024
    # a multi-chunk camera with a chunk in the second trip
    multi = np.flatnonzero(n_chunks > 1)
    assert multi.size >= 3 and np.any(first_chunk[multi] + n_chunks[multi] - 1 >= cap["camera_chunks"])
    # runs of the free points in the row order: [a, b)
    e = w.n_rows_e
    starts = np.flatnonzero(np.concatenate([[True], np.diff(rpt[:e]) != 0]))
    ends = np.concatenate([starts[1:], [e]])
    length = ends - starts
    second = starts >= cap["rows"]
    assert np.any(second & (length > 64)), "a long point in the second trip"
    assert np.any(second & (length <= 64) & (starts // 64 != (ends - 1) // 64)), "an ordinary run across a chunk boundary in the second trip"
    if masks == "reduced":   # the constant blocks' rows: the tail (no E cell) and rows without an F cell, both beyond the cap
        assert e < rows and e >= cap["rows"] and np.any(~w.row_has_f[cap["rows"]:]) and np.any(~w.row_has_f[:cap["rows"]])


@pytest.mark.parametrize("camera,loss,masks", [("angle_axis", F.HUBER, "reduced"), ("quaternion", None, "none"), ("quaternion_manifold", F.CAUCHY, "reduced")])
def test_row_range_evaluator_is_the_plain_evaluator(oracle, camera, loss, masks):
    """On a small scene with uneven ranges (7 pieces): residuals and values to the bit (per row the same arithmetic), cost and gradient
    to the rounding of another summation order."""
    sc = C.small_scene(oracle, 3)
    cc, cp = ([0], [0, 1, 2]) if masks == "reduced" else (None, None)
    x0 = C.initial_state(sc, camera)
    plain = C.reference_problem(oracle, sc, camera, loss, cc, cp)
    ranged = F.row_parallel(C.reference_problem(oracle, sc, camera, loss, cc, cp), pieces=7)
    a, b = plain.evaluate(x0), ranged.evaluate(x0)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert abs(a[0] - b[0]) <= 1e-15 * a[0] and abs(plain.cost(x0) - ranged.cost(x0)) <= 1e-15 * a[0]
    assert np.max(np.abs(a[3] - b[3])) <= 1e-14 * np.max(np.abs(a[3]))
    terms = F.row_cost_terms(plain, x0)
    assert terms.shape[0] == plain.n_rows and abs(float(np.sum(terms)) - a[0]) <= 1e-15 * a[0]


@pytest.mark.parametrize("name", list(F.LINE_SEARCH_CASES))
def test_line_search_runs_on_the_scene_are_not_degenerate(oracle, name):
    _, _, (_, S) = F.run_line_search_reference(oracle, name)
    trace = S["trace"]
    print(name, "cost", S["initial_cost"], "->", S["final_cost"], "smallest margin", trace.min_margin(), "evaluations", S["counts"])
    assert S["num_iterations"] == F.LINE_SEARCH_ITERATIONS == len(S["iterations"]) - 1
    assert S["final_cost"] < S["initial_cost"] and all(b["cost"] < a["cost"] for a, b in zip(S["iterations"][:-1], S["iterations"][1:]))
    assert trace.min_margin() >= 1e-6, sorted(trace.margins, key=lambda m: m[1])[:3]
