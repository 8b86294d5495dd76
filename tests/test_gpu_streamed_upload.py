"""The upload hidden behind the evaluator (include/ceres_hip.h: ceres_hip_values_begin / _ready / _end): rows go up
from several threads while later rows are still being written, unscaled, Jacobi scaling on the device — and the step must be the
one ceres_hip_lm_compute_step computes from the same values — the same kernels on the same bytes, so equal up to the order of the
camera-space additions in LDS (1e-12) — which in turn is checked against the oracle.

The reference's side of this boundary: ProgramEvaluator::Evaluate's parallel loop (internal/ceres/program_evaluator.h:168-300) writing
BlockSparseMatrix::values() (pinned: internal/ceres/block_jacobian_writer.cc:261-262), then ScaleColumns
(internal/ceres/trust_region_minimizer.cc:263-279).

The second half of the module looks at what arrived in HBM instead of at a step computed from it (design/26_streamed_upload_tests.md)."""
import threading

import numpy as np
import pytest

import streamed_upload_reference as image
from test_gpu_lm_step import check_step, reference_step

pytestmark = pytest.mark.gpu


def same(a, b, tol=1e-12):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b))) <= tol * float(np.linalg.norm(np.asarray(b)))


def make(hip, p, solver_type, pre):
    o = hip.LinearSolverOptions(type=solver_type, preconditioner_type=pre, min_num_iterations=0, max_num_iterations=500,
                                elimination_groups=[p.num_eliminate_blocks if solver_type != hip.CGNR else 0])
    s = hip.HipLinearSolver(o)
    s.set_structure(p.bs)
    return s


def stream_up(s, p, values_src, b_src, n_threads=8, run=97, skip_every=0, scale=None, order="shuffled"):
    """Eight 'evaluator' threads fill the host arrays run by run (runs in a shuffled order) and announce them."""
    bs = p.bs
    hv = np.full(values_src.shape[0], np.nan)
    hb = np.full(b_src.shape[0], np.nan)
    ptr = bs.row_cell_ptr.astype(np.int64)
    rsz = bs.row_block_size.astype(np.int64)
    csz = bs.col_block_size.astype(np.int64)
    runs = [(r0, min(bs.num_row_blocks, r0 + run)) for r0 in range(0, bs.num_row_blocks, run)]
    if order == "shuffled":
        np.random.default_rng(5).shuffle(runs)
    s.values_begin(hv, hb)
    lock, errors = threading.Lock(), []

    def worker(t):
        try:
            while True:
                with lock:
                    if not runs:
                        return
                    k = len(runs)
                    r0, r1 = runs.pop()
                for r in range(r0, r1):
                    for c in range(ptr[r], ptr[r + 1]):
                        a = int(bs.cell_value_pos[c])
                        n = int(rsz[r] * csz[bs.cell_col_block[c]])
                        hv[a:a + n] = values_src[a:a + n]
                    b0 = int(bs.row_block_pos[r])
                    hb[b0:b0 + int(rsz[r])] = b_src[b0:b0 + int(rsz[r])]
                if skip_every and k % skip_every == 0:
                    continue   # never announced: values_end sends it
                s.values_ready(r0, r1 - r0)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(n_threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    s.values_end(scale)
    return s.stream_stats()


@pytest.mark.parametrize("layout,solver_type,pre,streams", [("schur", 5, 2, 2), ("schur", 6, 1, 2), ("cgnr", 6, 1, 1)])
def test_streamed_step_equals_the_plain_step(hip, oracle, problems, layout, solver_type, pre, streams):
    p = problems.synthetic_bal(None, layout=layout, num_cameras=31, num_points=4000, num_observations=17000, seed=11, skew=0.5)
    ref = make(hip, p, solver_type, pre)
    step0, summ0, mcc0 = ref.lm_compute_step(p.values, p.b, 1e4, 0.1)
    D = ref.lm_diagonal()
    check_step(oracle, hip, p, solver_type, pre, D, step0, summ0, mcc0, 0.1)
    s = make(hip, p, solver_type, pre)
    early, late, k = stream_up(s, p, p.values, p.b, skip_every=7)
    assert k == streams and early > 0 and late > 0 and early + late == 8 * (p.values.shape[0] + p.b.shape[0])
    step, summ, mcc = s.lm_compute_step(None, None, 1e4, 0.1, values_unchanged=True)
    assert summ.num_iterations == summ0.num_iterations and same(step, step0) and same(mcc, mcc0)
    # a second evaluation on the same handle (the next LM iteration): other values, everything announced, in row order
    v2 = p.values * (1.0 + 0.1 * np.cos(np.arange(p.values.shape[0])))
    early, late, _ = stream_up(s, p, v2, p.b, run=1000, order="rows")
    assert late == 0
    step2, summ2, mcc2 = s.lm_compute_step(None, None, 1e4, 0.1, values_unchanged=True)
    step2r, summ2r, mcc2r = ref.lm_compute_step(v2, p.b, 1e4, 0.1)
    assert same(step2, step2r) and same(mcc2, mcc2r)


def test_jacobi_scaling_on_the_device(hip, oracle, problems):
    p = problems.synthetic_bal(None, layout="schur", num_cameras=19, num_points=2500, num_observations=11000, seed=3, skew=0.4)
    m = oracle.Matrix(p.bs, 0)
    scale = 1.0 / (1.0 + np.sqrt(m.squared_column_norm(p.values)))   # TrustRegionMinimizer's jacobian_scaling_ (:263-279)
    scaled = ref_scaled = None
    ref = make(hip, p, 5, 2)
    ref.load(p.values, p.b)
    scaled = ref.scale_columns(scale)                                  # BlockSparseMatrix::ScaleColumns, already covered against the oracle
    step0, summ0, mcc0 = ref.lm_compute_step(scaled, p.b, 1e4, 0.1)
    s = make(hip, p, 5, 2)
    stream_up(s, p, p.values, p.b, scale=scale)                        # the UNSCALED values go up
    step, summ, mcc = s.lm_compute_step(None, None, 1e4, 0.1, values_unchanged=True)
    assert summ.num_iterations == summ0.num_iterations and same(step, step0) and same(mcc, mcc0)
    ps = type(p)(p.bs, scaled, p.b, None, p.num_eliminate_blocks)
    check_step(oracle, hip, ps, 5, 2, s.lm_diagonal(), step, summ, mcc, 0.1)
    del ref_scaled


def test_a_layout_without_monotone_streams_goes_up_at_the_end(hip, problems):
    # the cells of the rows in reverse order in the value array: not one or two monotone streams
    p = problems.synthetic_bal(None, layout="schur", num_cameras=9, num_points=300, num_observations=1200, seed=2)
    bs = p.bs
    n_cells = bs.cell_value_pos.shape[0]
    rows_of_cell = np.repeat(np.arange(bs.num_row_blocks), np.diff(bs.row_cell_ptr))
    size = bs.row_block_size[rows_of_cell].astype(np.int64) * bs.col_block_size[bs.cell_col_block].astype(np.int64)
    new_pos = np.zeros(n_cells, dtype=np.int64)
    new_pos[::-1] = np.concatenate([[0], np.cumsum(size[::-1])[:-1]])
    values = np.empty_like(p.values)
    for c in range(n_cells):
        values[new_pos[c]:new_pos[c] + size[c]] = p.values[bs.cell_value_pos[c]:bs.cell_value_pos[c] + size[c]]
    bs2 = type(bs)(bs.row_block_size, bs.row_block_pos, bs.col_block_size, bs.col_block_pos, bs.row_cell_ptr, bs.cell_col_block, new_pos.astype(np.int32))
    p2 = type(p)(bs2, values, p.b, None, p.num_eliminate_blocks)
    ref = make(hip, p2, 5, 2)
    step0, summ0, mcc0 = ref.lm_compute_step(p2.values, p2.b, 1e4, 0.1)
    s = make(hip, p2, 5, 2)
    early, late, k = stream_up(s, p2, p2.values, p2.b)
    assert k == 0 and early == 0 and late == 8 * (values.shape[0] + p.b.shape[0])
    step, summ, mcc = s.lm_compute_step(None, None, 1e4, 0.1, values_unchanged=True)
    assert same(step, step0) and same(mcc, mcc0)


def test_misuse_is_an_error(hip, problems):
    p = problems.synthetic_bal(None, layout="schur", num_cameras=7, num_points=200, num_observations=800, seed=4)
    s = make(hip, p, 5, 2)
    with pytest.raises(hip.HipError):
        s.values_ready(0, 1)                      # outside begin / end
    with pytest.raises(hip.HipError):
        s.values_end()
    hv, hb = p.values.copy(), p.b.copy()
    s.values_begin(hv, hb)
    s.values_ready(0, 10)
    with pytest.raises(hip.HipError):
        s.values_ready(5, 1)                      # announced twice
    with pytest.raises(hip.HipError):
        s.values_ready(p.bs.num_row_blocks - 1, 2)  # out of range
    s.values_end()
    step, summ, mcc = s.lm_compute_step(None, None, 1e4, 0.1, values_unchanged=True)
    assert np.isfinite(step).all() and mcc > 0


@pytest.mark.parametrize("shuffle,streams", [(False, 1), (True, 0)])
def test_streaming_on_the_generic_kernels(hip, oracle, problems, shuffle, streams):
    """Any block sizes, rows with several F cells and rows without an E block (the generic path): a row-sequential value layout is one
    stream, a shuffled one goes up at the end; the solve on the streamed values equals the plain solve and the oracle's."""
    p = problems.random_schur_problem(num_e_blocks=40, num_f_blocks=9, seed=8, shuffle_values=shuffle)
    ref = make(hip, p, 5, 2)
    assert ref.info().kernel_path == hip.PATH_GENERIC
    step0, summ0, mcc0 = ref.lm_compute_step(p.values, p.b, 1e4, 1e-12)
    s = make(hip, p, 5, 2)
    early, late, k = stream_up(s, p, p.values, p.b, run=3)
    assert k == streams and (early > 0) == (streams > 0)
    step, summ, mcc = s.lm_compute_step(None, None, 1e4, 1e-12, values_unchanged=True)
    assert summ.termination_type == hip.SUCCESS and same(step, step0, 1e-9) and same(mcc, mcc0, 1e-9)
    check_step(oracle, hip, p, 5, 2, s.lm_diagonal(), step, summ, mcc, 1e-12, tol=1e-8)


# ---- what arrived in HBM ---------------------------------------------------------------------------------------------------------------
# The tests above compare a STEP with another run of the same library.  A run of rows that goes up one double short passes them whenever
# a neighbouring announcement or the previous iteration's values cover the hole, and a second upload lands on a copy that already holds
# nearly the right numbers.  The tests below read the device's copy back (ceres_hip_debug_read_loaded) and compare it bit for bit with
# tests/streamed_upload_reference.py: every double of a cell is the host's (times scale[column]: one fp64 multiply, bit-equal to numpy's
# product), every residual is the host's; doubles of the value array that belong to no cell are unconstrained.  Every handle first loads
# a sentinel image (values -7, residuals -9) and every host array starts as NaN, so a byte that never went up shows either way; the host
# arrays are pinned, so the copies really are asynchronous.

def pinned(n):
    import torch
    return torch.empty(n, dtype=torch.float64).pin_memory().numpy()


def sentinel(s, bs):
    s.load(np.full(bs.values_extent(), -7.0), np.full(bs.num_rows, -9.0))


def column_scale(bs, seed=17):
    return 1.0 / (1.0 + np.random.default_rng(seed).random(bs.num_cols))


def row_filler(bs, hv, hb, values_src, b_src):
    """fill(r0, r1): what an evaluator thread does for row blocks [r0, r1) — their cells and residuals, nothing else."""
    ptr, rsz, rpos = bs.row_cell_ptr.tolist(), bs.row_block_size.tolist(), bs.row_block_pos.tolist()
    pos, width = bs.cell_value_pos.tolist(), bs.col_block_size[bs.cell_col_block].tolist()

    def fill(r0, r1):
        for r in range(r0, r1):
            for c in range(ptr[r], ptr[r + 1]):
                a, n = pos[c], rsz[r] * width[c]
                hv[a:a + n] = values_src[a:a + n]
            hb[rpos[r]:rpos[r] + rsz[r]] = b_src[rpos[r]:rpos[r] + rsz[r]]
    return fill


def runs_of(bs, run=97, seed=5):
    runs = [(r0, min(bs.num_row_blocks, r0 + run)) for r0 in range(0, bs.num_row_blocks, run)]
    np.random.default_rng(seed).shuffle(runs)
    return runs


def every_seventh_unannounced(runs):
    return [(r0, r1, [] if i % 7 == 0 else [(r0, r1 - r0)]) for i, (r0, r1) in enumerate(runs)]


def session(s, bs, values_src, b_src, plan, n_threads=8, scale=None, after_end=None):
    """One streamed upload from pinned arrays.  plan = [(r0, r1, calls)]: a thread fills row blocks [r0, r1) and then makes the
    values_ready calls `calls` = [(first, n), ...]; the plan is worked off from its end.  after_end(hv, hb) runs as soon as values_end has
    returned.  Returns the host arrays."""
    hv, hb = pinned(bs.values_extent()), pinned(bs.num_rows)
    hv.fill(np.nan)
    hb.fill(np.nan)
    fill = row_filler(bs, hv, hb, values_src, b_src)
    todo = list(plan)
    s.values_begin(hv, hb)
    lock, errors = threading.Lock(), []

    def worker():
        try:
            while True:
                with lock:
                    if not todo:
                        return
                    r0, r1, calls = todo.pop()
                fill(r0, r1)
                for first, n in calls:
                    s.values_ready(first, n)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=worker) for _ in range(n_threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    s.values_end(scale)
    if after_end is not None:
        after_end(hv, hb)
    return hv, hb


def check_image(s, bs, values, b, scale=None):
    dv, db = s.read_loaded()
    want_v, want_b, mask = image.device_image(bs, values, b, scale)
    assert int(mask.sum()) == bs.num_nonzeros and np.isfinite(want_v[mask]).all() and np.isfinite(want_b).all()
    at = np.flatnonzero(mask)
    bad = np.flatnonzero(dv[at].view(np.uint64) != want_v[at].view(np.uint64))
    assert bad.size == 0, (f"{bad.size} of {at.size} cell doubles differ; the first is value {at[bad[0]]}: "
                           f"device {dv[at[bad[0]]]!r}, expected {want_v[at[bad[0]]]!r}")
    bad = np.flatnonzero(db.view(np.uint64) != want_b.view(np.uint64))
    assert bad.size == 0, f"{bad.size} of {db.size} residuals differ; the first is {bad[0]}: device {db[bad[0]]!r}, expected {want_b[bad[0]]!r}"


def all_bytes(bs):
    v, b = image.run_bytes(bs, 0, bs.num_row_blocks)
    return 8 * (int(v.shape[0]) + int(b.shape[0]))


BIG = dict(num_cameras=31, num_points=4000, num_observations=17000, seed=11, skew=0.5)
MID = dict(num_cameras=19, num_points=2500, num_observations=11000, seed=3, skew=0.4)
SMALL = dict(num_cameras=7, num_points=200, num_observations=800, seed=4)


def layout_problem(problems, name):
    """(problem, solver type, preconditioner, value streams of the layout: design/26_streamed_upload_tests.md)"""
    if name == "schur":
        return problems.synthetic_bal(None, layout="schur", **BIG), 5, 2, 2
    if name == "cgnr":
        return problems.synthetic_bal(None, layout="cgnr", **BIG), 6, 1, 1
    if name == "schur+camera rows":   # Ceres' Schur layout with camera priors: the priors' first cells lie behind the F cells — no stream
        return problems.add_camera_rows(problems.synthetic_bal(None, layout="schur", **MID), 60, seed=1, pair_fraction=0.4), 5, 2, 0
    if name in ("cgnr+camera rows", "cgnr+camera rows, permuted"):
        p = problems.add_camera_rows(problems.synthetic_bal(None, layout="cgnr", **MID), 60, seed=1, pair_fraction=0.4)
        if name == "cgnr+camera rows":
            return p, 6, 1, 1
        return problems.permute_rows(p, np.random.default_rng(9).permutation(p.bs.num_row_blocks)), 6, 1, 0
    if name == "strip":
        return problems.synthetic_structured(19, 2500, 11000, camera_width=9, shared_widths=(3,), seed=5, skew=0.4), 5, 2, 2
    if name == "camera width 6":
        return problems.synthetic_structured(19, 2500, 11000, camera_width=6, seed=6, skew=0.4), 5, 2, 2
    if name == "generic":
        return problems.random_schur_problem(num_e_blocks=40, num_f_blocks=9, seed=8, shuffle_values=False), 5, 2, 1
    if name == "generic, shuffled values":
        return problems.random_schur_problem(num_e_blocks=40, num_f_blocks=9, seed=8, shuffle_values=True), 5, 2, 0
    raise ValueError(name)


LAYOUTS = ["schur", "cgnr", "schur+camera rows", "cgnr+camera rows", "cgnr+camera rows, permuted", "strip", "camera width 6", "generic",
           "generic, shuffled values"]


@pytest.mark.parametrize("with_scale", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("name", LAYOUTS, ids=[n.replace(" ", "_").replace(",", "") for n in LAYOUTS])
def test_the_device_holds_the_bytes_of_the_host(hip, problems, name, with_scale):
    """Eight threads, shuffled runs of 97 row blocks, every 7th run never announced, pinned arrays."""
    p, solver_type, pre, streams = layout_problem(problems, name)
    bs = p.bs
    with make(hip, p, solver_type, pre) as s:
        if name.startswith("generic"):
            assert s.info().kernel_path == hip.PATH_GENERIC
        elif name in ("schur", "cgnr", "strip", "camera width 6"):
            assert s.info().kernel_path == hip.PATH_BAL
        sentinel(s, bs)
        scale = column_scale(bs) if with_scale else None
        hv, hb = session(s, bs, p.values, p.b, every_seventh_unannounced(runs_of(bs)), scale=scale)
        early, late, k = s.stream_stats()
        print(f"{name}: value streams {k}, {early} bytes early, {late} late")
        assert k == image.value_streams(bs) == streams
        if k == 0:   # nothing goes up by rows: values_end sends both arrays whole
            assert early == 0 and late == 8 * (bs.values_extent() + bs.num_rows)
        else:        # every run sends exactly its cells and its residuals (tests/test_value_streams_cpu.py), early or late
            assert early > 0 and late > 0 and early + late == all_bytes(bs)
        check_image(s, bs, hv, hb, scale)


@pytest.mark.parametrize("with_scale", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("mode", ["every row last first", "one call", "nothing announced", "empty calls"])
def test_granularity_edges(hip, problems, mode, with_scale):
    """(with a scale too: ceres_hip_values_end must scale whether or not it had rows of its own to send)"""
    p = problems.synthetic_bal(None, layout="schur", **SMALL)
    bs, n = p.bs, p.bs.num_row_blocks
    plan = {"every row last first": [(0, n, [(r, 1) for r in reversed(range(n))])],
            "one call": [(0, n, [(0, n)])],
            "nothing announced": [(0, n, [])],
            # ceres_hip_values_ready(r, 0) is a no-op for any r: row 3 can still be announced afterwards
            "empty calls": [(0, n, [(3, 0), (n, 0), (0, 3), (3, 1), (4, n - 4), (n - 1, 0)])]}[mode]
    with make(hip, p, 5, 2) as s:
        sentinel(s, bs)
        scale = column_scale(bs) if with_scale else None
        hv, hb = session(s, bs, p.values, p.b, plan, n_threads=1, scale=scale)
        early, late, k = s.stream_stats()
        assert k == 2
        assert (early, late) == ((0, all_bytes(bs)) if mode == "nothing announced" else (all_bytes(bs), 0))
        check_image(s, bs, hv, hb, scale)


def plain_step(hip, p, values, b, solver_type=5, pre=2):
    with make(hip, p, solver_type, pre) as fresh:
        return fresh.lm_compute_step(values, b, 1e4, 0.1)


def test_back_to_back_iterations_on_one_handle(hip, problems):
    """streamed -> step -> streamed with other values -> step -> plain lm_compute_step -> streamed again: after every upload the image
    is the host's and the step is a fresh handle's plain step on the same values (same(): the module's 1e-12, for the reason given at its
    top).  The second upload differs from the first in EVERY entry and by sign: no stale byte can pass."""
    p = problems.synthetic_bal(None, layout="schur", **MID)
    bs = p.bs
    wave = 1.5 + 0.4 * np.cos(np.arange(p.values.shape[0]))
    ripple = 1.25 + 0.2 * np.sin(np.arange(p.b.shape[0]))
    assert (p.values != 0).all() and (p.b != 0).all()
    rounds = [("streamed", p.values, p.b), ("streamed", -p.values * wave, -p.b * ripple), ("plain", p.values * wave[::-1], p.b * ripple[::-1]),
              ("streamed", -p.values, p.b * ripple)]
    with make(hip, p, 5, 2) as s:
        sentinel(s, bs)
        for i, (how, values, b) in enumerate(rounds):
            step0, summ0, mcc0 = plain_step(hip, p, values, b)
            if how == "streamed":
                hv, hb = session(s, bs, values, b, every_seventh_unannounced(runs_of(bs, seed=20 + i)))
                check_image(s, bs, hv, hb)
                step, summ, mcc = s.lm_compute_step(None, None, 1e4, 0.1, values_unchanged=True)
            else:
                step, summ, mcc = s.lm_compute_step(values, b, 1e4, 0.1)
            check_image(s, bs, values, b)   # (the step leaves the loaded values as they are)
            assert summ.termination_type == hip.SUCCESS and summ.num_iterations == summ0.num_iterations, (i, how)
            assert same(step, step0) and same(mcc, mcc0), (i, how)


@pytest.mark.parametrize("solver_type,pre,scene", [(5, 2, "MID"), (6, 1, "MID"), (3, 1, "SMALL")], ids=["iterative_schur", "cgnr", "dense_schur"])
def test_the_linear_solver_entry_after_a_streamed_upload(hip, problems, solver_type, pre, scene):
    """ceres_hip_solve_unchanged_values (LinearSolver::Solve, not the LM entry) on streamed values = ceres_hip_solve on a fresh handle."""
    p = problems.synthetic_bal(None, layout="cgnr" if solver_type == 6 else "schur", **{"MID": MID, "SMALL": SMALL}[scene])
    bs = p.bs
    per_solve = hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=0.1)
    with make(hip, p, solver_type, pre) as fresh:
        x0, summ0 = fresh.solve(p.values, p.b, per_solve)
    assert summ0.termination_type == hip.SUCCESS and np.isfinite(x0).all()
    with make(hip, p, solver_type, pre) as s:
        sentinel(s, bs)
        hv, hb = session(s, bs, p.values, p.b, every_seventh_unannounced(runs_of(bs)))
        check_image(s, bs, hv, hb)
        x, summ = s.solve_unchanged_values(per_solve)
        assert summ.termination_type == hip.SUCCESS and summ.num_iterations == summ0.num_iterations
        assert same(x, x0)


def test_the_caller_may_reuse_its_arrays_when_values_end_has_returned(hip, problems):
    """Nothing announced: every byte is enqueued inside ceres_hip_values_end, from pinned memory.  The arrays are overwritten the moment
    it returns; the device must hold what they held (ceres_hip_values_end waits for its copies on the host)."""
    p = problems.synthetic_bal(None, layout="schur", **BIG)
    bs = p.bs
    with make(hip, p, 5, 2) as s:
        sentinel(s, bs)

        def overwrite(hv, hb):
            hv.fill(np.nan)
            hb.fill(np.nan)
        hv, hb = session(s, bs, p.values, p.b, [(0, bs.num_row_blocks, [])], n_threads=1, after_end=overwrite)
        assert np.isnan(hv).all() and np.isnan(hb).all()
        assert s.stream_stats() == (0, all_bytes(bs), 2)
        check_image(s, bs, p.values, p.b)


def test_the_ceres_order_end_then_scale_the_host_copy(hip, problems):
    """TrustRegionMinimizer scales its Jacobian in place right behind the evaluation (internal/ceres/trust_region_minimizer.cc:263-279).
    With the streamed upload that comes AFTER ceres_hip_values_end(scale): the rows nobody announced go up unscaled
    inside it and are scaled once, on the device.  The step is the plain step on the host-scaled values."""
    p = problems.synthetic_bal(None, layout="schur", **MID)
    bs = p.bs
    scale = column_scale(bs)
    extent = bs.values_extent()
    mask, col = image.cell_mask(bs, extent), image.column_of_value(bs, extent)

    def scale_in_place(hv, hb):
        hv[mask] *= scale[col[mask]]
    with make(hip, p, 5, 2) as s:
        sentinel(s, bs)
        hv, hb = session(s, bs, p.values, p.b, every_seventh_unannounced(runs_of(bs)), scale=scale, after_end=scale_in_place)
        early, late, _ = s.stream_stats()
        assert early > 0 and late > 0
        check_image(s, bs, p.values, p.b, scale)
        check_image(s, bs, hv, hb)                      # the same thing: the host's copy is now the scaled Jacobian, bit for bit
        step, summ, mcc = s.lm_compute_step(None, None, 1e4, 0.1, values_unchanged=True)
    step0, summ0, mcc0 = plain_step(hip, p, np.array(hv), np.array(hb))
    assert summ.termination_type == hip.SUCCESS and summ.num_iterations == summ0.num_iterations and same(step, step0) and same(mcc, mcc0)


def test_entry_points_are_refused_while_a_session_is_open(hip, problems):
    """Between values_begin and values_end the device copy is half written while the handle still counts as loaded (here: the sentinel):
    whatever reads or replaces the loaded values is an error, and the open session survives it."""
    p = problems.synthetic_bal(None, layout="schur", **SMALL)
    bs, n = p.bs, p.bs.num_row_blocks
    other_v, other_b = pinned(bs.values_extent()), pinned(bs.num_rows)
    other_v[:] = 2.0 * p.values
    other_b[:] = 2.0 * p.b
    per_solve = hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=0.1)
    with make(hip, p, 5, 2) as s:
        sentinel(s, bs)
        hv, hb = pinned(bs.values_extent()), pinned(bs.num_rows)
        hv.fill(np.nan)
        hb.fill(np.nan)
        fill = row_filler(bs, hv, hb, p.values, p.b)
        s.values_begin(hv, hb)
        half = n // 2
        fill(0, half)
        s.values_ready(0, half)
        refused = {"load": lambda: s.load(other_v, other_b),
                   "solve": lambda: s.solve(other_v, other_b, per_solve),
                   "solve_unchanged_values": lambda: s.solve_unchanged_values(per_solve),
                   "lm_compute_step": lambda: s.lm_compute_step(other_v, other_b, 1e4, 0.1),
                   "lm_compute_step, values_unchanged": lambda: s.lm_compute_step(None, None, 1e4, 0.1, values_unchanged=True),
                   "scale_columns": lambda: s.scale_columns(np.full(bs.num_cols, 2.0)),
                   "jtb": s.jtb,
                   "values_begin": lambda: s.values_begin(other_v, other_b)}
        for name, call in refused.items():
            with pytest.raises(hip.HipError, match="between ceres_hip_values_begin and ceres_hip_values_end"):
                call()
                pytest.fail(f"{name} went through while a streamed upload was open")
        # the session is as it was: the rest goes up (three rows left to values_end), from the arrays of the FIRST values_begin
        fill(half, n)
        s.values_ready(half + 3, n - half - 3)
        with pytest.raises(hip.HipError):
            s.values_ready(0, 1)                      # (still remembered as announced)
        s.values_end()
        early, late, k = s.stream_stats()
        assert k == 2 and late > 0 and early + late == all_bytes(bs)
        check_image(s, bs, hv, hb)
        step, summ, mcc = s.lm_compute_step(None, None, 1e4, 0.1, values_unchanged=True)
    step0, summ0, mcc0 = plain_step(hip, p, p.values, p.b)
    assert summ.num_iterations == summ0.num_iterations and same(step, step0) and same(mcc, mcc0)
