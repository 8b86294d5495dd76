"""Shared camera intrinsics of the BAL front end without a GPU: the restatement (tests/shared_intrinsics_reference.py) against the
problem it wraps (tests/frontend_reference.py), what ceres_hip_bal_create_with_shared_intrinsics refuses before any device call, the
conditioning of every case the GPU tests compare trajectories on (tests/shared_intrinsics_cases.py), and the scene of the GPU test of
the parameter-tolerance test's |x|."""
import ctypes

import numpy as np
import pytest

import frontend_reference as F
import shared_intrinsics_cases as C
import shared_intrinsics_reference as SI
from conftest import pkg
from test_gpu_frontend_matrix import LOSS_PARAMS, NAMES, tolerances

hs = pkg.hip_solver
HUBER = ("huber",) + LOSS_PARAMS["huber"] + (1.0,)


@pytest.fixture(scope="module")
def scenes(oracle):
    return C.scenes(oracle)


def test_table_gives_every_layout_every_level():
    """The coverage of the GPU table and the cap on excused cases (as tests/test_gpu_fixed_intrinsics.py caps them: one in eight, and
    only table cases)."""
    assert len(set(C.TABLE)) == len(C.TABLE)
    for layout in C.LAYOUTS:
        mine = [e for e in C.TABLE if e[0] == layout]
        cases = [dict(zip(NAMES, e[2])) for e in mine]
        for solver in C.FACTORS[0][1]:
            assert any(c["solver"] == solver for c in cases), (layout, solver)
        for strategy in C.FACTORS[1][1]:
            assert any(c["strategy"] == strategy for c in cases), (layout, strategy)
        for generic in (0, 1):
            assert any(c["generic"] == generic for c in cases), (layout, generic)
        for loss in C.FACTORS[3][1]:
            assert any(c["loss"] == loss for c in cases), (layout, loss)
        for jacobi in (1, 0):
            assert any(c["jacobi"] == jacobi for c in cases), (layout, jacobi)
        for constant in SI.CONSTANT_SETS:
            assert any(e[1] == constant for e in mine), (layout, constant)
    for e in C.TABLE:
        c = dict(zip(NAMES, e[2]))
        assert c["camera"] == "angle_axis" and c["inner"] is None and c["tiles"] is None and c["inner_form"] is None
        assert c["strategy"] == "lm" or c["solver"] == (3, 0)
    ids = {C.si_id(e) for e in C.TABLE}
    assert set(C.EDGE_ILL_CONDITIONED) <= ids
    assert 8 * len(C.EDGE_ILL_CONDITIONED) <= len(C.TABLE), (len(C.EDGE_ILL_CONDITIONED), len(C.TABLE))


def test_layouts_and_constant_sets():
    for nc in (10, 66):
        assert SI.layout("one", nc).max() == 0 and SI.layout("three", nc).max() == 2 and SI.layout("each", nc).max() == nc - 1
        two, single = SI.layout("two", nc), SI.layout("two_single", nc)
        assert two.tolist() == [c % 2 for c in range(nc)] and np.flatnonzero(single == 1).tolist() == [1]
        for name in SI.LAYOUTS:
            g = SI.layout(name, nc)
            k = SI.constant_cameras("two", g)
            assert k.size == 2 and k[0] == 0 and (name == "each" or g[k[0]] == g[k[1]])   # the two in one group
            assert SI.constant_cameras("camera0", g).tolist() == [0] and SI.constant_cameras("none", g).size == 0


@pytest.mark.parametrize("loss", [None, HUBER], ids=["squared", "huber"])
@pytest.mark.parametrize("scene", ["clean", "edge"])
def test_a_group_per_camera_is_the_wrapped_problem(oracle, scenes, scene, loss):
    """num_groups == num_cameras: the wrapped problem up to a column permutation — evaluate bit-equal after permuting, and the
    8-iteration LM trajectory the same to 1e-9 in every cost."""
    sc = scenes[scene]
    nc, npts = sc[0], sc[1]
    w, x0, xc, groups, _ = C.reference(oracle, sc, "each", "none", loss)
    assert np.array_equal(x0, C.ambient_state(sc)) and w.n == w.inner.n and np.array_equal(w.expand(xc), x0)
    assert np.array_equal(w.scene[4], sc[4])   # (nothing shared: no pixel moves)
    cost_i, r_i, vals_i, g_i = w.inner.evaluate(x0)
    cost, r, vals, g = w.evaluate(xc)
    perm = w.amb_col   # ambient column -> compact column, a permutation here
    assert np.array_equal(np.sort(perm), np.arange(w.n))
    assert cost == cost_i and np.array_equal(r, r_i) and np.array_equal(g[perm], g_i)
    J_i, J = w.inner.dense_jacobian(vals_i), w.dense_jacobian(vals)
    assert np.array_equal(J[:, perm], J_i)
    # the values: E cells as they were; per row the pose cell (2 x 6) then the group cell (2 x 3) of the wrapped 2 x 9 cell
    n = w.n_rows
    assert vals.size == 24 * n and np.array_equal(vals[:6 * n], vals_i[:6 * n])
    cells, cells_i = vals[6 * n:].reshape(n, 18), vals_i[6 * n:].reshape(n, 2, 9)
    assert np.array_equal(cells[:, :12].reshape(n, 2, 6), cells_i[:, :, :6]) and np.array_equal(cells[:, 12:].reshape(n, 2, 3), cells_i[:, :, 6:])
    xa, Sa = F.minimize(w.inner, x0, "lm", max_num_iterations=8)
    xb, Sb = F.minimize(w, xc, "lm", max_num_iterations=8)
    assert len(Sa["iterations"]) == len(Sb["iterations"]) >= 3
    for a, b in zip(Sa["iterations"], Sb["iterations"]):
        assert (a["step_is_successful"], a["step_is_valid"]) == (b["step_is_successful"], b["step_is_valid"])
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * abs(a["cost"])
    assert Sb["final_cost"] < Sb["initial_cost"]


@pytest.mark.parametrize("layout,constant", [("one", "none"), ("two", "two"), ("two_single", "camera0"), ("three", "two")])
def test_jacobian_is_the_ambient_one_times_P(oracle, scenes, layout, constant):
    """The group's columns are the sums of its cameras' intrinsics columns, a constant camera's pose columns are gone; the gradient is
    J^T r, and with respect to a group's intrinsics it equals central differences of the cost on the compact state to 1e-6."""
    sc = scenes["edge"]
    nc, npts = sc[0], sc[1]
    w, x0, xc, groups, const = C.reference(oracle, sc, layout, constant, HUBER)
    ng = int(groups.max()) + 1
    nfc = nc - const.size
    assert w.n == 3 * npts + 6 * nfc + 3 * ng and xc.size == w.n
    cost_i, r_i, vals_i, g_i = w.inner.evaluate(x0)
    cost, r, vals, g = w.evaluate(xc)
    assert cost == cost_i and np.array_equal(r, r_i)
    J_i, J = w.inner.dense_jacobian(vals_i), w.dense_jacobian(vals)
    assert J.shape == (r.size, w.n)
    assert np.array_equal(J[:, :3 * npts], J_i[:, :3 * npts])
    for k, c in enumerate(w.free_cams):
        assert np.array_equal(J[:, 3 * npts + 6 * k:3 * npts + 6 * k + 6], J_i[:, 3 * npts + 9 * c:3 * npts + 9 * c + 6])
    for gid in range(ng):
        cols = [3 * npts + 9 * c + 6 + np.arange(3) for c in np.flatnonzero(groups == gid)]
        want = sum(J_i[:, cc] for cc in cols)   # (the cameras of a group share no row: one non-zero term per entry)
        assert np.array_equal(J[:, 3 * npts + 6 * nfc + 3 * gid:3 * npts + 6 * nfc + 3 * gid + 3], want)
    # the values: 6 per E cell, then per row 12 + 6 (a free camera) or 6 (a constant one)
    n_const_rows = int(np.count_nonzero(np.isin(w.row_cam, const)))
    assert vals.size == 6 * w.n_rows + 18 * (w.n_rows - n_const_rows) + 6 * n_const_rows
    assert np.allclose(J.T @ r, g, rtol=1e-12, atol=1e-12 * np.abs(g).max())
    assert w.gradient_max_norm(xc, g) == float(np.max(np.abs(g)))
    # central differences of the cost over every group's three entries, on the squared loss (a smooth cost): the group's gradient as
    # a vector, relative to its norm
    w2, _, xc2, _, _ = C.reference(oracle, sc, layout, constant, None)
    g2 = w2.evaluate(xc2)[3]
    for gid in range(ng):
        at = 3 * npts + 6 * nfc + 3 * gid
        fd = np.zeros(3)
        for j in range(3):
            h = 1e-5 * max(1e-2, abs(xc2[at + j]))
            e = np.zeros(w2.n)
            e[at + j] = h
            # cost(x + e) - cost(x - e) = 1/2 sum (r+ - r-)(r+ + r-), summed in that form: the two costs agree to their first ten
            # digits, and their rounding alone would leave a small group's gradient (camera 1 on its own) three digits
            rp, rm = w2.evaluate(xc2 + e)[1], w2.evaluate(xc2 - e)[1]
            fd[j] = 0.5 * float(np.dot(rp - rm, rp + rm)) / (2.0 * h)
        err = np.linalg.norm(fd - g2[at:at + 3]) / np.linalg.norm(g2[at:at + 3])
        print(layout, constant, "group", gid, "central differences", fd, "gradient", g2[at:at + 3], "relative", err)
        assert err <= 1e-6, (gid, fd, g2[at:at + 3])


@pytest.mark.parametrize("layout", list(SI.LAYOUTS))
def test_expand_after_plus_keeps_groups_bit_identical(oracle, scenes, layout):
    sc = scenes["clean"]
    nc, npts = sc[0], sc[1]
    w, x0, xc, groups, const = C.reference(oracle, sc, layout, "two", None)
    assert w.groups_identical(x0) and np.array_equal(w.compact(w.expand(xc)), xc)
    d = np.random.default_rng(5).normal(size=w.n)
    x1 = w.expand(w.plus(xc, d))
    assert w.groups_identical(x1)
    assert np.array_equal(x1[w.constant_state].view(np.int64), x0[w.constant_state].view(np.int64)) and w.constant_state.size == 6 * const.size
    moved = np.ones(x0.size, bool)
    moved[w.constant_state] = False
    assert np.all(x1[moved] != x0[moved])
    bad = x1.copy()
    bad[3 * npts + 9 * (nc - 1) + 7] = np.nextafter(bad[3 * npts + 9 * (nc - 1) + 7], np.inf)
    assert w.groups_identical(bad) == (layout == "each")   # (a camera alone in its group has nobody to differ from)
    x, S = F.minimize(w, xc, "lm", max_num_iterations=4)
    assert S["final_cost"] < S["initial_cost"] and w.groups_identical(w.expand(x))


@pytest.mark.parametrize("scene", ["clean", "edge"])
def test_which_layouts_the_tile_plan_takes(oracle, scenes, scene):
    """The program's block structure through the host-side tile plan (no device): one or two groups fit the shared strip of the fused
    <2,3,6> kernels — with constant cameras, whose rows have no camera cell —, three groups (nine shared scalars) do not."""
    sc = scenes[scene]
    BS = pkg.block_structure.BlockStructure
    for layout, constant, eligible in (("one", "none", True), ("one", "two", True), ("two", "none", True), ("two", "camera0", True),
                                       ("three", "none", False), ("three", "two", False)):
        w, _, _, _, _ = C.reference(oracle, sc, layout, constant, None)
        sizes, rows = w.structure()
        assert sum(2 * {3: 3, 6: 6}[sizes[b]] for _, cells in rows for b, _ in cells) == w.n_values
        plan = hs.debug_plan(BS.from_rows(sizes, rows), sc[1])
        assert plan["eligible"] == eligible, (layout, constant, plan.get("why"))
        if eligible:   # the plan's cameras are the free cameras' 6-wide poses and nothing else: the groups went to the shared strip
            cams = plan["slot_cam"][plan["valid"] == 1]
            assert cams[cams >= 0].max() + 1 == w.nfc and all(s == 6 for s in sizes[sc[1]:sc[1] + w.nfc])
            assert np.count_nonzero(cams < 0) == np.count_nonzero(~w.row_has_pose)   # (a constant camera's rows: no camera cell)
        if not eligible:
            assert "shared strip" in plan["why"]


def test_python_arguments(scenes):
    nc, npts, cam, pt, obs, _ = scenes["clean"]
    o = hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI)
    groups = np.zeros(nc, np.int32)
    for kw in (dict(constant_intrinsics=["f"]), dict(constant_points=[3])):
        with pytest.raises(ValueError, match="camera_groups cannot be combined"):
            hs.BalProblem(o, nc, npts, cam, pt, obs, camera_groups=groups, **kw)
    with pytest.raises(ValueError, match="one entry per camera"):
        hs.BalProblem(o, nc, npts, cam, pt, obs, camera_groups=groups[:-1])


def test_creator_refuses_before_any_device_call(scenes):
    """What ceres_hip_bal_create_with_shared_intrinsics refuses, it refuses before any device call: the same messages with and without
    a GPU."""
    nc, npts, cam, pt, obs, _ = scenes["clean"]
    o = hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI)
    fn = "ceres_hip_bal_create_with_shared_intrinsics: "
    lib = hs.load_library()
    c = hs.COptions(o.type, o.preconditioner_type, o.min_num_iterations, o.max_num_iterations, o.residual_reset_period, npts, o.device,
                    int(o.force_generic_path), o.cg_check_interval, o.jacobian_storage, o.max_num_spse_iterations,
                    int(o.use_spse_initialization), o.spse_tolerance, int(o.use_explicit_schur_complement), int(o.visibility_clustering_type))
    u8p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    flat = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1)

    def raw(model, groups, num_groups, constant=None, camera=cam):
        g = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        k = None if constant is None else np.ascontiguousarray(constant, dtype=np.uint8)
        h = lib.ceres_hip_bal_create_with_shared_intrinsics(ctypes.byref(c), model, nc, npts, cam.shape[0], i32(camera), i32(pt), hs._p(flat),
                                                            None if k is None else u8p(k), None if g is None else i32(g), num_groups)
        if h:
            lib.ceres_hip_bal_destroy(h)
            return None
        return lib.ceres_hip_bal_last_error(None).decode()

    zeros = np.zeros(nc, np.int32)
    for model in (hs.CAMERA_QUATERNION, hs.CAMERA_QUATERNION_MANIFOLD):
        msg = raw(model, zeros, 1)
        assert fn in msg and "angle-axis camera only" in msg and "shared intrinsics" in msg
    for ng in (0, -3, nc + 1):
        assert fn + f"num_groups {ng} is not in [1, num_cameras = {nc}]" in raw(0, zeros, ng)
    bad = zeros.copy()
    bad[4] = 2
    assert fn + "camera 4 has group 2, not in [0, 2)" in raw(0, bad, 2)
    bad[4] = -1
    assert fn + "camera 4 has group -1, not in [0, 2)" in raw(0, bad, 2)
    assert fn + "group 1 has no camera" in raw(0, zeros, 2)
    skip = zeros.copy()
    skip[5:] = 2
    assert fn + "group 1 has no camera" in raw(0, skip, 3)
    # what ceres_hip_bal_create_with_constant_blocks refuses, under the new creator's name
    assert fn + "every camera is constant" in raw(0, zeros, 1, constant=np.ones(nc))
    assert fn + "unknown camera_model 7" in raw(7, zeros, 1)
    off = cam.copy()
    off[0] = nc
    assert fn + "observation index out of range" in raw(0, zeros, 1, camera=off)
    assert not lib.ceres_hip_bal_create_with_shared_intrinsics(None, 0, 0, 0, 0, None, None, None, None, None, 0)
    assert "bad arguments" in lib.ceres_hip_bal_last_error(None).decode()
    # no grouping: the constant-block creator's path, messages included
    assert "ceres_hip_bal_create_with_constant_blocks: every camera is constant" in raw(0, None, 0, constant=np.ones(nc))
    # through the Python class: the library's refusals
    for groups, text in ((np.full(nc, -1), "num_groups 0 is not in"), (np.arange(nc) * 2, "num_groups"), ([0] * (nc - 1) + [2], "group 1 has no camera")):
        with pytest.raises(hs.HipError) as e:
            hs.BalProblem(o, nc, npts, cam, pt, obs, camera_groups=groups)
        assert fn in str(e.value) and text in str(e.value), str(e.value)
    with pytest.raises(hs.HipError) as e:
        hs.BalProblem(o, nc, npts, cam, pt, obs, camera_groups=zeros, camera_model="quaternion")
    assert fn in str(e.value) and "angle-axis camera only" in str(e.value)
    # valid groups are accepted and the call gets as far as the device
    if hs.device_count() == 0:
        msg = raw(0, np.arange(nc) % 2, 2, constant=(np.arange(nc) < 2))
        assert msg is not None and ("no HIP device" in msg or "no CPU fallback" in msg), msg


@pytest.mark.parametrize("entry", C.TABLE, ids=C.si_id)
def test_every_table_case_is_well_conditioned(oracle, scenes, entry):
    """fixed_intrinsics_reference.conditioning's method on every GPU table case, on both scenes: 100 x the deviation within the case's
    cost tolerance and no flag changed — the restatement alone keeps every case inside the rule, so the GPU table excuses none."""
    from fixed_intrinsics_reference import conditioning
    layout, constant, case = entry
    c = dict(zip(NAMES, case))
    cost_tol = tolerances(case)[0]
    for scene in ("clean", "edge"):
        w, _, xc, _, _ = C.reference(oracle, scenes[scene], layout, constant, C.loss_of(case))
        dev, flags = conditioning(w, xc, c["strategy"], jacobi_scaling=c["jacobi"])
        print(C.si_id(entry), scene, "deviation %.2e" % dev, "flags", flags, "tolerance", cost_tol)
        assert flags == 0
        assert 100.0 * dev <= cost_tol, (scene, dev, cost_tol)
    assert C.si_id(entry) not in C.EDGE_ILL_CONDITIONED and C.edge_values_compared(entry) == (c["strategy"] != "lm" or c["solver"] in ((5, 2), (3, 0)))


def norm_scene(oracle):
    """The scene of the |x| test (test_gpu_shared_intrinsics.test_parameter_tolerance_counts_a_group_once): the clean scene with ONE
    group, camera 0 constant and the intrinsics scaled (f and the pixels times 4: the same geometry, residuals times 4), so that f — ten
    times in the ambient state, once in the program — is nearly all of |x|.  Returns (scene, parameter_tolerance, the iteration the
    restatement's parameter-tolerance test ends at, the earlier iteration it would end at if |x| ran over the ambient state)."""
    nc, npts, cam, pt, obs, par = C.scenes(oracle)["clean"]
    par = par.copy()
    par[:9 * nc].reshape(nc, 9)[:, 6] *= 4.0
    sc = (nc, npts, cam, pt, 4.0 * obs, par)
    w, x0, xc, _, _ = C.reference(oracle, sc, "one", "camera0", None)
    log = []
    plus = w.plus

    def recording_plus(x, d):
        log.append((float(np.linalg.norm(d)), float(np.linalg.norm(x)), float(np.linalg.norm(np.delete(w.expand(x), w.constant_state)))))
        return plus(x, d)
    w.plus = recording_plus
    off = dict(function_tolerance=0.0, gradient_tolerance=0.0)
    _, S = F.minimize(w, xc, "lm", max_num_iterations=12, parameter_tolerance=0.0, **off)
    assert all(it["step_is_valid"] for it in S["iterations"]) and len(log) == len(S["iterations"]) - 1
    ratio_c, ratio_a = [d / a for d, a, _ in log], [d / b for d, _, b in log]
    # iteration k + 1 (log entry k), after a success: the ambient |x| would end the run there, the program's |x| one iteration later
    for k in range(1, len(log) - 1):
        lo, hi = max(ratio_a[k], ratio_c[k + 1]), ratio_c[k]
        if hi >= 2.0 * lo and min(ratio_a[:k]) > hi and S["iterations"][k]["step_is_successful"] and S["iterations"][k + 1]["step_is_successful"]:
            return sc, float(np.sqrt(lo * hi)), k + 2, k + 1
    raise AssertionError((ratio_c, ratio_a))


def test_parameter_tolerance_scene_tells_the_countings_apart(oracle):
    """With the restatement first: at the chosen tolerance its run ends by the parameter-tolerance test at the iteration norm_scene
    names, a factor >= sqrt 2 inside on both sides, where the ambient |x| would have ended it one iteration earlier."""
    sc, tol, ends_at, ambient_ends_at = norm_scene(oracle)
    assert ambient_ends_at == ends_at - 1 >= 2
    w, x0, xc, _, _ = C.reference(oracle, sc, "one", "camera0", None)
    cams = x0[3 * sc[1]:].reshape(sc[0], 9)
    assert np.linalg.norm(cams[0, 6:]) > 0.9 * np.linalg.norm(xc)   # f is nearly all of |x|
    _, S = F.minimize(w, xc, "lm", max_num_iterations=12, parameter_tolerance=tol, function_tolerance=0.0, gradient_tolerance=0.0)
    assert S["termination_type"] == F.CONVERGENCE and len(S["iterations"]) == ends_at + 1
    last = S["iterations"][-1]
    assert not last["step_is_successful"] and "relative_decrease" not in last   # (ended before the step was judged)
